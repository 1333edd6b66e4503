"""The per-sample backward off the GPU: the six conditional matrix layers reach the kernels' host-tensor check under
autograd (they used to refuse before it), the new ops names and C entries exist, and the written-out gradient formulas
the kernels implement (tests/_per_sample_backward_util.py) equal float64 autograd."""
import pytest
import torch

import _per_sample_backward_util as U
from flowconductor_amd import _hip, ops
from flowconductor_amd import transforms as T

CLASSES = {"lu": (T.ConditionalLUTransform, 5), "rotation": (T.ConditionalRotationTransform, 2),
           "orthogonal": (T.ConditionalOrthogonalTransform, 5), "svd": (T.ConditionalSVDTransform, 5),
           "planar": (T.ConditionalPlanarTransform, 5), "sylvester": (T.ConditionalSylvesterTransform, 5)}


def test_names_and_entries():
    assert T.ConditionalLUTransform._HIP_AUTOGRAD is True
    for name in ("linear_per_sample_autograd", "_LinearPerSampleFunction", "_HouseholderPerSampleFunction",
                 "_PlanarPerSampleFunction", "householder_autograd", "planar_autograd", "sylvester_autograd"):
        assert hasattr(ops, name), name
    for entry in ("fc_linear_per_sample_backward", "fc_householder_backward_per_sample", "fc_planar_backward_per_sample"):
        assert entry in _hip.SIGNATURES, entry
    assert _hip.ABI_VERSION == 3


@pytest.mark.parametrize("kind", sorted(CLASSES))
@pytest.mark.parametrize("inverse", [False, True])
def test_training_call_reaches_the_host_tensor_check(kind, inverse):
    """With autograd on, a CPU call gets as far as the kernels' own refusal of host tensors -- not the refusals of a
    layer without a backward."""
    cls, d = CLASSES[kind]
    if inverse and kind in ("planar", "sylvester"):      # no inverse: raises as before
        t = cls(d, 16, 4).train()
        with pytest.raises(NotImplementedError):
            t.inverse(torch.randn(8, d), torch.randn(8, 4))
        return
    torch.manual_seed(0)
    t = cls(d, 16, 4).train()
    x = torch.randn(8, d, requires_grad=True)
    with pytest.raises(RuntimeError) as err:
        (t.inverse if inverse else t)(x, torch.randn(8, 4))
    message = str(err.value)
    assert "the bijector kernels run on a HIP device only" in message
    assert "no backward kernel" not in message and "not available yet" not in message


def test_scale_non_diag_keeps_its_state_dict_key():
    t = T.ConditionalLUTransform(3, 8, 2)
    assert "scale_non_diag" in t.state_dict() and t.scale_non_diag.requires_grad


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
@pytest.mark.parametrize("n,d", [(7, 1), (6, 2), (5, 5), (3, 17)])
def test_linear_formulas_equal_float64_autograd(mode, n, d):
    x, m, gy, gl = (t.double() for t in U.linear_case(n, d, 100 + 10 * d + mode))
    gx, gm, gs = U.linear_truth(x, m, gy, gl, mode, torch.float64)
    first = U.linear_forward(x, m, mode, U.OFFDIAG_SCALE, U.EPS)[0] if mode == 3 else x
    fx, fm, fs = U.linear_backward_formula(first, gy, gl, m, mode)
    for got, want in ((fx, gx), (fm, gm), (fs, gs.reshape(-1))):
        assert float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("d,k", [(1, 2), (5, 5), (16, 3), (9, 11)])
def test_householder_formulas_equal_float64_autograd(d, k, reverse):
    gen = torch.Generator().manual_seed(7 * d + k)
    n = 6
    x, q, gy = (torch.randn(*s, generator=gen, dtype=torch.float64) for s in ((n, d), (n, k, d), (n, d)))
    gx, gq = U.autograd_grads(lambda a, b: U.householder_forward(a, b, reverse), (x, q), gy, None, torch.float64)
    y, _ = U.householder_forward(x, q, reverse)
    fx, fq = U.householder_backward_formula(y, gy, q, reverse)
    assert float((fx - gx).abs().max()) <= 1e-12 * max(1.0, float(gx.abs().max()))
    assert float((fq - gq).abs().max()) <= 1e-12 * max(1.0, float(gq.abs().max()))


@pytest.mark.parametrize("d", [1, 2, 7, 30])
def test_planar_formulas_equal_float64_autograd(d):
    gen = torch.Generator().manual_seed(d)
    n = 9
    x, w, u, gy = (torch.randn(n, d, generator=gen, dtype=torch.float64) for _ in range(4))
    b, gl = (torch.randn(n, generator=gen, dtype=torch.float64) for _ in range(2))
    want = U.autograd_grads(U.planar_forward, (x, w, u, b), gy, gl, torch.float64)
    got = U.planar_backward_formula(x, gy, gl, w, u, b)
    for g, r in zip(got, want):
        assert float((g - r).abs().max()) <= 1e-12 * max(1.0, float(r.abs().max()))
