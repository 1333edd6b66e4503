"""SVDLinear / QRLinear off the GPU: API, reference checkpoints, the dense weights against the reference's fixtures and the
C ABI of the fused Householder-diagonal-Householder entries."""
import ctypes
import inspect
import os
import re

import pytest
import torch

import _linear_family_util as U
from flowconductor_amd import _hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["fc_hdh_linear", "fc_hdh_linear_backward"]


def test_imports_and_constructor_defaults():
    import flowconductor_amd.transforms as T
    from flowconductor_amd.transforms.linear import Linear

    svd = inspect.signature(T.SVDLinear.__init__).parameters
    assert list(svd)[1:] == ["features", "num_householder", "using_cache", "identity_init", "eps"]
    assert (svd["using_cache"].default, svd["identity_init"].default, svd["eps"].default) == (False, True, 1e-3)
    assert svd["num_householder"].default is inspect.Parameter.empty
    qr = inspect.signature(T.QRLinear.__init__).parameters
    assert list(qr)[1:] == ["features", "num_householder", "using_cache"]
    assert qr["using_cache"].default is False and qr["num_householder"].default is inspect.Parameter.empty
    assert issubclass(T.SVDLinear, Linear) and issubclass(T.QRLinear, Linear)
    assert T.SVDLinear._HIP_AUTOGRAD and T.QRLinear._HIP_AUTOGRAD
    m = T.SVDLinear(6, 4)
    assert isinstance(m.orthogonal_1, T.HouseholderSequence) and isinstance(m.orthogonal_2, T.HouseholderSequence)
    assert m.orthogonal_1.q_vectors.shape == (4, 6) and m.unconstrained_diagonal.shape == (6,)
    assert set(m.state_dict()) == U.STATE_KEYS["svd"]
    q = T.QRLinear(6, 3)
    assert isinstance(q.orthogonal, T.HouseholderSequence) and q.upper_entries.shape == (15,) and q.log_upper_diag.shape == (6,)
    assert set(q.state_dict()) == U.STATE_KEYS["qr"]


def test_odd_num_householder_is_refused():
    import flowconductor_amd.transforms as T

    with pytest.raises(AssertionError):
        T.SVDLinear(6, 3)
    T.QRLinear(6, 3)       # the QR form takes any count


@pytest.mark.parametrize("d,k", [(1, 2), (5, 2), (64, 8)])
def test_identity_initialisation(d, k):
    import flowconductor_amd.transforms as T

    m = T.SVDLinear(d, k)
    eye = torch.eye(d)
    with torch.no_grad():
        assert float((m.weight() - eye).abs().max()) <= 1e-6
        assert float((m.weight_inverse() - eye).abs().max()) <= 1e-6
        assert float(m.logabsdet().abs()) <= 1e-6 * d
        assert float((m.diagonal - 1).abs().max()) <= 1e-6 and float(m.log_diagonal.abs().max()) <= 1e-6
    assert float(m.bias.abs().max()) == 0.0
    torch.manual_seed(3)
    r = T.SVDLinear(d, k, identity_init=False)
    bound = d ** -0.5
    assert float(r.unconstrained_diagonal.abs().max()) <= bound and float(r.unconstrained_diagonal.abs().max()) > 0
    q = T.QRLinear(d, k)
    assert float(q.log_upper_diag.abs().max()) <= bound and float(q.bias.abs().max()) == 0.0
    if d > 1:
        assert float(q.upper_entries.abs().max()) <= bound


@pytest.mark.parametrize("name", U.FIXTURES)
def test_reference_checkpoint_loads_and_dense_weights_match(name):
    """strict load of the reference's state_dict; ``x @ W.T + b`` and logabsdet on the CPU within 4 x the fixture's own
    float32 noise floor of the reference's float64 values; ``W W^-1 = I`` within 1e-4."""
    t, kind, d, k = U.fixture(name)
    module = U.build(name)
    assert set(module.state_dict()) == {key[4:] for key in t if key.startswith("sd::")} == U.STATE_KEYS[kind]
    with torch.no_grad():
        w, w_inv, lad = module.weight(), module.weight_inverse(), module.logabsdet()
        y = t["x"] @ w.T + module.bias
    assert w.shape == (d, d) and w.dtype == torch.float32 and w_inv.dtype == torch.float32 and lad.dim() == 0
    err_y = float((y.double() - t["y64"]).abs().max())
    err_lad = float((lad.double() - t["lad64"]).abs().max())
    err_eye = float((w.double() @ w_inv.double() - torch.eye(d, dtype=torch.float64)).abs().max())
    print(name, "y %.3g lad %.3g (floor %.3g) W W^-1 - I %.3g" % (err_y, err_lad, float(t["floor_fwd"]), err_eye))
    assert err_y <= 4 * float(t["floor_fwd"])
    assert err_lad <= 4 * float(t["floor_fwd"])
    assert err_eye <= 1e-4


def test_fixture_cases_are_the_issue_s():
    for name in U.FIXTURES:
        t, kind, d, k = U.fixture(name)
        assert os.path.getsize(os.path.join(U.GOLDEN, name + ".npz")) <= 1 << 20
        assert t["x"].shape == (257, d) and t["y32"].dtype == torch.float32 and t["grad_x64"].shape == (257, d)
        assert float(t["floor_fwd"]) > 0 and float(t["floor_inv"]) > 0
    assert float(U.fixture("svd_linear_d64_k64")[0]["sd::bias"].abs().max()) > 100      # the bias that must come off first


def test_weights_are_differentiable_and_composition_matches_on_cpu():
    """``weight()`` carries a graph to every parameter, and the torch composition (the route above
    ``ops.MAX_ROW_FEATURES`` features) is ``x @ W.T + b`` / its inverse."""
    for name in ("svd_linear_d5_k2", "qr_linear_d5_k3"):
        module = U.build(name)
        t = U.fixture(name)[0]
        module.weight().sum().backward()
        assert all(p.grad is not None for n, p in module.named_parameters() if n != "bias")
        with torch.no_grad():
            y = module._composition(t["x"], False)
            x_back = module._composition(y, True)
        assert float((y.double() - t["y64"]).abs().max()) <= 4 * float(t["floor_fwd"])
        assert float((x_back - t["x"]).abs().max()) <= 1e-4
    assert isinstance(U.build("qr_linear_d5_k3").weight_inverse(), torch.Tensor)      # identity on the parameters' device


@pytest.mark.parametrize("name", ENTRIES)
def test_entries_are_declared_bound_and_exported(name):
    assert name in _hip.SIGNATURES
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "flowcon_hip.h")).read(), flags=re.S)
    decl = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, header)
    assert decl is not None, "%s is not declared in include/flowcon_hip.h" % name
    assert len(decl.group(1).split(",")) == len(_hip.SIGNATURES[name])
    assert hasattr(ctypes.CDLL(_hip.LIB_PATH), name), "libflowcon_hip.so does not export %s" % name
    assert _hip.ABI_VERSION == 3
