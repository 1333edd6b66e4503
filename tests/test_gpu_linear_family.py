"""GPU: SVDLinear / QRLinear against the reference's fixtures, and the fused Householder-diagonal-Householder kernel
(fc_hdh_linear / fc_hdh_linear_backward) against float64 compositions of the oracle's reflections."""
import copy

import pytest
import torch

import _linear_family_util as U
from flowconductor_amd import ops
from oracle import torch_oracle as O

pytestmark = pytest.mark.gpu

# (d, ka, kb, n): one / several registers per lane, a partial last register, a narrow row, sequences shorter and longer than
# one register chunk, row counts that do not fill the last workgroup; (512, 40, 40) is past the LDS budget (q rows and
# gradient rows from global memory / registers), (200, 0, 3) has one sequence empty
SHAPES = [(2, 2, 2, 1), (5, 2, 4, 7), (64, 8, 8, 777), (65, 18, 18, 333), (130, 6, 6, 257), (512, 40, 40, 129), (200, 0, 3, 64)]


def maxdiff(a, b):
    return float((a.detach().cpu().double() - b.detach().cpu().double()).abs().max())


def operands(d, ka, kb, n, shifts):
    torch.manual_seed(1000 * d + 10 * ka + kb)
    x, gy = torch.randn(n, d), torch.randn(n, d)
    q_a, q_b = torch.randn(ka, d), torch.randn(kb, d)
    scale = torch.exp(0.5 * torch.randn(d))
    pre, post = (torch.randn(d), torch.randn(d)) if shifts else (None, None)
    return x, gy, q_a, q_b, scale, pre, post


def composed64(x, q_a, q_b, scale, pre, post, reverse):
    """The map in float64 from the oracle's reflections (orthogonal.py:144-171)."""
    v = x if pre is None else x - pre
    v = O.householder_apply(v, q_a.flip(0) if reverse else q_a) * scale
    v = O.householder_apply(v, q_b.flip(0) if reverse else q_b)
    return v if post is None else v + post


@pytest.mark.parametrize("name", U.FIXTURES)
def test_modules_match_reference_fixtures(name, device):
    """No-grad forward and inverse of the loaded checkpoint: outputs and logabsdet within 4 x the fixture's float32 noise
    floor of the reference's float64 values (the inverse is applied to the reference's float32 outputs)."""
    t, kind, d, k = U.fixture(name)
    module = U.build(name).to(device)
    with torch.no_grad():
        y, lad = module(t["x"].to(device))
        xinv, ladinv = module.inverse(t["y32"].to(device))
    errs = (maxdiff(y, t["y64"]), maxdiff(lad, t["lad64"]), maxdiff(xinv, t["xinv64"]), maxdiff(ladinv, t["ladinv64"]))
    print(name, "fwd y %.3g lad %.3g (floor %.3g) | inv x %.3g lad %.3g (floor %.3g)"
          % (errs[0], errs[1], float(t["floor_fwd"]), errs[2], errs[3], float(t["floor_inv"])))
    assert y.dtype == torch.float32 and lad.shape == (257,)
    assert errs[0] <= 4 * float(t["floor_fwd"]) and errs[1] <= 4 * float(t["floor_fwd"])
    assert errs[2] <= 4 * float(t["floor_inv"]) and errs[3] <= 4 * float(t["floor_inv"])


@pytest.mark.parametrize("shifts", [False, True])
@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("d,ka,kb,n", SHAPES)
def test_hdh_linear_kernel_matches_float64(d, ka, kb, n, reverse, shifts, device):
    """fc_hdh_linear against the float64 composition, at fc_householder's tolerance: 1e-5 max|y_ref| (ka + kb)."""
    x, _, q_a, q_b, scale, pre, post = operands(d, ka, kb, n, shifts)
    ref = composed64(*(None if v is None else v.double() for v in (x, q_a, q_b, scale, pre, post)), reverse)
    dev = [None if v is None else v.to(device) for v in (x, q_a, q_b, scale, pre, post)]
    with torch.no_grad(), ops.KernelTimer("fc_hdh_linear") as timer:
        y = ops.hdh_linear(*dev, reverse_a=reverse, reverse_b=reverse)
    assert len(timer.pairs) == 1
    err = maxdiff(y, ref)
    print((d, ka, kb, n), "err %.3g of %.3g" % (err, 1e-5 * float(ref.abs().max()) * (ka + kb)))
    assert err <= 1e-5 * float(ref.abs().max()) * (ka + kb)


@pytest.mark.parametrize("shifts", [False, True])
@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("d,ka,kb,n", SHAPES[1:])
def test_hdh_linear_backward_matches_float64_autograd(d, ka, kb, n, reverse, shifts, device):
    """fc_hdh_linear_backward (from the saved output) against float64 autograd of the composed map, at the tolerance of
    test_householder_backward_kernel_matches_float64_autograd: 2e-5 max|g_ref| (ka + kb) + 1e-5."""
    x, gy, *params = operands(d, ka, kb, n, shifts)
    leaves64 = [None if v is None else v.double().requires_grad_(True) for v in [x] + params]
    ref = composed64(*leaves64, reverse)
    (ref * gy.double()).sum().backward()
    leaves = [None if v is None else v.to(device).requires_grad_(True) for v in [x] + params]
    with ops.KernelTimer("fc_hdh_linear") as fwd, ops.KernelTimer("fc_hdh_linear_backward") as bwd:
        y = ops.hdh_linear_autograd(*leaves, reverse_a=reverse, reverse_b=reverse)
        assert type(y.grad_fn).__name__ == "_HDHLinearFunctionBackward"
        (y * gy.to(device)).sum().backward()
    assert len(fwd.pairs) == 1 and len(bwd.pairs) == 1
    assert maxdiff(y, ref) <= 1e-5 * float(ref.abs().max()) * (ka + kb)
    for got, want, name in zip(leaves, leaves64, ("x", "q_a", "q_b", "scale", "pre", "post")):
        if want is None or want.numel() == 0:
            continue
        bound = 2e-5 * float(want.grad.abs().max()) * (ka + kb) + 1e-5
        err = maxdiff(got.grad, want.grad)
        print((d, ka, kb, n), name, "err %.3g of %.3g" % (err, bound))
        assert got.grad.shape == want.grad.shape and err <= bound, name


def reflections(kind, k):
    return 2 * k if kind == "svd" else k


@pytest.mark.parametrize("name", U.FIXTURES)
def test_module_round_trip_and_training_gradients(name, device):
    """inverse(forward(x)) = x within 1e-5 max(1, |x|) K and logabsdets that cancel within 1e-5; in train mode the
    gradients of ``(y * gy).sum() + lad.sum()`` against the fixture's float64 gradients at the backward tolerance."""
    t, kind, d, k = U.fixture(name)
    kk = reflections(kind, k)
    module = U.build(name).to(device)
    x = t["x"].to(device)
    with torch.no_grad():
        y, lad = module(x)
        back, lad_back = module.inverse(y)
    assert maxdiff(back, x) <= 1e-5 * max(1.0, float(x.abs().max())) * kk
    assert float((lad + lad_back).abs().max()) <= 1e-5
    module.train()
    xg = x.clone().requires_grad_(True)
    y, lad = module(xg)
    if kind == "svd":
        assert type(y.grad_fn).__name__ == "_HDHLinearFunctionBackward"
    ((y * t["gy"].to(device)).sum() + lad.sum()).backward()
    got = dict(module.named_parameters())
    pairs = [("x", xg.grad, t["grad_x64"])] + [(key[8:], got[key[8:]].grad, v) for key, v in t.items() if key.startswith("grad64::")]
    assert len(pairs) == 5
    for pname, g, want in pairs:
        bound = 2e-5 * float(want.abs().max()) * kk + 1e-5
        err = maxdiff(g, want)
        print(name, pname, "err %.3g of %.3g" % (err, bound))
        assert err <= bound, pname
    # the inverse under autograd: one node as well, and it undoes the forward
    z, _ = module.inverse(y.detach().requires_grad_(True))
    if kind == "svd":
        assert type(z.grad_fn).__name__ == "_HDHLinearFunctionBackward"
    assert maxdiff(z, x) <= 1e-5 * max(1.0, float(x.abs().max())) * kk


@pytest.mark.parametrize("kind", ["svd", "qr"])
def test_wide_batches_take_the_matrix_core_route(kind, device):
    """d = 64, k = 8, n = 2048 + 5 without gradients: the folded weight through fc_dense_mm (fc_dense_mm_shifted for the
    inverse: the bias comes off first), the five tail rows through the row kernels; against the float64 composition at the
    tolerance of test_householder_and_lu_dense_matrix_core_path."""
    import flowconductor_amd.transforms as T

    d, k, n = 64, 8, 2048 + 5
    torch.manual_seed(17)
    module = (T.SVDLinear(d, k, identity_init=False) if kind == "svd" else T.QRLinear(d, k)).eval()
    with torch.no_grad():
        for p in module.parameters():
            p.add_(0.3 * torch.randn(p.shape))
    x = torch.randn(n, d)
    on_device = copy.deepcopy(module).to(device)
    for inverse in (False, True):
        with torch.no_grad():
            ref = copy.deepcopy(module).double()._composition(x.double(), inverse)
            f32 = module._composition(x, inverse)
        entry = "fc_dense_mm_shifted" if inverse else "fc_dense_mm"
        with torch.no_grad(), ops.KernelTimer(entry) as timer:
            y, lad = (on_device.inverse if inverse else on_device)(x.to(device))
        assert len(timer.pairs) == 1, "the matrix-core kernel did not run"
        scale = max(1.0, float(ref.abs().max()))
        assert maxdiff(y, ref) <= 1e-5 * scale + 4 * maxdiff(f32, ref)
        want_lad = float(module.logabsdet()) * (-1 if inverse else 1)
        assert float((lad.cpu() - want_lad).abs().max()) <= 1e-5 * max(1.0, abs(want_lad))


@pytest.mark.parametrize("name", ["svd_linear_d64_k64", "svd_linear_d130_k6", "qr_linear_d64_k16"])
def test_cached_eval_path_agrees_with_uncached(name, device):
    """``using_cache`` in eval mode (one fc_linear launch from weight() / weight_inverse()) against the uncached kernels.
    Both are float32 evaluations of the same map: the uncached one within 1e-5 max|y| K of it (the kernel tolerance above), the
    cached one a single product with a weight rounded once from float64, within 1e-5 max|y|; so 1e-5 max|y| (K + 1)."""
    t, kind, d, k = U.fixture(name)
    kk = reflections(kind, k)
    module = U.build(name).to(device)
    x = t["x"].to(device)
    with torch.no_grad():
        y, lad = module(x)
        back, lad_back = module.inverse(y)
        module.use_cache(True)
        with ops.KernelTimer("fc_linear") as timer:
            y_c, lad_c = module(x)
            back_c, lad_back_c = module.inverse(y)
        assert len(timer.pairs) == 2 and module.cache.weight is not None and module.cache.inverse is not None
    assert maxdiff(y_c, y) <= 1e-5 * float(y.abs().max()) * (kk + 1)
    assert maxdiff(back_c, back) <= 1e-5 * max(1.0, float(back.abs().max())) * (kk + 1)
    assert maxdiff(lad_c, lad) <= 1e-5 and maxdiff(lad_back_c, lad_back) <= 1e-5
