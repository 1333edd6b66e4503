"""RadialTransform / UnitVector / NaiveLinear on the GPU: the reference's fixtures, fresh shapes against the float64
restatements of tests/_rownorm_util.py, round trips, edges, the sphere check, gradients and the NaiveLinear routes.

Bounds: ``1e-5 scale + 4 floor`` (tests/test_gpu_golden.py:21-44) with the floor the reference's -- or, for fresh inputs, the
restatement's -- own float32-vs-float64 error on the same inputs; gradients ``1e-4 scale + 1e-5``
(test_planar_backward_kernel_matches_float64_autograd)."""
import pytest
import torch

import _rownorm_util as U
from _util import maxdiff
from flowconductor_amd import distributions, flows, ops
from flowconductor_amd import transforms as T

pytestmark = pytest.mark.gpu

ROWS = (1, 7, 257)


def _within(got, ref64, floor, what, mult=1.0, scale=None):
    scale = float(ref64.abs().max()) if scale is None else scale
    bound = mult * U.bound(scale, floor)
    err = maxdiff(got, ref64)
    print("%s err %.3g bound %.3g (floor %.3g)" % (what, err, bound, float(floor)))
    assert err <= bound, (what, "err %.3g > bound %.3g (floor %.3g)" % (err, bound, float(floor)))


def _grad_close(got, ref, what):
    scale = max(1e-5, float(ref.abs().max()))
    err = maxdiff(got.reshape(ref.shape), ref)
    print("%s grad err %.3g scale %.3g" % (what, err, scale))
    assert err <= 1e-4 * scale + 1e-5, (what, err, scale)


def _radial_module(d, seed, device=None):
    torch.manual_seed(seed)
    module = T.RadialTransform(d)
    with torch.no_grad():
        module.alpha.add_(0.5 * torch.randn(1))
        module.beta.add_(0.5 * torch.randn(1))
    return module.eval() if device is None else module.eval().to(device)


def _radial_restate(module, x, dtype, inverse=False):
    p = [t.detach().cpu().to(dtype) for t in (module.z_0, module.alpha, module.beta)]
    return (U.radial_inverse if inverse else U.radial_forward)(x.to(dtype), p[0].reshape(1, -1), p[1], p[2])


# ---- fixtures -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", U.FIXTURES)
def test_fixtures(name, device):
    t, kind, d = U.fixture(name)
    module = U.build(name).to(device)
    with torch.no_grad():
        y, lad = module(t["x"].to(device))
    assert y.shape == t["y32"].shape and lad.shape == (257,)
    for ref in (t["y32"].double(), t["y64"]):
        _within(y, ref, t["floor_fwd_y"], name + " y")
    for ref in (t["lad32"].double(), t["lad64"]):
        _within(lad, ref, t["floor_fwd_lad"], name + " lad")
    if kind == "radial":
        row = int(t["edge_row"])      # a row equal to z_0 maps to z_0
        assert torch.equal(y[row].cpu(), t["sd::z_0"][0])
        return
    with torch.no_grad():
        x, ladinv = module.inverse(t["y32"].to(device))
    for ref in (t["xinv32"].double(), t["xinv64"]):
        _within(x, ref, t["floor_inv_x"], name + " xinv")
    for ref in (t["ladinv32"].double(), t["ladinv64"]):
        _within(ladinv, ref, t["floor_inv_lad"], name + " ladinv")


# ---- fresh shapes ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [1, 3, 4, 63, 64, 65, 128, 257, 512])
def test_radial_fresh_shapes(d, device):
    """One and several registers per lane, a partial last register, both sides of the 16-byte rule, sub-wave row groups, a
    partial last block; the inverse against the closed form and as a round trip."""
    module = _radial_module(d, 100 + d)
    dev = _radial_module(d, 100 + d, device)
    for n in ROWS:
        torch.manual_seed(1000 * d + n)
        x = torch.randn(n, d) * 1.5
        y64, lad64 = _radial_restate(module, x, torch.float64)
        y32, lad32 = _radial_restate(module, x, torch.float32)
        floor_y, floor_lad = maxdiff(y32, y64), maxdiff(lad32, lad64)
        with torch.no_grad():
            y, lad = dev(x.to(device))
            x_back, lad_back = dev.inverse(y)
        tag = "radial d%d n%d" % (d, n)
        _within(y, y64, floor_y, tag + " y")
        _within(lad, lad64, floor_lad, tag + " lad")
        # round trip: the float32 restatement's own round-trip error on the same inputs is the floor
        rt32, ladrt32 = _radial_restate(module, y32, torch.float32, inverse=True)
        scale = max(float(x.abs().max()), float(y64.abs().max()))
        _within(x_back, x.double(), maxdiff(rt32, x), tag + " round trip", scale=scale)
        _within(lad + lad_back, torch.zeros(n, dtype=torch.float64), max(maxdiff(lad32 + ladrt32, torch.zeros(n)), floor_lad),
                tag + " lad sum", mult=2.0, scale=float(lad64.abs().max()))


@pytest.mark.parametrize("d", [1, 3, 4, 63, 64, 127, 128, 511])
def test_unit_vector_fresh_shapes(d, device):
    module = T.UnitVector(d).to(device)
    for n in ROWS:
        torch.manual_seed(2000 * d + n)
        x = torch.randn(n, d) * min(1.0, (10.0 / d) ** 0.5)
        y64, lad64 = U.unit_forward(x.double())
        y32, lad32 = U.unit_forward(x)
        with torch.no_grad():
            y, lad = module(x.to(device))
            x_back, lad_back = module.inverse(y)              # points produced by forward never raise
            x_comp, lad_comp = T.InverseTransform(module).forward(y)
        tag = "unit_vector d%d n%d" % (d, n)
        assert y.shape == (n, d + 1) and lad.shape == (n,) and x_back.shape == (n, d)
        floor_lad = maxdiff(lad32, lad64)
        _within(y, y64, maxdiff(y32, y64), tag + " y")
        _within(lad, lad64, floor_lad, tag + " lad")
        xi64, ladi64 = U.unit_inverse(y32.double())
        xi32, ladi32 = U.unit_inverse(y32)
        with torch.no_grad():
            xi, ladi = module.inverse(y32.to(device))
        _within(xi, xi64, maxdiff(xi32, xi64), tag + " xinv")
        _within(ladi, ladi64, maxdiff(ladi32, ladi64), tag + " ladinv")
        scale = max(1.0, float(x.abs().max()))
        _within(x_back, x.double(), maxdiff(xi32, x), tag + " round trip", scale=scale)
        _within(lad + lad_back, torch.zeros(n, dtype=torch.float64), max(maxdiff(lad32 + ladi32, torch.zeros(n)), floor_lad),
                tag + " lad sum", mult=2.0, scale=float(lad64.abs().max()))
        assert torch.equal(x_comp, x_back) and torch.equal(lad_comp, lad_back)


def test_unit_vector_flattens_leading_dimensions(device):
    torch.manual_seed(5)
    module = T.UnitVector(5).to(device)
    x = torch.randn(3, 4, 5, device=device)
    with torch.no_grad():
        y, lad = module(x)
        y_flat, lad_flat = module(x.reshape(12, 5))
        x_back, lad_back = module.inverse(y)
    assert y.shape == (3, 4, 6) and lad.shape == (12,) and x_back.shape == (3, 4, 5) and lad_back.shape == (12,)
    assert torch.equal(y.reshape(12, 6), y_flat) and torch.equal(lad, lad_flat)


@pytest.mark.parametrize("name", U.NAIVE)
def test_naive_linear_round_trip(name, device):
    t, _, d = U.fixture(name)
    module = U.build(name).to(device)
    with torch.no_grad():
        y, lad = module(t["x"].to(device))
        x_back, lad_back = module.inverse(y)
    y32, lad32 = U.restate(name, t["x"], torch.float32)
    rt32, ladrt32 = U.restate(name, y32, torch.float32, inverse=True)
    scale = max(float(t["x"].abs().max()), float(t["y64"].abs().max()))
    _within(x_back, t["x"].double(), max(maxdiff(rt32, t["x"]), float(t["floor_inv_x"])), name + " round trip", scale=scale)
    _within(lad + lad_back, torch.zeros(257, dtype=torch.float64), t["floor_fwd_lad"], name + " lad sum", mult=2.0,
            scale=float(t["lad64"].abs().max()))


# ---- radial edges ---------------------------------------------------------------------------------------------------
def test_radial_4d_z0_equals_the_flattened_layer(device):
    torch.manual_seed(11)
    z_0 = torch.randn(1, 2, 4, 4)
    image = T.RadialTransform(32, z_0=z_0.clone())
    flat = T.RadialTransform(32, z_0=z_0.reshape(1, 32).clone())
    flat.load_state_dict({k: (v.reshape(1, 32) if k == "z_0" else v) for k, v in image.state_dict().items()})
    image, flat = image.eval().to(device), flat.eval().to(device)
    x = torch.randn(9, 2, 4, 4, device=device)
    with torch.no_grad():
        y, lad = image(x)
        y_flat, lad_flat = flat(x.reshape(9, 32))
        x_back, _ = image.inverse(y)
    assert y.shape == x.shape and lad.shape == (9,) and x_back.shape == x.shape
    assert torch.equal(y.reshape(9, 32), y_flat) and torch.equal(lad, lad_flat)
    ref, lad_ref = _radial_restate(flat, x.reshape(9, 32).cpu(), torch.float64)
    assert maxdiff(y.reshape(9, 32), ref) <= 1e-5 * float(ref.abs().max()) and maxdiff(lad, lad_ref) <= 1e-4


# ---- unit-vector domain ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [7, 64, 129])          # the narrow, the 16-byte-piece and the wave-per-row kernel
def test_unit_vector_domain(d, device):
    torch.manual_seed(13)
    module = T.UnitVector(d).to(device)
    with torch.no_grad():
        with pytest.raises(T.InputOutsideDomain):
            module.inverse(torch.randn(33, d + 1, device=device) + 1)
        y, _ = module(torch.randn(33, d, device=device) * min(1.0, (10.0 / d) ** 0.5))
        module.inverse(y)                                       # points produced by forward never raise
        bad = y.clone()
        bad[17] *= 0.5                                          # one row inside the sphere: every row is tested
        with pytest.raises(T.InputOutsideDomain):
            module.inverse(bad)
        reached = False
        with pytest.raises(ops.InputOutsideDomain):
            with ops.deferred_errors():
                module.inverse(bad)
                reached = True                                  # raised at the block's end, not inside
        assert reached
        module.inverse(y)                                       # the error word was cleared


# ---- gradients ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", U.RADIAL)
def test_radial_fixture_gradients(name, device):
    t, _, d = U.fixture(name)
    module = U.build(name).to(device)
    keep = torch.ones(257, 1)
    keep[int(t["edge_row"])] = 0.0              # the row on z_0 carries no loss: the fixture's sums leave it out
    x = t["x"].to(device).requires_grad_(True)
    y, lad = module(x)
    assert type(y.grad_fn).__name__ == "_RadialFunctionBackward"
    ((y * (t["gy"] * keep).to(device)).sum() + (lad * keep.reshape(-1).to(device)).sum()).backward()
    _grad_close(x.grad, t["grad_x64"].double(), name + " x")
    for pname in ("alpha", "beta", "z_0"):
        _grad_close(getattr(module, pname).grad, t["grad64::" + pname].double(), name + " " + pname)


@pytest.mark.parametrize("name", U.UNIT)
def test_unit_vector_fixture_gradients(name, device):
    t, _, d = U.fixture(name)
    module = U.build(name).to(device)
    x = t["x"].to(device).requires_grad_(True)
    y, lad = module(x)
    assert type(y.grad_fn).__name__ == "_UnitVectorFunctionBackward"
    ((y * t["gy"].to(device)).sum() + lad.sum()).backward()
    _grad_close(x.grad, t["grad_x64"].double(), name + " x")
    yin = t["y32"].to(device).requires_grad_(True)
    x_back, ladinv = module.inverse(yin)
    assert type(x_back.grad_fn).__name__ == "_UnitVectorFunctionBackward"
    ((x_back * t["gy"][:, :d].to(device)).sum() + ladinv.sum()).backward()
    _grad_close(yin.grad, t["grad_y64"].double(), name + " y")
    assert module.dim_sphere.grad is None


@pytest.mark.parametrize("name", U.NAIVE)
def test_naive_linear_training_step(name, device):
    t, _, d = U.fixture(name)
    module = U.build(name).to(device).train()
    x = t["x"].to(device).requires_grad_(True)
    y, lad = module(x)
    assert type(y.grad_fn).__name__ == "_DenseLinearFunctionBackward"
    ((y * t["gy"].to(device)).sum() + lad.sum()).backward()
    _within(y.detach(), t["y64"], t["floor_fwd_y"], name + " y under autograd")
    _grad_close(x.grad, t["grad_x64"].double(), name + " x")
    _grad_close(module._weight.grad, t["grad64::_weight"].double(), name + " _weight")
    _grad_close(module.bias.grad, t["grad64::bias"].double(), name + " bias")
    # the inverse under autograd: the kernel with the factorised W^-1, gradients by GEMMs, against float64 autograd
    leaves = [v.double().clone().requires_grad_(True) for v in (t["y32"], t["sd::_weight"], t["sd::bias"])]
    x_ref, _ = U.naive_inverse(*leaves)
    (x_ref * t["gy"].double()).sum().backward()
    module.zero_grad()
    yin = t["y32"].to(device).requires_grad_(True)
    x_back, ladinv = module.inverse(yin)
    assert type(x_back.grad_fn).__name__ == "_DenseLinearFunctionBackward"
    (x_back * t["gy"].to(device)).sum().backward()
    _within(x_back.detach(), t["xinv64"], t["floor_inv_x"], name + " xinv under autograd")
    _within(ladinv.detach(), t["ladinv64"], t["floor_inv_lad"], name + " ladinv under autograd")
    for got, ref, what in zip((yin.grad, module._weight.grad, module.bias.grad), leaves, ("y", "_weight", "bias")):
        _grad_close(got, ref.grad, name + " inverse " + what)


@pytest.mark.parametrize("d", [3, 64, 130, 500])
def test_backward_kernels_match_float64_autograd(d, device):
    torch.manual_seed(300 + d)
    n = 515
    # radial, forward direction, with and without grad_logabsdet
    module = _radial_module(d, 400 + d)
    x = torch.randn(n, d) * 1.5
    gy, gl = torch.randn(n, d), torch.randn(n)
    leaves = [t.detach().double().clone().requires_grad_(True) for t in (x, module.z_0, module.alpha, module.beta)]
    y_ref, lad_ref = U.radial_forward(*leaves)
    ((y_ref * gy.double()).sum() + (lad_ref * gl.double()).sum()).backward()
    dev = _radial_module(d, 400 + d, device).train()
    xg = x.to(device).requires_grad_(True)
    y, lad = dev(xg)
    assert type(y.grad_fn).__name__ == "_RadialFunctionBackward"
    ((y * gy.to(device)).sum() + (lad * gl.to(device)).sum()).backward()
    for got, ref, name in zip((xg.grad, dev.z_0.grad, dev.alpha.grad, dev.beta.grad), leaves, ("x", "z_0", "alpha", "beta")):
        _grad_close(got, ref.grad, "radial d%d %s" % (d, name))
    leaves2 = [t.detach().double().clone().requires_grad_(True) for t in (x, module.z_0, module.alpha, module.beta)]
    (U.radial_forward(*leaves2)[0] * gy.double()).sum().backward()
    dev.zero_grad()
    xg2 = x.to(device).requires_grad_(True)
    (dev(xg2)[0] * gy.to(device)).sum().backward()              # grad_logabsdet absent
    for got, ref, name in zip((xg2.grad, dev.z_0.grad, dev.alpha.grad, dev.beta.grad), leaves2, ("x", "z_0", "alpha", "beta")):
        _grad_close(got, ref.grad, "radial d%d %s, outputs only" % (d, name))

    # radial, inverse direction under autograd: the implicit-function gradients
    with torch.no_grad():
        y_in = U.radial_forward(x, module.z_0, module.alpha, module.beta)[0]
    leaves3 = [t.detach().double().clone().requires_grad_(True) for t in (y_in, module.z_0, module.alpha, module.beta)]
    x_ref, ladinv_ref = U.radial_inverse(*leaves3)
    ((x_ref * gy.double()).sum() + (ladinv_ref * gl.double()).sum()).backward()
    dev.zero_grad()
    yg = y_in.to(device).requires_grad_(True)
    x_back, ladinv = dev.inverse(yg)
    ((x_back * gy.to(device)).sum() + (ladinv * gl.to(device)).sum()).backward()
    assert maxdiff(x_back.detach(), x_ref.detach()) <= 1e-5 * float(x_ref.detach().abs().max()) + 1e-5
    for got, ref, name in zip((yg.grad, dev.z_0.grad, dev.alpha.grad, dev.beta.grad), leaves3, ("y", "z_0", "alpha", "beta")):
        _grad_close(got, ref.grad, "radial inverse d%d %s" % (d, name))

    # unit vector, both directions, with and without grad_logabsdet
    unit = T.UnitVector(d).to(device)
    xu = torch.randn(n, d) * min(1.0, (10.0 / d) ** 0.5)
    gyu = torch.randn(n, d + 1)
    for with_lad in (True, False):
        x64 = xu.double().requires_grad_(True)
        y_ref, lad_ref = U.unit_forward(x64)
        ((y_ref * gyu.double()).sum() + (lad_ref * gl.double()).sum() * float(with_lad)).backward()
        xg = xu.to(device).requires_grad_(True)
        y, lad = unit(xg)
        assert type(y.grad_fn).__name__ == "_UnitVectorFunctionBackward"
        loss = (y * gyu.to(device)).sum()
        (loss + (lad * gl.to(device)).sum() if with_lad else loss).backward()
        _grad_close(xg.grad, x64.grad, "unit_vector d%d forward lad=%s" % (d, with_lad))
        y64 = y_ref.detach().float().double().requires_grad_(True)
        x_ref, ladinv_ref = U.unit_inverse(y64)
        ((x_ref * gy.double()).sum() + (ladinv_ref * gl.double()).sum() * float(with_lad)).backward()
        yg = y_ref.detach().float().to(device).requires_grad_(True)
        x_back, ladinv = unit.inverse(yg)
        assert type(x_back.grad_fn).__name__ == "_UnitVectorFunctionBackward"
        loss = (x_back * gy.to(device)).sum()
        (loss + (ladinv * gl.to(device)).sum() if with_lad else loss).backward()
        _grad_close(yg.grad, y64.grad, "unit_vector d%d inverse lad=%s" % (d, with_lad))


# ---- NaiveLinear routes ---------------------------------------------------------------------------------------------
def test_naive_linear_routes_agree_with_the_fixtures(device, monkeypatch):
    name = "naive_linear_d64"
    t, _, d = U.fixture(name)
    module = U.build(name).to(device)
    cached = U.build(name, using_cache=True).to(device)
    reps = 4
    wide_x = t["x"].repeat(reps, 1)[:1024].to(device)          # 1024 rows: the matrix-core route
    wide_y = t["y32"].repeat(reps, 1)[:1024].to(device)
    calls = []
    real_call = ops._core._call
    monkeypatch.setattr(ops.rowwave, "_call", lambda entry, *a: (calls.append(entry), real_call(entry, *a))[1])
    with torch.no_grad():
        results = {"narrow": module(t["x"].to(device)) + module.inverse(t["y32"].to(device)),
                   "wide": module(wide_x) + module.inverse(wide_y),
                   "cached": cached(t["x"].to(device)) + cached.inverse(t["y32"].to(device))}
    assert calls == ["fc_linear", "fc_linear", "fc_dense_mm", "fc_dense_mm_shifted", "fc_linear", "fc_linear"]
    assert cached.cache.weight is not None and cached.cache.inverse is not None
    for route, (y, lad, x, ladinv) in results.items():
        rows = y.shape[0]
        ref = {k: t[k].repeat(reps, 1)[:rows] if t[k].dim() == 2 else t[k].repeat(reps)[:rows]
               for k in ("y64", "lad64", "xinv64", "ladinv64")}
        _within(y, ref["y64"], t["floor_fwd_y"], "%s %s y" % (name, route))
        _within(lad, ref["lad64"], t["floor_fwd_lad"], "%s %s lad" % (name, route))
        _within(x, ref["xinv64"], t["floor_inv_x"], "%s %s xinv" % (name, route))
        _within(ladinv, ref["ladinv64"], t["floor_inv_lad"], "%s %s ladinv" % (name, route))


def test_naive_linear_factorises_once_per_parameter_version(device, monkeypatch):
    name = "naive_linear_d5"
    t, _, d = U.fixture(name)
    module = U.build(name).to(device)
    count = []
    real = torch.linalg.lu_factor
    monkeypatch.setattr(torch.linalg, "lu_factor", lambda *a, **k: (count.append(1), real(*a, **k))[1])
    y = t["y32"].to(device)
    with torch.no_grad():
        first, _ = module.inverse(y)
        second, _ = module.inverse(y)
        module(t["x"].to(device))
        assert len(count) == 1 and torch.equal(first, second)           # a sampling loop factorises once
        module._weight.mul_(2.0)                                        # an in-place update invalidates the memo
        third, lad = module.inverse(y)
        assert len(count) == 2
    assert maxdiff(third * 2, first) <= 1e-5 * float(first.abs().max())
    assert maxdiff(lad, t["ladinv64"] - d * torch.log(torch.tensor(2.0, dtype=torch.float64))) <= 1e-5


# ---- composite ------------------------------------------------------------------------------------------------------
def test_flow_of_naive_linear_and_radial_layers(device):
    torch.manual_seed(21)
    layers = [T.NaiveLinear(6), _radial_module(6, 31), _radial_module(6, 32)]
    with torch.no_grad():
        layers[0]._weight.add_(0.3 * torch.randn(6, 6) / 6 ** 0.5)
        layers[0].bias.copy_(torch.randn(6))
    flow = flows.Flow(T.CompositeTransform(layers), distributions.StandardNormal([6])).eval()

    def log_prob(x, dtype):
        z = x.to(dtype)
        z, total = U.naive_forward(z, layers[0]._weight.detach().cpu().to(dtype), layers[0].bias.detach().cpu().to(dtype))
        for layer in layers[1:]:
            z, lad = _radial_restate(layer, z, dtype)
            total = total + lad
        return total - 0.5 * (z ** 2).sum(1) - 3.0 * torch.log(torch.tensor(2 * torch.pi, dtype=dtype))

    x = torch.randn(257, 6) * 1.5
    ref64, ref32 = log_prob(x, torch.float64), log_prob(x, torch.float32)
    flow = flow.to(device)
    with torch.no_grad():
        got = flow.log_prob(x.to(device))
        samples, lp_samples = flow.sample_and_log_prob(64)
        lp_again = flow.log_prob(samples)
    _within(got, ref64, maxdiff(ref32, ref64), "flow log_prob")
    assert samples.shape == (64, 6) and torch.isfinite(samples).all()
    s64, s32 = log_prob(samples.cpu(), torch.float64), log_prob(samples.cpu(), torch.float32)
    _within(lp_samples, lp_again.double().cpu(), maxdiff(s32, s64), "sample_and_log_prob vs log_prob(samples)", mult=2.0,
            scale=float(s64.abs().max()))
