"""``LULinear`` and the cached ``Linear`` on every dispatch route against float64: the row kernel (``fc_linear``) at every
register width and across its grid-stride sweep, the wide matrix-core route (``fc_dense_mm`` forward,
``fc_dense_mm_shifted`` inverse) and its boundary, a bias that dominates the result, ill-conditioned weights, inputs
that strain the split-f16 operands, autograd, ``OneByOneConvolution`` above the fused kernel's channel limit, and widths
above the row kernels' 512 features.

Every check uses the bound of tests/test_gpu_golden.py:  err <= 1e-5 max(1, max|ref64|) + 4 floor,  where floor is the
reference's own float32 algorithm against float64 on the same inputs (lu.py:56-91, linear.py:45-76).  Parameters are
always set explicitly (random strict triangles, diagonal and a nonzero bias), never the identity initialisation."""
import contextlib
import math

import pytest
import torch
from torch.nn import functional as F

from _util import maxdiff
from flowconductor_amd import ops
from flowconductor_amd import transforms as T

pytestmark = pytest.mark.gpu

ROW, WIDE, WIDE_SHIFTED = "fc_linear", "fc_dense_mm", "fc_dense_mm_shifted"
ENTRIES = (ROW, WIDE, WIDE_SHIFTED)
F64 = torch.float64


# ---- parameters, references, bounds --------------------------------------------------------------------------------

def _make(d, seed, bias_scale=1.0, offdiag=0.5, diag_scale=1.0, using_cache=False, cls=T.LULinear, **kw):
    """A module with strict triangles ~ N(0, offdiag^2 / d), diag U ~ U[0.5, 2] diag_scale, bias ~ N(0, bias_scale^2)."""
    gen = torch.Generator().manual_seed(seed)
    strict = d * (d - 1) // 2
    t = cls(d, using_cache=using_cache, identity_init=False, **kw)
    lower = torch.randn(strict, generator=gen, dtype=F64) * (offdiag / math.sqrt(d))
    upper = torch.randn(strict, generator=gen, dtype=F64) * (offdiag / math.sqrt(d))
    diag = (0.5 + 1.5 * torch.rand(d, generator=gen, dtype=F64)) * diag_scale
    bias = torch.randn(d, generator=gen, dtype=F64) * bias_scale
    with torch.no_grad():
        t.lower_entries.copy_(lower)
        t.upper_entries.copy_(upper)
        t.unconstrained_upper_diag.copy_(torch.log(torch.expm1(diag - t.eps)))
        t.bias.copy_(bias)
    return t


def _lu(t, dtype):
    """(L, U, bias) of module ``t`` built in ``dtype`` from its float32 parameters, on the host."""
    d = t.features
    lower, upper = torch.eye(d, dtype=dtype), torch.zeros(d, d, dtype=dtype)
    il, iu = torch.tril_indices(d, d, -1), torch.triu_indices(d, d, 1)
    lower[il[0], il[1]] = t.lower_entries.detach().cpu().to(dtype)
    upper[iu[0], iu[1]] = t.upper_entries.detach().cpu().to(dtype)
    upper.diagonal().copy_(F.softplus(t.unconstrained_upper_diag.detach().cpu().to(dtype)) + t.eps)
    return lower, upper, t.bias.detach().cpu().to(dtype)


def _reference(t, x, inverse, cached=False, dtype=torch.float32):
    """The reference's algorithm in ``dtype`` on the host: two F.linear / x - b and two triangular solves, or with the
    cache F.linear with W and F.linear(x - b, W^-1)."""
    lower, upper, bias = _lu(t, dtype)
    x = x.detach().cpu().to(dtype)
    if not inverse:
        return F.linear(x, lower @ upper, bias) if cached else F.linear(F.linear(x, upper), lower, bias)
    if cached:
        eye = torch.eye(t.features, dtype=dtype)
        l_inv = torch.linalg.solve_triangular(lower, eye, upper=False, unitriangular=True)
        return F.linear(x - bias, torch.linalg.solve_triangular(upper, l_inv, upper=True))
    out = torch.linalg.solve_triangular(lower, (x - bias).t(), upper=False, unitriangular=True)
    return torch.linalg.solve_triangular(upper, out, upper=True).t()


def _bound(ref32, ref64):
    return 1e-5 * max(1.0, float(ref64.abs().max())) + 4.0 * maxdiff(ref32, ref64)


def _check(t, x, got, inverse, cached, what):
    """``got`` against float64 truth; returns err / bound."""
    ref64 = _reference(t, x, inverse, dtype=F64)
    bound = _bound(_reference(t, x, inverse, cached), ref64)
    assert bool(torch.isfinite(got).all()), (what, "non-finite outputs")
    err = maxdiff(got, ref64)
    assert err <= bound, (what, "err %.3g > bound %.3g (ratio %.2f)" % (err, bound, err / bound))
    return err / bound


def _check_lad(t, lad, lad_inv, n, what, per_row=1.0):
    """log|det| against float64 sum log diag U (times ``per_row`` pixels); forward + inverse == 0 exactly."""
    lad64 = per_row * float(_lu(t, F64)[1].diagonal().log().sum())
    lad32 = per_row * float(_lu(t, torch.float32)[1].diagonal().log().sum())
    bound = 1e-5 * max(1.0, abs(lad64)) + 4.0 * abs(lad32 - lad64)
    assert lad.shape == (n,) and lad_inv.shape == (n,), what
    assert maxdiff(lad, torch.full((n,), lad64, dtype=F64)) <= bound, (what, "logabsdet")
    assert maxdiff(lad_inv, torch.full((n,), -lad64, dtype=F64)) <= bound, (what, "inverse logabsdet")
    assert bool(((lad + lad_inv) == 0).all()), (what, "lad_fwd + lad_inv != 0")


def _run(t, x, inverse):
    """``t(x)`` / ``t.inverse(x)`` without autograd, and the launches of each C entry of ENTRIES."""
    with torch.no_grad(), contextlib.ExitStack() as stack:
        timers = {name: stack.enter_context(ops.KernelTimer(name)) for name in ENTRIES}
        out, lad = (t.inverse if inverse else t)(x)
    return out, lad, {name: len(timer.pairs) for name, timer in timers.items()}


def _assert_route(launches, route, what):
    """``route``: the one C entry that must have launched, once (None: none of them)."""
    assert launches == {name: int(name == route) for name in ENTRIES}, (what, route, launches)


def _pair(t, n, seed, scale=1.0):
    """(z, x = W z + b): z ~ N(0, scale^2) and the matching input of the inverse, formed in float64, rounded once."""
    gen = torch.Generator().manual_seed(seed)
    z = torch.randn(n, t.features, generator=gen, dtype=F64) * scale
    lower, upper, bias = _lu(t, F64)
    return z.float(), (z @ (lower @ upper).T + bias).float()


def _both(t, z, x, device, routes, cached=False, what=""):
    """Both directions through the expected routes, against float64; returns the two err / bound ratios."""
    y, lad, fwd = _run(t, z.to(device), False)
    back, lad_inv, inv = _run(t, x.to(device), True)
    ratios = (_check(t, z, y, False, cached, (what, "forward")), _check(t, x, back, True, cached, (what, "inverse")))
    _check_lad(t, lad, lad_inv, z.shape[0], what)
    _assert_route(fwd, routes[0], (what, "forward"))
    _assert_route(inv, routes[1], (what, "inverse"))
    return ratios


# ---- 1-2. the row kernel: every register width, the grid-stride sweep ----------------------------------------------

@pytest.mark.parametrize("n", (1, 3, 257))
@pytest.mark.parametrize("d", (1, 2, 3, 15, 16, 17, 31, 33, 63, 64, 65, 100, 127, 128, 129, 200, 255, 256, 257, 384,
                               511, 512))
def test_row_kernel_widths(d, n, device):
    """fc_linear modes 1 / 2 at E = 1 / 2 / 4 / 8 registers per lane and the width edges of each."""
    t = _make(d, 10 + d).to(device)
    z, x = _pair(t, n, d + n)
    _both(t, z, x, device, (ROW, ROW), what=(d, n))


@pytest.mark.parametrize("d,n", ((200, 2 * 8192 + 3), (64, 2 * 8192 + 3), (64, 8195)))
def test_row_kernel_grid_stride(d, n, device):
    """More rows than one sweep of the capped grid (2048 blocks x 4 waves = 8192 rows), with a partial last sweep;
    n % 16 != 0 keeps D = 64 on the row kernel."""
    t = _make(d, 20 + d).to(device)
    z, x = _pair(t, n, n)
    _both(t, z, x, device, (ROW, ROW), what=(d, n))


# ---- 3. the wide route and its boundary ------------------------------------------------------------------------------

@pytest.mark.parametrize("n", (1024, 1040, (1 << 17) + 16))
@pytest.mark.parametrize("d", (32, 64, 96, 128))
def test_wide_route(d, n, device):
    """fc_dense_mm (W = L U) / fc_dense_mm_shifted (W^-1 (x - b)): one and several grid sweeps (65536 rows per sweep
    at D <= 64, 32768 at D = 96 / 128), the last one partial."""
    t = _make(d, 30 + d).to(device)
    z, x = _pair(t, n, n + d)
    _both(t, z, x, device, (WIDE, WIDE_SHIFTED), what=(d, n))


@pytest.mark.parametrize("d", (32, 64, 96, 128, 160))
def test_wide_route_boundary(d, device):
    """The same data one row short of the wide route (n = 1023), at n % 16 != 0 (1030), and D = 160 at n = 1040: the
    row kernel, held to the same float64 bound."""
    t = _make(d, 30 + d).to(device)
    z, x = _pair(t, 1040, 1040 + d)
    for n in (1023, 1030) if d != 160 else (1023, 1030, 1040):
        _both(t, z[:n], x[:n], device, (ROW, ROW), what=(d, n))


# ---- 4. a bias that dominates the result -----------------------------------------------------------------------------

@pytest.mark.parametrize("scale", (10.0, 100.0, 1000.0))
@pytest.mark.parametrize("route", ("wide", "row", "cached"))
@pytest.mark.parametrize("d", (64, 128))
def test_bias_dominates(d, route, scale, device):
    """|b| >> |W z|: the inverse must subtract the bias before W^-1 (W^-1 x - W^-1 b cancels two large terms)."""
    t = _make(d, 40 + d, bias_scale=scale, using_cache=route == "cached").to(device).eval()
    n = 2048 if route != "row" else 2040
    z, x = _pair(t, n, int(scale) + d)
    routes = (WIDE, WIDE_SHIFTED) if route == "wide" else (ROW, ROW)
    _both(t, z, x, device, routes, cached=route == "cached", what=(d, route, scale))


# ---- 5. conditioning -------------------------------------------------------------------------------------------------

def _conditioned(d, seed, target):
    """LULinear with cond(W) within 3x of ``target``: the diagonal shrunk to U[0.25, 1], the off-diagonal scale set by
    bisection (cond grows monotonically with it for a fixed draw)."""
    def cond_of(off):
        lower, upper, _ = _lu(_make(d, seed, offdiag=off, diag_scale=0.5), F64)
        return float(torch.linalg.cond(lower @ upper))
    lo, hi = 0.0, 8.0
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        if cond_of(mid) < target:
            lo = mid
        else:
            hi = mid
    t = _make(d, seed, offdiag=hi, diag_scale=0.5)
    cond = cond_of(hi)
    assert target / 3 <= cond <= 3 * target, cond
    return t, cond


@pytest.mark.parametrize("target", (1e3, 1e5))
@pytest.mark.parametrize("route", ("wide", "row"))
def test_ill_conditioned(route, target, device):
    d = 64
    t, cond = _conditioned(d, 50, target)
    t = t.to(device)
    n = 2048 if route == "wide" else 2040
    z, x = _pair(t, n, 51)
    routes = (WIDE, WIDE_SHIFTED) if route == "wide" else (ROW, ROW)
    _both(t, z, x, device, routes, what=(route, "cond %.3g" % cond))


# ---- 6. inputs that strain the split-f16 operands ----------------------------------------------------------------------

def test_split_f16_route_inputs(device):
    """Rows with one entry of 1e4 / 7e4 (above the f16 maximum) beside O(1) entries, all-zero rows and rows of 1e-30 on
    the wide route: finite, and within the bound for every group of rows on its own."""
    d, n = 64, 1024
    t = _make(d, 60).to(device)
    gen = torch.Generator().manual_seed(61)
    x = torch.randn(n, d, generator=gen)
    x[0:8, 5] = 1e4
    x[8:16, 40] = 7e4
    x[16:32] = 0.0
    x[32:48] = torch.randn(16, d, generator=gen) * 1e-30
    groups = {"1e4": slice(0, 8), "7e4": slice(8, 16), "zero": slice(16, 32), "1e-30": slice(32, 48),
              "normal": slice(48, n)}
    for inverse, route in ((False, WIDE), (True, WIDE_SHIFTED)):
        got, _, launches = _run(t, x.to(device), inverse)
        for name, rows in groups.items():
            _check(t, x[rows], got[rows], inverse, False, (name, "inverse" if inverse else "forward"))
        _assert_route(launches, route, "inverse" if inverse else "forward")


# ---- 7. the cached Linear ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("scale", (1.0, 100.0))
@pytest.mark.parametrize("d", (9, 70, 200, 512))
def test_cached_linear(d, scale, device):
    """Eval mode with using_cache: fc_linear mode 0 with W (forward) and W^-1 applied to x - b (inverse)."""
    t = _make(d, 70 + d, bias_scale=scale, using_cache=True).to(device).eval()
    z, x = _pair(t, 257, d)
    _both(t, z, x, device, (ROW, ROW), cached=True, what=(d, scale))
    assert t.cache.weight is not None and t.cache.inverse is not None


def test_cached_linear_reuse_and_invalidation(device):
    d = 70
    t = _make(d, 77, using_cache=True).to(device).eval()
    z, x = _pair(t, 100, 78)
    z, x = z.to(device), x.to(device)
    with torch.no_grad():
        y1, _ = t(z)
        b1, _ = t.inverse(x)
        weight, inverse = t.cache.weight, t.cache.inverse
        y2, _ = t(z)
        b2, _ = t.inverse(x)
    assert t.cache.weight is weight and t.cache.inverse is inverse, "the cache was rebuilt between calls"
    assert torch.equal(y1, y2) and torch.equal(b1, b2)
    with torch.no_grad():
        t.lower_entries.mul_(1.5)
        t.bias.add_(0.25)
    t.train()
    t.eval()
    assert t.cache.weight is None and t.cache.inverse is None
    with torch.no_grad():
        y3, _ = t(z)
        b3, _ = t.inverse(x)
    assert not torch.equal(y1, y3) and not torch.equal(b1, b3)
    _check(t, z, y3, False, True, "forward after a parameter change")
    _check(t, x, b3, True, True, "inverse after a parameter change")


# ---- 8. autograd -----------------------------------------------------------------------------------------------------

def _reference_grads(t, x, gy, glad, inverse, dtype):
    """Gradients of sum(y gy) + sum(lad glad) wrt x and the four parameters, autograd through the reference's
    composition in ``dtype`` on the host."""
    d = t.features
    names = ("lower_entries", "upper_entries", "unconstrained_upper_diag", "bias")
    params = [getattr(t, k).detach().cpu().to(dtype).requires_grad_(True) for k in names]
    lo, up, ud, b = params
    xs = x.cpu().to(dtype).requires_grad_(True)
    il, iu = torch.tril_indices(d, d, -1), torch.triu_indices(d, d, 1)
    diag = F.softplus(ud) + t.eps
    lower = torch.eye(d, dtype=dtype).index_put((il[0], il[1]), lo)
    upper = torch.diag(diag).index_put((iu[0], iu[1]), up)
    if not inverse:
        y = F.linear(F.linear(xs, upper), lower, b)
        lad = diag.log().sum()
    else:
        y = torch.linalg.solve_triangular(lower, (xs - b).t(), upper=False, unitriangular=True)
        y = torch.linalg.solve_triangular(upper, y, upper=True).t()
        lad = -diag.log().sum()
    loss = (y * gy.to(dtype)).sum() + (lad * glad.to(dtype)).sum()
    return torch.autograd.grad(loss, [xs] + params)


@pytest.mark.parametrize("cached_eval", (False, True))
@pytest.mark.parametrize("inverse", (False, True))
@pytest.mark.parametrize("d", (17, 64, 200))
def test_autograd(d, inverse, cached_eval, device):
    """_LULinearFunction: fc_linear forward, gradients of x and every parameter against float64 autograd.  In eval
    mode with using_cache the cache steps aside (Linear._cache_active) and stays empty."""
    t = _make(d, 80 + d, using_cache=cached_eval)
    t = (t.eval() if cached_eval else t.train()).to(device)
    n = 300
    gen = torch.Generator().manual_seed(81)
    x = torch.randn(n, d, generator=gen)
    gy, glad = torch.randn(n, d, generator=gen), torch.randn(n, generator=gen)
    xd = x.to(device).requires_grad_(True)
    with ops.KernelTimer(ROW) as timer:
        y, lad = (t.inverse if inverse else t)(xd)
        loss = (y * gy.to(device)).sum() + (lad * glad.to(device)).sum()
        grads = torch.autograd.grad(loss, [xd, t.lower_entries, t.upper_entries, t.unconstrained_upper_diag, t.bias])
    assert len(timer.pairs) == 1, "the forward kernel did not run"
    assert t.cache.weight is None and t.cache.inverse is None
    _check(t, x, y.detach(), inverse, False, "outputs")
    g64 = _reference_grads(t, x, gy, glad, inverse, F64)
    g32 = _reference_grads(t, x, gy, glad, inverse, torch.float32)
    for name, g, r64, r32 in zip(("x", "lower_entries", "upper_entries", "unconstrained_upper_diag", "bias"),
                                 grads, g64, g32):
        bound = _bound(r32, r64)
        err = maxdiff(g, r64)
        assert err <= bound, (name, "err %.3g > bound %.3g" % (err, bound))


# ---- 9. OneByOneConvolution above the fused kernel's channel limit ----------------------------------------------------

def _random_conv(c, seed, device, offdiag=0.5):
    torch.manual_seed(seed)
    t = T.OneByOneConvolution(c, identity_init=False)
    with torch.no_grad():
        t.lower_entries.mul_(2.0 * offdiag)      # uniform(+-offdiag / sqrt(c)) off the diagonal
        t.upper_entries.mul_(2.0 * offdiag)
        t.bias.uniform_(-0.5, 0.5)
    return t.to(device).eval()


def _conv_reference(t, x, inverse, dtype):
    """The reference's composition on the host: permute, LULinear on rows (two F.linear / two triangular solves),
    permute back."""
    lower, upper, bias = _lu(t, dtype)
    perm = t.permutation._permutation.cpu()
    b, c, h, w = x.shape
    xs = x.detach().cpu().to(dtype)
    if not inverse:
        rows = xs[:, perm].permute(0, 2, 3, 1).reshape(-1, c)
        out = F.linear(F.linear(rows, upper), lower, bias)
        return out.reshape(b, h, w, c).permute(0, 3, 1, 2)
    rows = (xs.permute(0, 2, 3, 1).reshape(-1, c) - bias).t()
    rows = torch.linalg.solve_triangular(lower, rows, upper=False, unitriangular=True)
    out = torch.linalg.solve_triangular(upper, rows, upper=True).t().reshape(b, h, w, c).permute(0, 3, 1, 2)
    return out[:, torch.argsort(perm)]


@pytest.mark.parametrize("c", (192, 384, 520))
def test_conv_wide_channels(c, device):
    """More than 128 channels: permutation + LULinear on rows through fc_linear at E = 4 / 8 (C = 520: above the row
    kernels, the reference's composition), both directions."""
    t = _random_conv(c, 90 + c, device)
    b, h, w = 2, 8, 6
    x = torch.randn(b, c, h, w, generator=torch.Generator().manual_seed(c))
    with torch.no_grad(), ops.KernelTimer(ROW) as rows, ops.KernelTimer("fc_conv1x1") as conv:
        y, lad = t(x.to(device))
        back, lad_inv = t.inverse(x.to(device))
    assert len(rows.pairs) == (2 if c <= ops.MAX_ROW_FEATURES else 0) and len(conv.pairs) == 0
    for got, inverse in ((y, False), (back, True)):
        ref64 = _conv_reference(t, x, inverse, F64)
        bound = _bound(_conv_reference(t, x, inverse, torch.float32), ref64)
        err = maxdiff(got, ref64)
        assert err <= bound, (c, inverse, "err %.3g > bound %.3g" % (err, bound))
    _check_lad(t, lad, lad_inv, b, c, per_row=h * w)


# ---- 10. above the row kernels' 512 features ----------------------------------------------------------------------------

@pytest.mark.parametrize("cached", (False, True))
@pytest.mark.parametrize("d", (513, 784))
def test_above_512_features(d, cached, device):
    """LULinear(784) (flattened MNIST) and the first width past the row kernels: the reference's composition on the
    device, no kernel launch, both directions against float64; uncached also under autograd."""
    t = _make(d, 100 + d, using_cache=cached).to(device).eval()
    z, x = _pair(t, 64, d)
    _both(t, z, x, device, (None, None), cached=cached, what=(d, cached))
    if cached:
        return
    t.train()
    xd = x.to(device).requires_grad_(True)
    back, lad = t.inverse(xd)
    (gx,) = torch.autograd.grad(back.sum() + lad.sum(), xd)
    ones = torch.ones(x.shape[0], d)
    g64 = _reference_grads(t, x, ones, torch.ones(x.shape[0]), True, F64)[0]
    g32 = _reference_grads(t, x, ones, torch.ones(x.shape[0]), True, torch.float32)[0]
    assert maxdiff(gx, g64) <= _bound(g32, g64)
