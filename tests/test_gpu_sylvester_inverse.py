"""SylvesterTransform.inverse on the GPU: the ``fc_sylvester_inverse`` route (one lane per row between the two applications
of Q) against float64 truth.  The criterion is in y-space -- pushing the kernel's z through the float64 forward must land
on y -- and logabsdet must be minus the float64 forward's at the returned point.

Bounds follow tests/test_gpu_golden.py: 1e-5 * max(1, max|expected|) + 4 * floor.  The floor never comes from the code
under test: for the fixtures it is the reference's float32-vs-float64 difference stored in the .npz; elsewhere it is the
error of the existing FORWARD kernel against float64 at the same points."""
import copy

import numpy as np
import pytest
import torch

from flowconductor_amd import distributions, flows, ops, options, transforms as T

import _sylvester_inverse_util as U
from _util import SIZES, build_case, golden, maxdiff
from oracle import torch_oracle as O

pytestmark = pytest.mark.gpu

FIXTURES = ("sylvester_d12_m5", "sylvester_d128_m32")


def _inverse(t, y):
    """(z, logabsdet, launches of fc_sylvester_inverse) of one ``inverse`` call."""
    with torch.no_grad(), ops.KernelTimer("fc_sylvester_inverse") as timer:
        z, lad = t.inverse(y)
    return z, lad, len(timer.pairs)


# ---- fixtures ------------------------------------------------------------------------------------------------------------

def _fixture_floor(g, key, n):
    return float(np.max(np.abs(g["%s_%d" % (key, n)].astype(np.float64) - g["%s64_%d" % (key, n)])))


def _check_fixture(name, n, t, device, g):
    p = U.params64(t)
    y = torch.from_numpy(g["y_%d" % n])
    x = torch.from_numpy(g["x_%d" % n])
    z, lad, launches = _inverse(t, y.to(device))
    assert launches == 1
    assert z.shape == y.shape and lad.shape == (n,) and z.dtype == torch.float32
    y_back, lad64 = U.forward64(p, z)
    bound_y = U.bound(y, _fixture_floor(g, "y", n))
    res_y = maxdiff(y_back, y)
    print(name, n, "y-space residual %.3g bound %.3g" % (res_y, bound_y))
    assert res_y <= bound_y
    bound_lad = U.bound(lad64, _fixture_floor(g, "lad", n))
    err_lad = maxdiff(lad, -lad64)
    print(name, n, "logabsdet error %.3g bound %.3g" % (err_lad, bound_lad))
    assert err_lad <= bound_lad
    bound_x = np.sqrt(y.shape[1]) * bound_y / U.sigma_min(p, z)
    err_x = maxdiff(z, x)
    print(name, n, "x error %.3g bound %.3g" % (err_x, bound_x))
    assert err_x <= bound_x
    return z


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_inverse_on_the_kernel(name, n, device):
    g = golden(name)
    t, _ = build_case(name, g)
    _check_fixture(name, n, t.to(device), device, g)


# ---- random parameters: floors from the forward kernel --------------------------------------------------------------------

def _transform(d, seed=11, m=None):
    sigma = 0.4 if d <= 16 else 0.15
    m = max(1, d // 4) if m is None else m
    return U.randomize(T.SylvesterTransform(d, num_householder=m, device="cpu"), sigma, seed).eval()


def _check_against_forward_floor(t, y, device, expect_launches=1):
    """y-space and logabsdet checks of ``t.inverse(y)`` with the floors of the forward kernel; returns (z, lad)."""
    p = U.params64(t)
    td = t.to(device)
    z, lad, launches = _inverse(td, y.to(device))
    assert launches == expect_launches
    assert z.shape == y.shape and lad.shape == (y.shape[0],)
    assert torch.isfinite(z).all() and torch.isfinite(lad).all()
    z64 = U.inverse64(p, y)
    with torch.no_grad():
        y_hip, _ = td(z64.float().to(device))                  # forward kernel at the float64 solution
        _, lad_hip = td(z)                                     # and its logabsdet at the kernel's own output
    y_back, lad64 = U.forward64(p, z)
    floor_y = maxdiff(y_hip, y)
    floor_lad = maxdiff(lad_hip, lad64)
    res_y, bound_y = maxdiff(y_back, y), U.bound(y, floor_y)
    err_lad, bound_lad = maxdiff(lad, -lad64), U.bound(lad64, floor_lad)
    print("d %d n %d: y-space residual %.3g bound %.3g (floor %.3g); logabsdet error %.3g bound %.3g (floor %.3g)"
          % (y.shape[1], y.shape[0], res_y, bound_y, floor_y, err_lad, bound_lad, floor_lad))
    assert res_y <= bound_y
    assert err_lad <= bound_lad
    return z, lad


@pytest.mark.parametrize("d", [1, 2, 3, 17, 63, 64, 65, 128])
def test_shapes(d, device):
    """Partial tile, exactly one tile, one row into the next, several tiles; one partial block of columns, whole blocks
    only, whole blocks plus a partial one."""
    t = _transform(d)
    for n in (1, 63, 64, 65, 257):
        y = 2 * torch.randn(n, d, generator=torch.Generator().manual_seed(100 * d + n))
        _check_against_forward_floor(t, y, device)


REGIMES = ("zero_diagonals", "near_singular", "saturated", "large_inputs")


@pytest.mark.parametrize("regime", REGIMES)
def test_regimes(regime, device):
    d, n = 8, 65
    t = _transform(d, seed=23)
    y = 2 * torch.randn(n, d, generator=torch.Generator().manual_seed(7))
    with torch.no_grad():
        if regime == "zero_diagonals":
            t.log_upper_diag1.zero_()
        elif regime == "near_singular":         # r1 r2 = -tanh(4)^2: the slope goes down to 1.3e-3
            t.log_upper_diag1.fill_(4.0)
            t.log_upper_diag2.fill_(-4.0)
        elif regime == "saturated":
            t.bias.copy_(30.0 * (1 - 2 * (torch.arange(d) % 2)).float())
        else:
            y = 1e3 * torch.randn(n, d, generator=torch.Generator().manual_seed(8))
    _check_against_forward_floor(t, y, device)


# ---- rows are independent -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("d", [8, 65])
def test_rows_are_independent(d, device):
    t = _transform(d, seed=31).to(device)
    y = (2 * torch.randn(65, d, generator=torch.Generator().manual_seed(9))).to(device)
    z, lad, _ = _inverse(t, y)
    z2, lad2, _ = _inverse(t, y)
    assert torch.equal(z, z2) and torch.equal(lad, lad2)
    z1, lad1, _ = _inverse(t, y[64:65])
    assert torch.equal(z[64], z1[0]) and torch.equal(lad[64], lad1[0])
    bad = y.clone()
    bad[17] = float("nan")
    zb, ladb, _ = _inverse(t, bad)              # returns: the scalar solves have a fixed cap of evaluations
    keep = torch.arange(65, device=device) != 17
    assert torch.isnan(zb[17]).all() and torch.isnan(ladb[17])
    assert torch.equal(zb[keep], z[keep]) and torch.equal(ladb[keep], lad[keep])


# ---- routes ---------------------------------------------------------------------------------------------------------------

def test_wide_layer_takes_the_composition(device):
    t = _transform(130, m=8)
    y = 2 * torch.randn(7, 130, generator=torch.Generator().manual_seed(12))
    _check_against_forward_floor(t, y, device, expect_launches=0)


def test_non_contiguous_input(device):
    t = _transform(17, seed=41).to(device)
    buf = (2 * torch.randn(17, 65, generator=torch.Generator().manual_seed(13))).to(device)
    y = buf.t()[:, ::1]
    assert not y.is_contiguous()
    z, lad, launches = _inverse(t, y)
    zc, ladc, _ = _inverse(t, y.contiguous())
    assert launches == 1 and torch.equal(z, zc) and torch.equal(lad, ladc)


def test_without_the_matrix_core_rotations(device):
    """Q as folded dense matrices (``fc_dense_mm``) or as reflections (``fc_householder``): both within the bounds."""
    name, n = "sylvester_d128_m32", 257
    g = golden(name)
    t, _ = build_case(name, g)
    t = t.to(device)
    y = torch.from_numpy(g["y_%d" % n]).to(device)
    with torch.no_grad(), ops.KernelTimer("fc_dense_mm") as mm:
        t.inverse(y)
    assert len(mm.pairs) == 2
    z_on = _check_fixture(name, n, t, device, g)
    with options.override(sylvester_mm=False):
        with torch.no_grad(), ops.KernelTimer("fc_dense_mm") as mm:
            t.inverse(y)
        assert len(mm.pairs) == 0
        z_off = _check_fixture(name, n, t, device, g)
    p = U.params64(t)
    bound_y = U.bound(y, _fixture_floor(g, "y", n))
    assert maxdiff(z_on, z_off) <= 2 * np.sqrt(128) * bound_y / U.sigma_min(p, z_on)


# ---- a flow that samples --------------------------------------------------------------------------------------------------

def test_flow_samples(device):
    torch.manual_seed(3)
    layers = []
    for i in range(3):
        layers += [U.randomize(T.SylvesterTransform(8, num_householder=4, device="cpu"), 0.4, 50 + i),
                   T.ReversePermutation(8)]
    flow = flows.Flow(T.CompositeTransform(layers), distributions.StandardNormal([8])).eval()
    flow64 = copy.deepcopy(flow).double()
    flow = flow.to(device)
    with torch.no_grad():
        draws = flow.sample(257)
        assert draws.shape == (257, 8) and torch.isfinite(draws).all()
        s, lp = flow.sample_and_log_prob(257)
        assert s.shape == (257, 8) and lp.shape == (257,)
        oracle64 = O.flow_log_prob(flow64, s.double().cpu())
        floor = maxdiff(flow.log_prob(s), oracle64)            # the existing forward kernels at the same points
    err, bound = maxdiff(lp, oracle64), U.bound(oracle64, floor)
    print("flow: log-density error %.3g bound %.3g (floor %.3g)" % (err, bound, floor))
    assert err <= bound
