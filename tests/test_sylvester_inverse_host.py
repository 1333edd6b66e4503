"""SylvesterTransform.inverse off the GPU: the torch composition of the back substitution (CPU tensors, float32 and float64)
against float64 truth.  The criterion is in y-space -- the map is injective, so pushing the returned z through the float64
forward must land on y; x-space errors are that residual amplified by the inverse Jacobian.

Bounds follow tests/test_gpu_golden.py: 1e-5 * max(1, max|expected|) + 4 * floor, the floor being the reference's own
float32-vs-float64 difference stored with the fixture (never anything the code under test produced)."""
import copy

import numpy as np
import pytest
import torch

from flowconductor_amd import transforms as T

import _sylvester_inverse_util as U
from _util import SIZES, build_case, copies, golden, maxdiff

FIXTURES = ("sylvester_d12_m5", "sylvester_d128_m32")
STATE_KEYS = {"upper_entries1", "log_upper_diag1", "upper_entries2", "log_upper_diag2", "Q_orth.q_vectors", "bias"}


def _fixture_floor(g, key, n):
    return float(np.max(np.abs(g["%s_%d" % (key, n)].astype(np.float64) - g["%s64_%d" % (key, n)])))


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_inverse_float32(name, n):
    g = golden(name)
    t, _ = build_case(name, g)
    p = U.params64(t)
    y = torch.from_numpy(g["y_%d" % n])
    x = torch.from_numpy(g["x_%d" % n])
    with torch.no_grad():
        z, lad = t.inverse(y)
    assert z.shape == y.shape and z.dtype == torch.float32 and lad.shape == (n,)
    y_back, lad64 = U.forward64(p, z)
    bound_y = U.bound(y, _fixture_floor(g, "y", n))
    res_y = maxdiff(y_back, y)
    print(name, n, "y-space residual %.3g bound %.3g" % (res_y, bound_y))
    assert res_y <= bound_y
    bound_lad = U.bound(lad64, _fixture_floor(g, "lad", n))
    err_lad = maxdiff(lad, -lad64)
    print(name, n, "logabsdet error %.3g bound %.3g" % (err_lad, bound_lad))
    assert err_lad <= bound_lad
    # x-space: the y-space bound through the inverse Jacobian (2-norm of a D-vector of entries <= bound_y, over sigma_min)
    bound_x = np.sqrt(y.shape[1]) * bound_y / U.sigma_min(p, z)
    err_x = maxdiff(z, x)
    print(name, n, "x error %.3g bound %.3g" % (err_x, bound_x))
    assert err_x <= bound_x


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_inverse_float64(name, n):
    g = golden(name)
    t, _ = build_case(name, g)
    p = U.params64(t)
    t64 = copy.deepcopy(t).double()
    y = torch.from_numpy(g["y_%d" % n]).double()
    with torch.no_grad():
        z, lad = t64.inverse(y)
    assert z.dtype == torch.float64 and lad.dtype == torch.float64
    y_back, lad64 = U.forward64(p, z)
    assert maxdiff(y_back, y) <= 1e-12
    assert maxdiff(lad, -lad64) <= 1e-12
    # a float64 input to the float32 module is solved in float64 as well
    with torch.no_grad():
        z_mixed, _ = t.inverse(y)
    assert z_mixed.dtype == torch.float64 and maxdiff(U.forward64(p, z_mixed)[0], y) <= 1e-12


def _random_transform(d, m, sigma=0.4, seed=5):
    return U.randomize(T.SylvesterTransform(d, num_householder=m, device="cpu"), sigma, seed).eval()


def _residual(t, y):
    with torch.no_grad():
        z, lad = t.inverse(y)
    p = U.params64(t)
    y_back, lad64 = U.forward64(p, z)
    return z, lad, maxdiff(y_back, y), maxdiff(lad, -lad64)


def test_zero_diagonal_returns_finite_values():
    """log_upper_diag1 = 0 makes every r1 = 0: the scalar equation is v = t - r2 tanh(s), slope exactly 1."""
    t = _random_transform(8, 4)
    with torch.no_grad():
        t.log_upper_diag1.zero_()
    y = 2 * torch.randn(65, 8, generator=torch.Generator().manual_seed(1))
    z, lad, res_y, err_lad = _residual(t, y)
    assert torch.isfinite(z).all() and torch.isfinite(lad).all()
    assert res_y <= 1e-5 * U.scale_of(y)          # no floor: rounding level only
    assert float(lad.abs().max()) == 0.0 and err_lad == 0.0
    with torch.no_grad():
        t.log_upper_diag2.zero_()                    # r2 = 0 as well: the bracket is the single point t
    z, lad, res_y, _ = _residual(t, y)
    assert torch.isfinite(z).all() and res_y <= 1e-5 * U.scale_of(y)


def test_one_feature():
    t = _random_transform(1, 1)
    y = 2 * torch.randn(33, 1, generator=torch.Generator().manual_seed(2))
    z, lad, res_y, err_lad = _residual(t, y)
    assert z.shape == (33, 1) and lad.shape == (33,)
    assert res_y <= 1e-5 * U.scale_of(y) and err_lad <= 1e-5


def test_empty_batch():
    t = _random_transform(6, 3)
    with torch.no_grad():
        z, lad = t.inverse(torch.zeros(0, 6))
    assert z.shape == (0, 6) and lad.shape == (0,)


def test_a_call_that_needs_a_gradient_raises():
    t = _random_transform(6, 3)
    y = torch.randn(5, 6)
    with pytest.raises(RuntimeError, match="no_grad"):
        t.inverse(y)                                 # parameters require grad and grad is enabled
    for prm in t.parameters():
        prm.requires_grad_(False)
    with pytest.raises(RuntimeError, match="no_grad"):
        t.inverse(y.clone().requires_grad_(True))
    z, _ = t.inverse(y)                              # nothing requires a gradient: no no_grad() block needed
    assert not z.requires_grad


def test_wrappers_and_copies():
    t = _random_transform(6, 3)
    y = 2 * torch.randn(9, 6, generator=torch.Generator().manual_seed(3))
    with torch.no_grad():
        z, lad = t.inverse(y)
        zi, ladi = T.InverseTransform(t)(y)
    assert torch.equal(z, zi) and torch.equal(lad, ladi)
    assert set(t.state_dict().keys()) == STATE_KEYS
    for c in copies(t):
        assert set(c.state_dict().keys()) == STATE_KEYS
        with torch.no_grad():
            zc, ladc = c.inverse(y)
        assert torch.equal(z, zc) and torch.equal(lad, ladc)


def test_planar_still_has_no_inverse():
    with pytest.raises(T.InverseNotAvailable):
        T.PlanarTransform(features=4).inverse(torch.zeros(3, 4))
