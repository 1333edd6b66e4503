"""The per-row ``dopri5`` route without a GPU: the float64 reference ``dopri5_rows`` of tests/_cnf_dopri5_util.py is pinned
before anything is compared with it, then the option, the routing predicates and the CPU route.

Bounds:

* ``row_field`` against the package's float64 composition: 1e-12 (two float64 evaluations of the same expressions);
* the affine ODE at tolerance 1e-9 against ``scipy.linalg.expm``: 1e-7, the rule tests/test_cnf_host.py applies to the
  package's own ``dopri5`` (the global error of a tolerance-controlled solve over T = 1 is a moderate multiple of the
  tolerance); ``delta logp = -T tr(W)`` has a constant slope, which every Runge-Kutta step integrates exactly: 1e-12;
* a D 2 net at tolerance 1e-8 against 256 ``rk4`` steps (truncation of the order of 256^-4 = 2e-10): 1e-6, the same
  hundredfold margin over the tolerance.
"""
import numpy as np
import pytest
import scipy.linalg
import torch

from flowconductor_amd import ops, options
from flowconductor_amd.CNF.neural_odes import ODEfunc, ODEnet

from _cnf_util import field64
from _cnf_dopri5_util import (ATTEMPT_GAP, ATTEMPT_ROWS, CAP, CAP_CASES, TOL, cap_case, dopri5_rows, make_cnf, make_func,
                              mixed_rows, rk_solve, row_field, scale_of, step_control_case, worst)


# ---- the reference against the truth ---------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["ignore", "concat", "concat_v2", "squash", "concatsquash"])
@pytest.mark.parametrize("act", ["tanh", "softplus", "relu"])
def test_row_field_is_the_float64_composition(kind, act):
    func = make_func(3, (17, 33), layer_type=kind, nonlinearity=act, seed=3, gain=1.5, residual=kind == "concat",
                     scale_output=0.75)
    y = torch.randn(9, 3, dtype=torch.float64, generator=torch.Generator().manual_seed(30))
    dy, negdiv = field64(func, 0.3, y)
    got_dy, got_negdiv = row_field(func)(torch.full((9,), 0.3, dtype=torch.float64), y)
    assert worst(got_dy, dy) <= 1e-12 * scale_of(dy) and worst(got_negdiv, negdiv) <= 1e-12 * scale_of(negdiv)
    times = torch.linspace(0.0, 1.0, 9, dtype=torch.float64)         # one time per row
    got_dy, got_negdiv = row_field(func)(times, y)
    for row in range(9):
        dy, negdiv = field64(func, float(times[row]), y[row:row + 1])
        assert worst(got_dy[row], dy[0]) <= 1e-12 * scale_of(dy) and worst(got_negdiv[row], negdiv[0]) <= 1e-12


@pytest.mark.parametrize("t0,t1", [(0.0, 1.0), (1.0, 0.0)])
def test_reference_on_the_affine_ode(t0, t1):
    func = make_func(3, (), layer_type="ignore", seed=5)
    layer = func.diffeq.layers[0]._layer
    w, b = layer.weight.detach().double().numpy(), layer.bias.detach().double().numpy()
    m = np.zeros((4, 4))
    m[:3, :3], m[:3, 3] = w, b
    e = scipy.linalg.expm(m * (t1 - t0))
    z = 1.5 * torch.randn(33, 3, generator=torch.Generator().manual_seed(50))
    z_t, logp_t, attempts = dopri5_rows(func, z, t0, t1, 1e-9, 1e-9)
    expected = z.double().numpy() @ e[:3, :3].T + e[:3, 3]
    assert float(np.abs(z_t.numpy() - expected).max()) <= 1e-7 * max(1.0, float(np.abs(expected).max()))
    assert float((logp_t + (t1 - t0) * np.trace(w)).abs().max()) <= 1e-12
    assert int(attempts.min()) >= 3


@pytest.mark.parametrize("t0,t1", [(0.0, 1.0), (1.0, 0.0)])
def test_reference_on_a_net(t0, t1):
    func = make_func(2, (64, 64, 64), seed=13, gain=1.5)
    z = 1.5 * torch.randn(33, 2, generator=torch.Generator().manual_seed(130))
    z_true, logp_true = rk_solve(func, z, t0, t1, 256, "rk4")
    for rounded in (False, True):       # at 1e-8 the rounding of the stage states, 6e-8 relative, still passes 1e-6
        z_t, logp_t, _ = dopri5_rows(func, z, t0, t1, 1e-8, 1e-8, round_stage_input=rounded)
        assert worst(z_t, z_true) <= 1e-6 * scale_of(z_true), worst(z_t, z_true)
        assert worst(logp_t, logp_true) <= 1e-6 * scale_of(logp_true), worst(logp_t, logp_true)
    assert float(logp_true.abs().max()) > 1e-3


# ---- identities --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("first_step", [None, 0.05])
def test_evaluations_are_two_plus_six_per_attempt(first_step):
    func, z = step_control_case()
    _, _, attempts = dopri5_rows(func, z, 0.0, 1.0, TOL, TOL, first_step=first_step)
    assert torch.equal(dopri5_rows.last_evals, (2 if first_step is None else 1) + 6 * attempts)
    assert int(attempts.min()) >= 1


def test_a_row_alone_is_the_row_in_the_batch():
    func, _ = step_control_case()
    z = mixed_rows(65, 150)
    z_t, logp_t, attempts = dopri5_rows(func, z, 0.0, 1.0, TOL, TOL, round_stage_input=True)
    for row in (0, 31, 64):
        alone = dopri5_rows(func, z[row:row + 1], 0.0, 1.0, TOL, TOL, round_stage_input=True)
        assert torch.equal(alone[0][0], z_t[row]) and torch.equal(alone[1][0], logp_t[row])
        assert int(alone[2][0]) == int(attempts[row])
    order = torch.randperm(65, generator=torch.Generator().manual_seed(151))
    shuffled = dopri5_rows(func, z[order], 0.0, 1.0, TOL, TOL, round_stage_input=True)
    assert torch.equal(shuffled[0], z_t[order]) and torch.equal(shuffled[2], attempts[order])


def test_a_poisoned_row_ends_nan_and_alone():
    func, z = step_control_case()
    clean = dopri5_rows(func, z, 0.0, 1.0, TOL, TOL)
    poisoned = z.clone()
    poisoned[3] = float("nan")
    z_t, logp_t, attempts = dopri5_rows(func, poisoned, 0.0, 1.0, TOL, TOL)
    keep = torch.arange(64) != 3
    assert torch.isnan(z_t[3]).all() and torch.isnan(logp_t[3]) and int(attempts[3]) == 1
    assert torch.equal(z_t[keep], clean[0][keep]) and torch.equal(attempts[keep], clean[2][keep])


def test_step_control_case_separates_the_halves_and_survives_the_rounding():
    """What tests/test_gpu_cnf_dopri5.py relies on: the two halves of the batch take different attempt counts, and the
    float32 rounding of the stage states moves the counts within the cap the kernel is held to."""
    func, z = step_control_case()
    rounded = dopri5_rows(func, z, 0.0, 1.0, TOL, TOL, round_stage_input=True)[2]
    exact = dopri5_rows(func, z, 0.0, 1.0, TOL, TOL, round_stage_input=False)[2]
    assert int(rounded[:32].min()) == int(rounded[:32].max()) == 4          # the easy rows start from a smaller step
    assert int((rounded[32:] == 3).sum()) >= 24
    gap = (rounded - exact).abs()
    assert int((gap > 0).sum()) <= ATTEMPT_ROWS and int(gap.max()) <= ATTEMPT_GAP


@pytest.mark.parametrize("name,seed,gain,first_step", CAP_CASES)
def test_cap_cases_have_rows_on_both_sides(name, seed, gain, first_step):
    func, z = cap_case(seed, gain)
    free = dopri5_rows(func, z, 0.0, 1.0, TOL, TOL, first_step=first_step, round_stage_input=True)
    assert int((free[2] > CAP).sum()) > 0 and int((free[2] <= CAP).sum()) > 0
    assert int((free[2] >= CAP + 2).sum()) > 0                       # rows that must come back NaN
    if first_step is not None:
        assert int((free[2] <= CAP - 2).sum()) > 0                   # rows that must come back finished
    capped = dopri5_rows(func, z, 0.0, 1.0, TOL, TOL, first_step=first_step, max_attempts=CAP, round_stage_input=True)
    over = free[2] > CAP
    assert torch.isnan(capped[0][over]).all() and torch.isnan(capped[1][over]).all()
    assert torch.equal(capped[2][over], torch.full_like(capped[2][over], CAP))
    assert torch.equal(capped[0][~over], free[0][~over]) and torch.equal(capped[2][~over], free[2][~over])


# ---- the option and the predicates -----------------------------------------------------------------------------------

def test_option_is_validated_and_off_by_default():
    assert options.get("cnf_dopri5_kernel") is False
    for value in (False, True, "force"):
        with options.override(cnf_dopri5_kernel=value):
            assert options.get("cnf_dopri5_kernel") == value
    for value in ("on", "Force", 1, None):
        with pytest.raises(ValueError):
            with options.override(cnf_dopri5_kernel=value):
                pass
    assert options.get("cnf_dopri5_kernel") is False


def test_routing_predicates_at_their_edges():
    assert ops.cnf_dopri5_fits(16, (64,) * 4, 1e-5, 1e-5) and ops.cnf_dopri5_fits(1, (), 1e-6, 1e-6)
    assert not ops.cnf_dopri5_fits(17, (8,), 1e-5, 1e-5)
    assert not ops.cnf_dopri5_fits(3, (65,), 1e-5, 1e-5)
    assert not ops.cnf_dopri5_fits(3, (8,) * 5, 1e-5, 1e-5)
    assert not ops.cnf_dopri5_fits(3, (8,), 9.9e-7, 1e-5) and not ops.cnf_dopri5_fits(3, (8,), 1e-5, 1e-7)
    assert not ops.cnf_dopri5_fits(3, (8,), 0.0, 1e-5)
    assert ops.CNF_DOPRI5_MAX_ATTEMPTS == 4096
    assert ops.cnf_dopri5_attempts(None) == 4096 and ops.cnf_dopri5_attempts(2 ** 31 - 1) == 4096
    assert ops.cnf_dopri5_attempts(4097) == 4096 and ops.cnf_dopri5_attempts(4096) == 4096
    assert ops.cnf_dopri5_attempts(3) == 3 and ops.cnf_dopri5_attempts(1) == 1
    assert ops.cnf_dopri5_attempts(0) is None       # the host loop raises on its first attempt: no kernel for that
    lanes = ops.CNF_DOPRI5_MAX_LANES
    assert lanes == 0 or lanes & (lanes - 1) == 0
    for d in (1, 2, 16):
        rows = lanes // ops.cnf_group_lanes(d)
        assert ops.cnf_dopri5_rows_pay(rows, d) and not ops.cnf_dopri5_rows_pay(rows + 1, d)


@pytest.mark.parametrize("value", [True, "force"])
def test_a_cpu_tensor_takes_the_composition(value):
    func = make_func(2, (16, 16), seed=19, gain=1.5)
    flow = make_cnf(func, solver="dopri5", tol=TOL)
    z = torch.randn(5, 2, generator=torch.Generator().manual_seed(190))
    with torch.no_grad():
        expected = flow(z, torch.zeros(5, 1))
        evals = flow.num_evals()
        with options.override(cnf_dopri5_kernel=value):
            got = flow(z, torch.zeros(5, 1))
    assert torch.equal(got[0], expected[0]) and torch.equal(got[1], expected[1]) and flow.num_evals() == evals
    assert isinstance(func, ODEfunc) and isinstance(func.diffeq, ODEnet)
