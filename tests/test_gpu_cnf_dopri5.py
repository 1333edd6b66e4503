"""``fc_cnf_dopri5`` behind ``CNF`` (options ``cnf_dopri5_kernel``): a whole adaptive solve in one launch, every row with
its own step control.

Bounds (none of them comes from what the kernel gives):

* accuracy: ``worst(got, truth) <= 1e-5 * scale_of(truth) + 4 * e_ref`` for ``z`` and ``logp``; ``truth`` is the float64
  ``rk4`` loop of tests/_cnf_util.py with 256 steps (the affine ODE: ``scipy.linalg.expm`` and ``-tr W``), ``e_ref`` the
  error of the float64 per-row reference ``dopri5_rows`` (tests/_cnf_dopri5_util.py, pinned by
  tests/test_cnf_dopri5_host.py) at the same tolerances against that truth;
* rows: bitwise;
* attempts: the kernel's count may differ from that of the reference with the kernel's one rounding
  (``round_stage_input=True``) in at most 1/8 of the rows and nowhere by more than 2; the host test checks that the
  rounding itself stays within that;
* the cap: rows the reference puts at least 2 attempts beyond it come back NaN, rows at least 2 below it finished and
  within the accuracy bound, rows nearer the cap either.
"""
import math

import numpy as np
import pytest
import scipy.linalg
import torch

from flowconductor_amd import distributions, flows, ops, options
from flowconductor_amd.CNF import CNFTransform
from flowconductor_amd.utils.graphs import GraphedCall

from _cnf_dopri5_util import (ATTEMPT_GAP, ATTEMPT_ROWS, CAP, CAP_CASES, TOL, cap_case, dopri5_rows, make_cnf, make_func,
                              mixed_rows, rk_solve, scale_of, step_control_case, worst)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
DEEP = (64, 64, 64, 64)
# D in {1, 2, 3, 7, 8, 15, 16} (every group size at both edges) twice each, N over the tile edges, the four depths,
# the five layer kinds, three activations
GRID = [
    (1, 1, (), "ignore", "tanh"), (1, 65, (17, 33), "squash", "softplus"),
    (2, 63, (5,), "concat", "relu"), (2, 257, DEEP, "concatsquash", "tanh"),
    (3, 64, DEEP, "concat_v2", "softplus"), (3, 257, (), "concat", "tanh"),
    (7, 65, DEEP, "squash", "relu"), (7, 1, (5,), "concatsquash", "softplus"),
    (8, 63, (17, 33), "ignore", "tanh"), (8, 64, (5,), "squash", "tanh"),
    (15, 257, (5,), "concat_v2", "relu"), (15, 64, (17, 33), "concat", "softplus"),
    (16, 65, (), "concatsquash", "relu"), (16, 63, DEEP, "concatsquash", "tanh"),
]


def rows(n, d, seed, scale=1.5):
    return (scale * torch.randn(n, d, generator=torch.Generator().manual_seed(seed))).to(DEV)


def solve(flow, z, reverse=False, **kw):
    """``(z_t, delta logp [N], launches of fc_cnf_dopri5, launches of fc_cnf_field)``."""
    with torch.no_grad(), ops.KernelTimer("fc_cnf_dopri5") as whole, ops.KernelTimer("fc_cnf_field") as single:
        z_t, logp_t = flow(z, torch.zeros(z.shape[0], 1, device=z.device), reverse=reverse, **kw)
    return z_t, logp_t.reshape(-1), len(whole.pairs), len(single.pairs)


def forced(flow, z, reverse=False):
    with options.override(cnf_dopri5_kernel="force"):
        return solve(flow, z, reverse)


def direct(func, z, t0=0.0, t1=1.0, tol=TOL, **kw):
    """``(z_t, logp_t, attempts)`` of one ``ops.cnf_dopri5`` call."""
    with torch.no_grad():
        plan = func._use_kernels(z)
        assert plan is not None
        func.before_odeint()
        return ops.cnf_dopri5(z, None, t0=t0, t1=t1, atol=tol, rtol=tol, **kw, **func._kernel_args(plan))


def within(tag, got, ref, true):
    """The accuracy bound of this file; prints the figures first."""
    error, e_ref = worst(got, true), worst(ref, true)
    bound = 1e-5 * scale_of(true) + 4 * e_ref
    print("%s: error %.3g, reference error %.3g, bound %.3g" % (tag, error, e_ref, bound))
    assert error <= bound, (tag, error, bound)


# ---- 1. one launch, and accuracy -------------------------------------------------------------------------------------

@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("d,n,hidden,kind,act", GRID)
def test_one_launch_and_accuracy(d, n, hidden, kind, act, reverse):
    func = make_func(d, hidden, layer_type=kind, nonlinearity=act, seed=200 + d + n, gain=1.5,
                     residual=(d + n) % 4 == 1, scale_output=1 if n % 2 else 0.75).to(DEV)
    flow = make_cnf(func, solver="dopri5", tol=TOL).to(DEV)
    z = rows(n, d, seed=d * 1000 + n)
    z_t, logp_t, whole, single = forced(flow, z, reverse)
    assert (whole, single) == (1, 0) and z_t.shape == (n, d) and logp_t.shape == (n,)
    t0, t1 = (1.0, 0.0) if reverse else (0.0, 1.0)
    z_true, logp_true = rk_solve(func, z, t0, t1, 256, "rk4")
    z_ref, logp_ref, attempts = dopri5_rows(func, z, t0, t1, TOL, TOL)
    assert flow.num_evals() >= 2 + 6 * 2 and int(attempts.min()) >= 2
    within("z", z_t, z_ref, z_true)
    within("logp", logp_t, logp_ref, logp_true)
    assert float(logp_true.abs().max()) > 1e-3


# ---- 2. the affine known answer ---------------------------------------------------------------------------------------

def test_affine_known_answer():
    func = make_func(3, (), layer_type="ignore", seed=5)
    layer = func.diffeq.layers[0]._layer
    w, b = layer.weight.detach().double().numpy(), layer.bias.detach().double().numpy()
    m = np.zeros((4, 4))
    m[:3, :3], m[:3, 3] = w, b
    e = scipy.linalg.expm(m)
    flow = make_cnf(func, solver="dopri5", tol=1e-6).to(DEV)
    z = rows(33, 3, seed=50)
    z_t, logp_t, whole, single = forced(flow, z)
    assert (whole, single) == (1, 0)
    z_true = torch.from_numpy(z.double().cpu().numpy() @ e[:3, :3].T + e[:3, 3])
    logp_true = torch.full((33,), -float(np.trace(w)), dtype=torch.float64)
    z_ref, logp_ref, _ = dopri5_rows(func, z, 0.0, 1.0, 1e-6, 1e-6)
    within("z", z_t, z_ref, z_true)
    within("logp", logp_t, logp_ref, logp_true)


# ---- 3. rows are independent, bitwise ----------------------------------------------------------------------------------

def test_rows_are_independent_bitwise():
    func = make_func(2, (64, 64, 64), seed=15, gain=2.0).to(DEV)
    z = mixed_rows(65, 150).to(DEV)
    z_t, logp_t, attempts = direct(func, z)
    assert torch.isfinite(z_t).all() and torch.isfinite(logp_t).all()
    again = direct(func, z)
    assert all(torch.equal(a, b) for a, b in zip(again, (z_t, logp_t, attempts)))
    for row in (0, 31, 64):
        alone = direct(func, z[row:row + 1].clone())
        assert torch.equal(alone[0][0], z_t[row]) and torch.equal(alone[1][0], logp_t[row])
        assert int(alone[2][0]) == int(attempts[row])
    order = torch.randperm(65, generator=torch.Generator().manual_seed(151)).to(DEV)
    shuffled = direct(func, z[order].contiguous())
    assert torch.equal(shuffled[0], z_t[order]) and torch.equal(shuffled[1], logp_t[order])
    assert torch.equal(shuffled[2], attempts[order])
    poisoned = z.clone()
    poisoned[3] = float("nan")
    z_p, logp_p, attempts_p = direct(func, poisoned)            # the launch finishes: the row stops at once
    keep = torch.arange(65, device=DEV) != 3
    assert torch.isnan(z_p[3]).all() and torch.isnan(logp_p[3]) and int(attempts_p[3]) == 1
    assert torch.equal(z_p[keep], z_t[keep]) and torch.equal(logp_p[keep], logp_t[keep])
    assert torch.equal(attempts_p[keep], attempts[keep])


# ---- 4. per-row step control -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("first_step", [None, 0.05])
def test_every_row_controls_its_own_step(first_step):
    func, z = step_control_case()
    expected = dopri5_rows(func, z, 0.0, 1.0, TOL, TOL, first_step=first_step, round_stage_input=True)[2]
    if first_step is None:
        assert int(expected[:32].min()) == int(expected[:32].max()) == 4 and int((expected[32:] == 3).sum()) >= 24
    func, z = func.to(DEV), z.to(DEV)
    kw = {} if first_step is None else {"first_step": first_step}
    attempts = direct(func, z, **kw)[2].cpu().long()
    gap = (attempts - expected).abs()
    print("attempts: kernel %s reference %s" % (attempts.tolist(), expected.tolist()))
    assert int((gap > 0).sum()) <= ATTEMPT_ROWS and int(gap.max()) <= ATTEMPT_GAP
    flow = make_cnf(func, solver="dopri5", tol=TOL).to(DEV)
    flow.solver_options = dict(kw)
    assert forced(flow, z)[2] == 1
    assert flow.num_evals() == (2 if first_step is None else 1) + 6 * int(attempts.max())


# ---- 5. the cap ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,seed,gain,first_step", CAP_CASES)
def test_rows_beyond_the_cap_come_back_nan(name, seed, gain, first_step):
    func, z = cap_case(seed, gain)
    z_ref, logp_ref, free = dopri5_rows(func, z, 0.0, 1.0, TOL, TOL, first_step=first_step, round_stage_input=True)
    assert int((free > CAP).sum()) > 0 and int((free <= CAP).sum()) > 0
    z_true, logp_true = rk_solve(func, z, 0.0, 1.0, 256, "rk4")
    func, z = func.to(DEV), z.to(DEV)
    flow = make_cnf(func, solver="dopri5", tol=TOL).to(DEV)
    flow.solver_options = {"max_num_steps": CAP}
    kw = {}
    if first_step is not None:
        flow.solver_options["first_step"] = kw["first_step"] = first_step
    z_t, logp_t, whole, single = forced(flow, z)                # a bounded loop that returns: nothing faults or hangs
    assert (whole, single) == (1, 0)
    attempts = direct(func, z, max_attempts=CAP, **kw)[2].cpu()
    z_t, logp_t = z_t.double().cpu(), logp_t.double().cpu()
    unfinished = torch.isnan(logp_t)
    assert torch.equal(torch.isnan(z_t).all(dim=1), unfinished) and torch.equal(torch.isnan(z_t).any(dim=1), unfinished)
    assert int(attempts.max()) <= CAP and bool((attempts[unfinished] == CAP).all())
    beyond, below = free >= CAP + 2, free <= CAP - 2
    print("%s: reference attempts %s, unfinished %d" % (name, sorted(free.tolist()), int(unfinished.sum())))
    assert bool(unfinished[beyond].all()) and not bool(unfinished[below].any())
    z_bound = 1e-5 * scale_of(z_true) + 4 * worst(z_ref, z_true)
    logp_bound = 1e-5 * scale_of(logp_true) + 4 * worst(logp_ref, logp_true)
    done = ~unfinished
    assert int(done.sum()) > 0
    assert worst(z_t[done], z_true[done]) <= z_bound and worst(logp_t[done], logp_true[done]) <= logp_bound


# ---- 6. flow level and graph replay ----------------------------------------------------------------------------------

def _density(z, delta, d):
    return -0.5 * z.square().sum(dim=1) - 0.5 * d * math.log(2 * math.pi) - delta


def _density64(func, x):
    return _density(*rk_solve(func, x, 0.0, 1.0, 256, "rk4"), x.shape[1])


def _density_ref(func, x):
    z, delta, _ = dopri5_rows(func, x, 0.0, 1.0, TOL, TOL)
    return _density(z, delta, x.shape[1])


def test_flow_density_sampling_and_graph_replay():
    func = make_func(2, (64, 64, 64), seed=14, gain=1.5).to(DEV)
    flow = flows.Flow(CNFTransform(make_cnf(func, solver="dopri5", tol=TOL)), distributions.StandardNormal([2]))
    flow = flow.to(DEV).eval()
    x = rows(65, 2, seed=140, scale=1.0)
    other = rows(65, 2, seed=142, scale=1.0)
    with options.override(cnf_dopri5_kernel="force"):
        with torch.no_grad(), ops.KernelTimer("fc_cnf_dopri5") as whole, ops.KernelTimer("fc_cnf_field") as single:
            log_prob = flow.log_prob(x)
            density_launches = len(whole.pairs)
            torch.manual_seed(141)
            samples, sample_log_prob = flow.sample_and_log_prob(65)
        assert density_launches == 1 and len(whole.pairs) == 2 and len(single.pairs) == 0
        within("log_prob", log_prob, _density_ref(func, x), _density64(func, x))
        within("sample_log_prob", sample_log_prob, _density_ref(func, samples), _density64(func, samples))
        assert samples.shape == (65, 2) and torch.isfinite(samples).all()

        graphed = GraphedCall(flow.log_prob, x)
        assert torch.equal(graphed(x), log_prob)
        with torch.no_grad():
            expected = flow.log_prob(other)
        assert torch.equal(graphed(other), expected)


# ---- 7. routing ----------------------------------------------------------------------------------------------------------

def test_default_option_keeps_the_host_loop():
    func = make_func(2, (64, 64, 64), seed=13, gain=1.5).to(DEV)
    flow = make_cnf(func, solver="dopri5", tol=TOL).to(DEV)
    z = rows(65, 2, seed=130)
    assert options.get("cnf_dopri5_kernel") is False
    z_t, logp_t, whole, single = solve(flow, z)
    assert whole == 0 and single == flow.num_evals() and single >= 8
    with options.override(cnf_dopri5_kernel=False):
        z_h, logp_h, none, _ = solve(flow, z)
    assert none == 0 and torch.equal(z_t, z_h) and torch.equal(logp_t, logp_h)


def _not_for_the_kernel():
    base = dict(d=3, hidden=(8, 8))
    return {
        "d17": (dict(d=17, hidden=(8,)), None),
        "width65": (dict(d=3, hidden=(65,)), None),
        "five_hidden": (dict(d=3, hidden=(8,) * 5), None),
        "hyper": (dict(base, layer_type="hyper"), None),
        "training_mode": (base, "train"),
        "requires_grad": (base, "requires_grad"),
        "three_times": (base, "three_times"),
        "tol_1e-7": (base, "tol"),
        "rows_over_the_budget": (dict(d=2, hidden=(8,)), "rows"),
    }


@pytest.mark.parametrize("what", sorted(_not_for_the_kernel()))
def test_these_keep_the_route_they_had(what):
    kw, how = _not_for_the_kernel()[what]
    func = make_func(seed=7, gain=1.5, **kw).to(DEV)
    flow = make_cnf(func, solver="dopri5", tol=1e-7 if how == "tol" else TOL).to(DEV)
    d = kw["d"]
    count = ops.CNF_DOPRI5_MAX_LANES // ops.cnf_group_lanes(d) + 1 if how == "rows" else 9
    z = rows(count, d, seed=70)
    if how == "train":
        flow.train()

    def run():
        torch.manual_seed(71)       # training mode draws the noise of Hutchinson's estimator
        zeros = torch.zeros(count, 1, device=DEV)
        with ops.KernelTimer("fc_cnf_dopri5") as whole:
            if how == "requires_grad":
                z_t, logp_t = flow(z.clone().requires_grad_(True), zeros)
                assert z_t.requires_grad
            elif how == "train":
                z_t, logp_t = flow(z, zeros)
            else:
                with torch.no_grad():
                    times = torch.tensor([0.0, 0.5, 1.0]) if how == "three_times" else None
                    z_t, logp_t = flow(z, zeros, integration_times=times)
        return z_t.detach(), logp_t.detach(), len(whole.pairs)

    # "rows": the field kernel forced, so that the batch limit of the new route is the only thing in the way
    with options.override(cnf_kernels="force" if how == "rows" else True):
        expected = run()
        with options.override(cnf_dopri5_kernel=True if how == "rows" else "force"):
            got = run()
        assert expected[2] == 0 and got[2] == 0
        assert torch.equal(got[0], expected[0]) and torch.equal(got[1], expected[1])
        if how in ("tol", "rows"):      # within the kernel's limits otherwise: "force" at 1e-5 reaches it
            flow.test_atol = flow.test_rtol = TOL
            assert forced(flow, z)[2] == 1


@pytest.mark.parametrize("max_attempts", [0, 5000])
def test_attempt_bound_outside_the_range_raises(max_attempts):
    func = make_func(3, (8, 8), seed=7).to(DEV)
    with pytest.raises(ValueError):
        direct(func, rows(9, 3, seed=70), max_attempts=max_attempts)
