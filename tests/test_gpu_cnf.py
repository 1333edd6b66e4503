"""Continuous normalizing flows on the GPU: ``fc_cnf_field`` behind ``ODEfunc`` and ``fc_cnf_integrate`` behind ``CNF``.

Bounds (none of them comes from what the kernels give):

* fixtures (tests/golden/cnf_*.npz): field and divergence within ``1e-5 max(1, max|expected|) + 4 floor`` of the recorded
  float32 values with the recorded ``floor = max|ref32 - ref64|`` (the rule of tests/test_gpu_golden.py), in exactly
  one launch per evaluation;
* shape grid (every group size, every tile edge, empty to full-depth nets; a pairwise table over D x N x hidden):
  the same bound against the float64 composition, the floor of a case being ``max|composition32 - composition64|`` on
  the same inputs;
* beyond the limits (and beyond the batch size up to which the kernels measured faster): no kernel launch, and bitwise
  what the composition gives;
* rows: bitwise;
* fixed-step solves: against the float64 Runge-Kutta loop of tests/_cnf_util.py with the same tableau and step count
  (so only rounding is compared) within ``1e-5 max(1, max|.|) + 4 e_comp``, ``e_comp`` being the error of the float32
  torch composition solve with the same steps against that truth; the affine ODE against ``scipy.linalg.expm``
  (64 ``rk4`` steps: truncation ~1e-9, the rest is float32 rounding of the state: ``1e-5 max(1, max|.|)``);
* ``dopri5`` runs the host loop over ``fc_cnf_field``: against the float64 ``rk4`` loop with 256 steps, within
  ``4 e_comp + 1e-5 max(1, max|.|)`` with ``e_comp`` the error of the composition's ``dopri5`` at the same tolerances;
* flow level: ``log_prob`` and ``sample_and_log_prob`` against the float64 composition density under the same rule
  (64 steps, so that forward and backward solves are inverses of each other far below the bound).
"""
import copy
import math

import numpy as np
import pytest
import scipy.linalg
import torch

from flowconductor_amd import distributions, flows, ops, options
from flowconductor_amd.CNF import CNFTransform
from flowconductor_amd.utils.graphs import GraphedCall

from _cnf_util import (CASE_NAMES, KERNEL_CASES, field64, load_case, make_cnf, make_func, rk_solve, scale_of, worst)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
KINDS = ["ignore", "concat", "concat_v2", "squash", "concatsquash"]
ACTS = ["tanh", "relu", "softplus", "elu", "swish", "square", "identity"]
DIMS = [1, 2, 3, 7, 8, 15, 16]
ROWS = [1, 63, 64, 65, 257]
HIDDEN = [(), (5,), (17, 33), (64, 64, 64, 64)]
# every (D, N), (D, hidden) and (N, hidden) pair occurs: hidden walks with the sum of the two indices
GRID = [(d, n, HIDDEN[(i + j) % 4], KINDS[(i + 2 * j) % 5], ACTS[(3 * i + j) % 7])
        for i, d in enumerate(DIMS) for j, n in enumerate(ROWS)]


def rows(n, d, seed, scale=1.5):
    return (scale * torch.randn(n, d, generator=torch.Generator().manual_seed(seed))).to(DEV)


def evaluate(func, t, y):
    """``(dy, negdiv [N], launches of fc_cnf_field)`` of one call of ``func`` without gradients."""
    func.before_odeint()
    with torch.no_grad(), ops.KernelTimer("fc_cnf_field") as timer:
        dy, negdiv = func(t, (y, torch.zeros(y.shape[0], 1, device=y.device)))
    return dy, negdiv.reshape(-1), len(timer.pairs)


def composition(func, t, y):
    with options.override(cnf_kernels=False):
        return evaluate(func, t, y)


# ---- the field: fixtures ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", CASE_NAMES)
def test_fixture_on_the_kernel(name):
    func, g = load_case(name)
    func = func.to(DEV)
    t, y = torch.from_numpy(g["t"]).to(DEV), torch.from_numpy(g["y"]).to(DEV)
    dy, negdiv, launches = evaluate(func, t, y)
    assert launches == (1 if name in KERNEL_CASES else 0)       # hyper / blend: the weights depend on t
    assert func.num_evals() == 1.0
    for tag, got in (("dy", dy), ("negdiv", negdiv)):
        expected = torch.from_numpy(g[tag + "32"]).reshape(got.shape)
        bound = 1e-5 * scale_of(expected) + 4 * float(g["floor_" + tag])
        assert worst(got, expected) <= bound, (name, tag, worst(got, expected), bound)
    dy_host, negdiv_host, _ = evaluate(func, float(g["t"]), y)        # t as a number: a kernel argument
    assert torch.equal(dy_host, dy) and torch.equal(negdiv_host, negdiv)


# ---- the field: shape grid -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("d,n,hidden,kind,act", GRID)
def test_field_shape_grid(d, n, hidden, kind, act):
    func = make_func(d, hidden, layer_type=kind, nonlinearity=act, seed=100 + d + n, gain=1.5,
                     residual=(d + n) % 2 == 1, scale_output=1 if n % 2 else 0.75).to(DEV)
    y = rows(n, d, seed=d * 1000 + n)
    t = 0.3
    dy, negdiv, launches = evaluate(func, t, y)
    assert launches == 1 and dy.shape == (n, d) and negdiv.shape == (n,)
    dy32, negdiv32, none = composition(func, t, y)
    dy64, negdiv64 = field64(func, t, y)
    assert none == 0
    for tag, got, c32, c64 in (("dy", dy, dy32, dy64), ("negdiv", negdiv, negdiv32, negdiv64)):
        bound = 1e-5 * scale_of(c64) + 4 * worst(c32, c64)
        assert worst(got, c64) <= bound, (tag, worst(got, c64), bound)


# ---- the field: beyond the limits ------------------------------------------------------------------------------------

def _beyond():
    base = dict(d=3, hidden=(8, 8))
    return {
        "d17": (dict(d=17, hidden=(8,)), None),
        "width65": (dict(d=3, hidden=(65,)), None),
        "five_hidden": (dict(d=3, hidden=(8,) * 5), None),
        "hyper": (dict(base, layer_type="hyper"), None),
        "blend": (dict(base, layer_type="blend"), None),
        "act_norm": (dict(base, act_norm=True), None),
        "transposed": (base, "transposed"),
        "requires_grad": (base, "requires_grad"),
        "option_off": (base, "option_off"),
        "rows_over_the_budget": (dict(d=2, hidden=(8,)), "rows"),
    }


@pytest.mark.parametrize("what", sorted(_beyond()))
def test_beyond_the_limits_takes_the_composition(what):
    kw, how = _beyond()[what]
    func = make_func(seed=7, gain=1.5, **kw).to(DEV)
    if what == "act_norm":
        with torch.no_grad():
            for norm in (func.diffeq.t_actnorm, func.diffeq.x_actnorm):
                norm.log_scale.add_(0.2)
                norm.shift.add_(0.1)
    d = kw["d"]
    count = ops.CNF_KERNEL_MAX_LANES // ops.cnf_group_lanes(d) + 1 if how == "rows" else 9
    y = rows(count, d, seed=70)
    t = torch.tensor(0.6, device=DEV)
    if how == "transposed":
        y = rows(d, 9, seed=70).t()
        assert not y.is_contiguous()
    func.before_odeint()
    with ops.KernelTimer("fc_cnf_field") as timer:
        if how == "requires_grad":
            dy, negdiv = func(t, (y.clone().requires_grad_(True), None))
            assert dy.requires_grad and negdiv.requires_grad
        elif how == "option_off":
            with torch.no_grad(), options.override(cnf_kernels=False):
                dy, negdiv = func(t, (y, None))
        else:
            with torch.no_grad():
                dy, negdiv = func(t, (y, None))
    assert len(timer.pairs) == 0 and func.num_evals() == 1.0
    with torch.no_grad():
        dy_c, negdiv_c = func._composition(t, (y, None))
    assert torch.equal(dy.detach(), dy_c) and torch.equal(negdiv.detach(), negdiv_c)
    if what == "act_norm":          # the float32 device kernels of ActNorm have no float64 twin: spell the net out
        net = copy.deepcopy(func.diffeq).double()
        y64 = (y.double() * net.x_actnorm.log_scale.exp() + net.x_actnorm.shift).requires_grad_(True)
        t64 = t.double() * net.t_actnorm.log_scale.exp()[0] + net.t_actnorm.shift[0]
        out = y64
        for index, layer in enumerate(net.layers):
            out = layer(t64, out)
            out = torch.tanh(out) if index < len(net.layers) - 1 else out
        assert worst(dy, out) <= 1e-5 * scale_of(out)
        return
    if how in ("option_off", "transposed", "requires_grad", "rows"):  # within the limits otherwise: the kernel agrees
        with options.override(cnf_kernels="force"):
            dy_k, negdiv_k, launches = evaluate(func, t, y.contiguous())
        dy64, negdiv64 = field64(func, 0.6, y.contiguous())
        assert launches == 1
        assert worst(dy_k, dy64) <= 1e-5 * scale_of(dy64) + 4 * worst(dy_c, dy64)
        assert worst(negdiv_k, negdiv64) <= 1e-5 * scale_of(negdiv64) + 4 * worst(negdiv_c.reshape(-1), negdiv64)


def test_training_mode_and_float64_take_the_composition():
    func = make_func(3, (8, 8), seed=8).to(DEV)
    y = rows(5, 3, seed=80)
    with ops.KernelTimer("fc_cnf_field") as timer:
        func.train()
        func(0.2, (y, None))
        func.eval()
        with torch.no_grad():
            copy.deepcopy(func).double()(0.2, (y.double(), None))
            copy.deepcopy(func).cpu()(0.2, (y.cpu(), None))
    assert len(timer.pairs) == 0


# ---- the field: rows ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("d,hidden", [(2, (64, 64, 64)), (7, (17,)), (16, (33, 5))])
def test_rows_are_independent_bitwise(d, hidden):
    func = make_func(d, hidden, seed=9, gain=1.5).to(DEV)
    y = rows(65, d, seed=90)
    dy, negdiv, _ = evaluate(func, 0.4, y)
    again = evaluate(func, 0.4, y)
    assert torch.equal(again[0], dy) and torch.equal(again[1], negdiv)
    for row in (0, 31, 64):
        alone = evaluate(func, 0.4, y[row:row + 1].clone())
        assert torch.equal(alone[0][0], dy[row]) and torch.equal(alone[1][0], negdiv[row])
    poisoned = y.clone()
    poisoned[3] = float("nan")
    dy_p, negdiv_p, _ = evaluate(func, 0.4, poisoned)
    keep = torch.arange(65, device=DEV) != 3
    assert torch.equal(dy_p[keep], dy[keep]) and torch.equal(negdiv_p[keep], negdiv[keep])
    assert torch.isnan(dy_p[3]).all() and torch.isnan(negdiv_p[3])


# ---- the integrator: fixed-step solvers ------------------------------------------------------------------------------

def solve(flow, z, reverse=False):
    """``(z_t, delta logp [N], launches of fc_cnf_integrate, launches of fc_cnf_field)``."""
    with torch.no_grad(), ops.KernelTimer("fc_cnf_integrate") as whole, ops.KernelTimer("fc_cnf_field") as single:
        z_t, logp_t = flow(z, torch.zeros(z.shape[0], 1, device=z.device), reverse=reverse)
    return z_t, logp_t.reshape(-1), len(whole.pairs), len(single.pairs)


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("d,hidden", [(2, (64, 64, 64)), (16, (32, 32))])
@pytest.mark.parametrize("method", ["rk4", "euler", "midpoint"])
def test_fixed_step_solve_is_one_launch(method, d, hidden, reverse):
    func = make_func(d, hidden, seed=11, gain=1.5).to(DEV)
    flow = make_cnf(func, solver=method, steps=8).to(DEV)
    z = rows(65, d, seed=110)
    z_t, logp_t, whole, single = solve(flow, z, reverse)
    assert (whole, single) == (1, 0)
    assert flow.num_evals() == 8 * {"euler": 1, "midpoint": 2, "rk4": 4}[method]
    t0, t1 = (1.0, 0.0) if reverse else (0.0, 1.0)
    z_true, logp_true = rk_solve(func, z, t0, t1, 8, method)
    with options.override(cnf_kernels=False):
        z_c, logp_c, none, none_either = solve(flow, z, reverse)
    assert (none, none_either) == (0, 0)
    for tag, got, comp, true in (("z", z_t, z_c, z_true), ("logp", logp_t, logp_c, logp_true)):
        bound = 1e-5 * scale_of(true) + 4 * worst(comp, true)
        assert worst(got, true) <= bound, (tag, worst(got, true), bound)
    assert float(logp_true.abs().max()) > 1e-3


def test_solve_with_an_initial_logp_and_without_one():
    func = make_func(3, (17,), seed=12, gain=1.5).to(DEV)
    flow = make_cnf(func, solver="rk4", steps=4).to(DEV)
    z = rows(10, 3, seed=120)
    start = torch.randn(10, 1, generator=torch.Generator().manual_seed(121)).to(DEV)
    with torch.no_grad(), ops.KernelTimer("fc_cnf_integrate") as whole:
        z_a, logp_a = flow(z, start)
        z_b, logp_b = flow(z, torch.zeros(10, 1, device=DEV))
        z_only = flow(z)
        z_three = flow(z, integration_times=torch.tensor([0.0, 0.5, 1.0]))      # more than two: the host loop
    assert len(whole.pairs) == 3 and logp_a.shape == (10, 1)
    assert torch.equal(z_a, z_b) and torch.equal(z_only, z_a)
    assert worst(logp_a, start + logp_b) <= 4e-7 * scale_of(logp_a)      # one float32 rounding of the sum
    assert z_three.shape == (3, 10, 3) and worst(z_three[2], z_a) <= 1e-5 * scale_of(z_a)


def test_affine_known_answer_on_the_kernel():
    func = make_func(3, (), layer_type="ignore", seed=5)
    layer = func.diffeq.layers[0]._layer
    w, b = layer.weight.detach().double().numpy(), layer.bias.detach().double().numpy()
    m = np.zeros((4, 4))
    m[:3, :3], m[:3, 3] = w, b
    e = scipy.linalg.expm(m)
    flow = make_cnf(func, solver="rk4", steps=64).to(DEV)
    z = rows(33, 3, seed=50)
    z_t, logp_t, whole, single = solve(flow, z)
    expected = z.double().cpu().numpy() @ e[:3, :3].T + e[:3, 3]
    assert (whole, single) == (1, 0)
    assert float(np.abs(z_t.double().cpu().numpy() - expected).max()) <= 1e-5 * max(1.0, float(np.abs(expected).max()))
    assert float((logp_t.double().cpu() + np.trace(w)).abs().max()) <= 1e-5 * max(1.0, abs(float(np.trace(w))))


# ---- dopri5: the host loop over the field kernel ---------------------------------------------------------------------

def test_dopri5_runs_the_host_loop_over_the_field_kernel():
    func = make_func(2, (64, 64, 64), seed=13, gain=1.5).to(DEV)
    flow = make_cnf(func, solver="dopri5", tol=1e-5).to(DEV)
    z = rows(65, 2, seed=130)
    z_t, logp_t, whole, single = solve(flow, z)
    assert whole == 0 and single == flow.num_evals() and single >= 8
    z_true, logp_true = rk_solve(func, z, 0.0, 1.0, 256, "rk4")
    with options.override(cnf_kernels=False):
        z_c, logp_c, _, none = solve(flow, z)
    assert none == 0
    for tag, got, comp, true in (("z", z_t, z_c, z_true), ("logp", logp_t, logp_c, logp_true)):
        bound = 1e-5 * scale_of(true) + 4 * worst(comp, true)
        assert worst(got, true) <= bound, (tag, worst(got, true), bound)


# ---- flow level -------------------------------------------------------------------------------------------------------

def _density64(func, x, steps):
    z, delta = rk_solve(func, x, 0.0, 1.0, steps, "rk4")
    return -0.5 * z.square().sum(dim=1) - 0.5 * x.shape[1] * math.log(2 * math.pi) - delta


def test_flow_density_sampling_and_graph_replay():
    func = make_func(2, (64, 64, 64), seed=14, gain=1.5).to(DEV)
    flow = flows.Flow(CNFTransform(make_cnf(func, solver="rk4", steps=64)), distributions.StandardNormal([2]))
    flow = flow.to(DEV).eval()
    x = rows(65, 2, seed=140, scale=1.0)
    with torch.no_grad(), ops.KernelTimer("fc_cnf_integrate") as whole:
        log_prob = flow.log_prob(x)
        torch.manual_seed(141)
        samples, sample_log_prob = flow.sample_and_log_prob(65)
    assert len(whole.pairs) == 2
    with torch.no_grad(), options.override(cnf_kernels=False):
        log_prob_c = flow.log_prob(x)
        torch.manual_seed(141)
        samples_c, sample_log_prob_c = flow.sample_and_log_prob(65)
    true = _density64(func, x, 64)
    assert worst(log_prob, true) <= 1e-5 * scale_of(true) + 4 * worst(log_prob_c, true)
    true_s, true_c = _density64(func, samples, 64), _density64(func, samples_c, 64)
    assert worst(sample_log_prob, true_s) <= 1e-5 * scale_of(true_s) + 4 * worst(sample_log_prob_c, true_c)
    assert samples.shape == (65, 2) and torch.isfinite(samples).all()

    graphed = GraphedCall(flow.log_prob, x)
    assert torch.equal(graphed(x), log_prob)
    other = rows(65, 2, seed=142, scale=1.0)
    with torch.no_grad():
        expected = flow.log_prob(other)
    assert torch.equal(graphed(other), expected)
    assert flow._transform.cnf.num_evals() == 256.0
