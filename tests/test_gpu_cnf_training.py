"""Continuous normalizing flows trained on the GPU: one evaluation of ``ODEfunc`` as one autograd node of
``fc_cnf_field_train`` + ``fc_cnf_field_backward`` (options ``cnf_training``).

Bounds (none of them comes from what the kernels give): every entry -- ``dy``, ``negdiv``, the gradient with respect to
``y`` and to each parameter -- is held to ``1e-5 max(1, max|expected|) + 4 floor``:

* fixtures (tests/golden/cnf_train_*.npz): against the recorded float32 values with the recorded
  ``floor = max|ref32 - ref64|``;
* everything else: against the package's float64 composition on the same inputs and the same preset noise, the floor
  being ``max|composition32 - composition64|`` of that entry (tests/test_cnf_training_host.py pins the composition to
  the reference).

Launch counts are those of the C-ABI entries: exactly one of each per evaluation on the route, none off it.  Routes that
must stay the composition are compared bitwise with the option off.
"""
import copy
import math

import pytest
import torch

from flowconductor_amd import distributions, flows, ops, options, transforms
from flowconductor_amd.CNF import CNF, CNFTransform
from flowconductor_amd.CNF.neural_odes.wrappers.cnf_regularization import l2_regularzation_fn

import _cnf_training_util as U

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
MODES = ["approximate", "brute_force"]
KINDS = ["ignore", "concat", "concat_v2", "squash", "concatsquash"]
ACTS = ["tanh", "relu", "softplus", "elu", "swish", "square", "identity"]
DIMS = [1, 2, 3, 7, 8, 15, 16]
ROWS = [1, 63, 64, 65, 257]
HIDDEN = [(), (5,), (17, 33), (64, 64, 64)]
# every (D, N), (D, hidden) and (N, hidden) pair occurs: hidden walks with the sum of the two indices
GRID = [(d, n, HIDDEN[(i + j) % 4], KINDS[(i + 2 * j) % 5], ACTS[(3 * i + j) % 7], (i + j) % 2 == 1,
         1 if j % 2 else 0.75)
        for i, d in enumerate(DIMS) for j, n in enumerate(ROWS)]
# relu / elu cells: a seed for which no hidden pre-activation of the float64 composition lies within 1e-4 of the kink
# (the test asserts it); found by walking the seeds upwards from the default on the host
KINK_SEEDS = {(1, 65): 1021, (3, 257): 651, (8, 65): 485, (15, 64): 1175, (16, 257): 3702}


def grid_seed(d, n):
    return KINK_SEEDS.get((d, n), 300 + 10 * d + n)


def three_ways(func, data, preset=True):
    """One evaluation on the kernels, on the float32 composition and on the float64 one."""
    got, forward, backward = U.evaluate(func, data, route="force", preset=preset)
    assert (forward, backward) == (1, 1)
    c32, none, none_either = U.evaluate(func, data, route=False, preset=preset)
    assert (none, none_either) == (0, 0)
    c64, _, _ = U.evaluate(func, data, route=False, dtype=torch.float64, preset=preset)
    return got, c32, c64


# ---- fixtures ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,mode", U.FIXTURES)
def test_training_fixture_on_the_kernels(name, mode):
    func, g = U.load_train_case(name, mode)
    func = func.to(DEV)
    data = U.fixture_data(g, DEV)
    got, forward, backward = U.evaluate(func, data, route="force")
    assert (forward, backward) == (1, 1) and func.num_evals() == 1.0
    for key in got:
        expected = torch.from_numpy(g[key + "32"])
        bound = 1e-5 * U.scale_of(expected) + 4 * float(g["floor::" + key])
        assert U.worst(got[key], expected) <= bound, (key, U.worst(got[key], expected), bound)
    off, forward, backward = U.evaluate(func, data, route=False)
    assert (forward, backward) == (0, 0) and set(off) == set(got)
    by_size, forward, backward = U.evaluate(func, data, route=True)      # the measured size rule decides
    pays = ops.cnf_train_rows_pay(data.y.shape[0], data.y.shape[1], mode == "approximate")
    assert (forward, backward) == ((1, 1) if pays else (0, 0))
    for key in got:
        assert torch.equal(by_size[key], got[key] if pays else off[key]), key


# ---- shape grid -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("d,n,hidden,kind,act,residual,scale", GRID)
def test_training_shape_grid(d, n, hidden, kind, act, residual, scale, mode):
    func = U.make_train_func(d, hidden, layer_type=kind, nonlinearity=act, mode=mode, seed=grid_seed(d, n),
                             residual=residual, scale_output=scale).to(DEV)
    data = U.make_data(n, d, seed=grid_seed(d, n) + 1, device=DEV)
    if act in ("relu", "elu") and hidden:
        assert float(U.hidden_preactivations(func, data).abs().min()) > 1e-4
    got, c32, c64 = three_ways(func, data)
    assert got["dy"].shape == (n, d) and got["negdiv"].shape == (n, 1)
    U.assert_within(got, c32, c64, (d, n, hidden, kind, act, mode))


def test_eval_mode_with_a_gradient_is_exact_on_the_kernels():
    func = U.make_train_func(3, (17, 33), nonlinearity="softplus", seed=31).to(DEV).eval()
    data = U.make_data(65, 3, seed=32, device=DEV)
    got, c32, c64 = three_ways(func, data, preset=False)        # no noise is drawn or used: the exact divergence
    assert func._e is None
    U.assert_within(got, c32, c64, "eval")


def test_training_mode_without_a_gradient_is_the_forward_launch_alone():
    func = U.make_train_func(3, (17, 33), seed=33).to(DEV)
    data = U.make_data(65, 3, seed=34, device=DEV)
    got, _, _ = U.evaluate(func, data, route="force")
    func.before_odeint(e=data.e)
    with torch.no_grad(), options.override(cnf_training="force"), ops.KernelTimer("fc_cnf_field_train") as forward, \
            ops.KernelTimer("fc_cnf_field_backward") as backward, ops.KernelTimer("fc_cnf_field") as field:
        dy, negdiv = func(data.t, (data.y, None))
    assert (len(forward.pairs), len(backward.pairs), len(field.pairs)) == (1, 0, 0)
    assert not dy.requires_grad and torch.equal(dy, got["dy"]) and torch.equal(negdiv, got["negdiv"])


def test_noise_is_drawn_where_the_composition_draws_it():
    func = U.make_train_func(3, (8, 8), seed=35).to(DEV)
    data = U.make_data(9, 3, seed=36, device=DEV)
    drawn = {}
    for route in ("force", False):
        torch.manual_seed(37)
        U.evaluate(func, data, route=route, preset=False)
        drawn[route] = (func._e.clone(), torch.randn(3, device=DEV))
    assert torch.equal(drawn["force"][0], drawn[False][0]) and torch.equal(drawn["force"][1], drawn[False][1])
    func.rademacher = True
    torch.manual_seed(38)
    got, forward, backward = U.evaluate(func, data, route="force", preset=False)
    assert (forward, backward) == (1, 1) and set(func._e.unique().tolist()) == {-1.0, 1.0}
    kept = data._replace(e=func._e.clone())
    c32, _, _ = U.evaluate(func, kept, route=False)
    c64, _, _ = U.evaluate(func, kept, route=False, dtype=torch.float64)
    U.assert_within(got, c32, c64, "rademacher")


# ---- the sums over rows -----------------------------------------------------------------------------------------------

# rows of one block - 1, exactly, + 1; three blocks and a row; past the grid cap, where a block owns a second tile
@pytest.mark.parametrize("what,extra", [("rows", -1), ("rows", 0), ("rows", 1), ("3rows", 1), ("grid", 1)])
def test_reduction_edges(what, extra):
    d, hidden = 2, (5,)
    per_block = ops.cnf_backward_rows(d, hidden, True)
    assert per_block >= 32
    n = {"rows": per_block, "3rows": 3 * per_block, "grid": ops.CNF_BACKWARD_MAX_BLOCKS * per_block}[what] + extra
    func = U.make_train_func(d, hidden, seed=41).to(DEV)
    data = U.make_data(n, d, seed=42, device=DEV)
    got, c32, c64 = three_ways(func, data)
    U.assert_within(got, c32, c64, (what, extra, n))


def _raw(func, data, hutchinson=True):
    plan = func._kernel_plan()
    kw = func._kernel_args(plan)
    kw.pop("evals")
    e = data.e if hutchinson else None
    return lambda y, e=e, c1=data.c1, c2=data.c2: ops.cnf_field_backward(
        data.t, y, e, g_dy=c1, g_negdiv=c2.reshape(-1).contiguous(), **kw)


@pytest.mark.parametrize("d,hidden,hutchinson", [(2, (64, 64, 64), True), (7, (17,), False), (16, (33, 5), True)])
def test_backward_is_bitwise_reproducible_and_rows_are_independent(d, hidden, hutchinson):
    func = U.make_train_func(d, hidden, seed=43).to(DEV)
    n = 3 * ops.cnf_backward_rows(d, hidden, hutchinson) + 1
    data = U.make_data(n, d, seed=44, device=DEV)
    backward = _raw(func, data, hutchinson)
    with ops.KernelTimer("fc_cnf_field_backward") as timer:
        g_y, g_image = backward(data.y)
        g_y_again, g_image_again = backward(data.y)
    assert len(timer.pairs) == 2
    assert torch.equal(g_image, g_image_again) and torch.equal(g_y, g_y_again)
    assert g_image.shape == (ops.cnf_image_floats(d, hidden),) and float(g_image.abs().max()) > 0
    for row in (0, n // 2, n - 1):
        piece = slice(row, row + 1)
        alone = _raw(func, data._replace(e=data.e[piece].clone(), c1=data.c1[piece].clone(),
                                         c2=data.c2[piece].clone()), hutchinson)(data.y[piece].clone())
        assert torch.equal(alone[0][0], g_y[row]), row
    poisoned = data.y.clone()
    poisoned[3] = float("nan")
    g_y_p, g_image_p = backward(poisoned)
    keep = torch.arange(n, device=DEV) != 3
    assert torch.equal(g_y_p[keep], g_y[keep]) and torch.isnan(g_y_p[3]).all()
    assert torch.isnan(g_image_p).any()


def test_raw_wrappers_check_their_arguments():
    func = U.make_train_func(3, (8,), seed=45).to(DEV)
    data = U.make_data(5, 3, seed=46, device=DEV)
    kw = func._kernel_args(func._kernel_plan())
    with pytest.raises(ValueError):
        ops.cnf_field_train(0.1, data.y, data.e[:4].contiguous(), **kw)
    with pytest.raises(ValueError):
        ops.cnf_field_train(0.1, data.y, data.e.double(), **kw)
    with pytest.raises(ValueError):
        ops.cnf_field_train(0.1, data.y, data.e, **dict(kw, hidden=(8, 8, 8, 8)))
    wide = U.make_train_func(3, (8, 8, 8, 8), seed=45).to(DEV)
    with pytest.raises(ValueError):
        ops.cnf_field_train(0.1, data.y, data.e, **wide._kernel_args(wide._kernel_plan()))
    with pytest.raises(ValueError):
        ops.cnf_backward_rows(3, (8, 8, 8, 8), True)
    dy, negdiv = ops.cnf_field_train(0.1, data.y, data.e, **kw)
    assert dy.shape == (5, 3) and negdiv.shape == (5,) and func.num_evals() == 1.0


# ---- what keeps the composition ---------------------------------------------------------------------------------------

def _keep_noise(func, e):
    """``before_odeint`` of ``func`` from now on presets the noise ``e`` (a solve calls it without arguments)."""
    original = func.before_odeint
    func.before_odeint = lambda *unused, **also_unused: original(e=e)


def _solve_and_differentiate(flow, z, route):
    z = z.clone().requires_grad_(True)
    with options.override(cnf_training=route), ops.KernelTimer("fc_cnf_field_train") as forward, \
            ops.KernelTimer("fc_cnf_field_backward") as backward:
        z_t, logp_t = flow(z, torch.zeros(z.shape[0], 1, device=z.device))
        loss = z_t.square().sum() + logp_t.sum() + sum((r.sum() for r in flow.get_regularization_states()), 0.0)
        grads = torch.autograd.grad(loss, [z] + list(flow.parameters()))
    return [z_t.detach(), logp_t.detach()] + list(grads), len(forward.pairs) + len(backward.pairs)


@pytest.mark.parametrize("what", ["regularised", "train_T"])
def test_solves_that_keep_the_composition(what):
    func = U.make_train_func(3, (8, 8), seed=51).to(DEV)
    data = U.make_data(9, 3, seed=52, device=DEV)
    _keep_noise(func, data.e)
    extra = dict(regularization_fns=[l2_regularzation_fn]) if what == "regularised" else dict(train_T=True)
    flow = CNF(func, solver="rk4", **extra).to(DEV).train()
    flow.solver_options = {"step_size": 0.25}
    forced, launches = _solve_and_differentiate(flow, data.y, "force")
    plain, none = _solve_and_differentiate(flow, data.y, False)
    assert (launches, none) == (0, 0) and len(forced) == len(plain)
    for a, b in zip(forced, plain):
        assert torch.equal(a, b)


@pytest.mark.parametrize("what", ["hyper", "act_norm", "transposed", "four_hidden_layers"])
def test_evaluations_that_keep_the_composition(what):
    kw = dict(hyper=dict(layer_type="hyper"), act_norm=dict(act_norm=True)).get(what, {})
    hidden = (8, 8, 8, 8) if what == "four_hidden_layers" else (8, 8)
    func = U.make_train_func(3, hidden, seed=53, **kw).to(DEV)
    data = U.make_data(9, 3, seed=54, device=DEV)
    if what == "transposed":
        data = data._replace(y=U.make_data(3, 9, seed=54, device=DEV).y.t())
        assert not data.y.is_contiguous()
    if what == "act_norm":      # as after its data-dependent initialisation (one t has no spread to take it from)
        with torch.no_grad():
            for norm in (func.diffeq.t_actnorm, func.diffeq.x_actnorm):
                norm.initialized.fill_(True)
                norm.log_scale.add_(0.2)
                norm.shift.add_(0.1)
    forced, forward, backward = U.evaluate(func, data, route="force")
    plain, _, _ = U.evaluate(func, data, route=False)
    assert (forward, backward) == (0, 0) and set(forced) == set(plain)
    for key in plain:
        assert torch.equal(forced[key], plain[key]), key


def test_double_backward_raises():
    func = U.make_train_func(3, (8, 8), seed=55).to(DEV)
    data = U.make_data(9, 3, seed=56, device=DEV)
    func.before_odeint(e=data.e)
    y = data.y.clone().requires_grad_(True)
    with options.override(cnf_training="force"):
        dy, negdiv = func(data.t, (y, None))
        with pytest.raises(RuntimeError, match="cnf_training=False"):
            torch.autograd.grad(dy.sum() + negdiv.sum(), y, create_graph=True)


# ---- end to end -------------------------------------------------------------------------------------------------------

def _flow(mode, solver, seed):
    func = U.make_train_func(2, (16, 16), mode=mode, seed=seed)
    cnf = CNF(func, solver=solver, atol=1e-5, rtol=1e-5)
    if solver != "dopri5":
        cnf.solver_options = {"step_size": 0.25}
    return flows.Flow(transforms.CompositeTransform([CNFTransform(cnf)]), distributions.StandardNormal([2])).train()


CNF_PREFIX = "_transform._transforms.0.cnf."


def _cnf_of(flow):
    return flow._transform._transforms[0].cnf


def _func_of(flow):
    return _cnf_of(flow).odefunc


def _loss_gradients(flow, x, route):
    with options.override(cnf_training=route), ops.KernelTimer("fc_cnf_field_train") as forward, \
            ops.KernelTimer("fc_cnf_field_backward") as backward:
        loss = -flow.log_prob(x).mean()
        nodes = _nodes_behind(loss)
        grads = torch.autograd.grad(loss, list(flow.parameters()))
    names = [k for k, _ in flow.named_parameters()]
    out = dict(zip(names, grads))
    out["loss"] = loss.detach().reshape(1)
    return out, len(forward.pairs), len(backward.pairs), nodes


def _nodes_behind(loss):
    """Evaluations of the ODE function the loss depends on: the ``_CnfFieldFunction`` nodes of its graph (an adaptive
    solver also evaluates steps it rejects and a last slope it never uses; those have no backward to run)."""
    seen, stack, count = set(), [loss.grad_fn], 0
    while stack:
        node = stack.pop()
        if node is None or node in seen:
            continue
        seen.add(node)
        count += type(node).__name__ == "_CnfFieldFunctionBackward"
        stack.extend(fn for fn, _ in node.next_functions)
    return count


def _loss_gradients64(cnf64, x):
    """The same loss from a float64 copy of the CNF, the standard normal density written out."""
    z, delta = cnf64(x, torch.zeros(x.shape[0], 1, dtype=x.dtype, device=x.device))
    log_prob = -0.5 * z.square().sum(dim=1) - 0.5 * x.shape[1] * math.log(2 * math.pi) - delta.reshape(-1)
    loss = -log_prob.mean()
    grads = torch.autograd.grad(loss, list(cnf64.parameters()))
    out = {CNF_PREFIX + k: g for (k, _), g in zip(cnf64.named_parameters(), grads)}
    out["loss"] = loss.detach().reshape(1)
    return out


@pytest.mark.parametrize("mode,solver", [("approximate", "rk4"), ("brute_force", "rk4"), ("brute_force", "dopri5")])
def test_flow_training_step(mode, solver):
    flow = _flow(mode, solver, seed=61).to(DEV)
    cnf64 = copy.deepcopy(_cnf_of(flow)).double()
    data = U.make_data(65, 2, seed=62, device=DEV)
    _keep_noise(_func_of(flow), data.e)
    _keep_noise(cnf64.odefunc, data.e.double())
    x = data.y / 1.5
    got, forward, backward, nodes = _loss_gradients(flow, x, "force")
    evals = _func_of(flow).num_evals()
    assert forward == evals and backward == nodes and evals >= (16 if solver == "rk4" else 8)
    # every fixed step counts; an accepted dopri5 step has six slopes with a weight
    assert nodes == evals if solver == "rk4" else 6 <= nodes <= evals
    c32, none, none_either, no_nodes = _loss_gradients(flow, x, False)
    assert (none, none_either, no_nodes) == (0, 0, 0)
    c64 = _loss_gradients64(cnf64, x.double())
    U.assert_within(got, c32, c64, (mode, solver))


def test_two_solves_then_two_backwards():
    flow = _flow("approximate", "rk4", seed=63).to(DEV)
    data = U.make_data(65, 2, seed=64, device=DEV)
    _keep_noise(_func_of(flow), data.e)
    x = data.y / 1.5
    expected, _, _, _ = _loss_gradients(flow, x, "force")
    with options.override(cnf_training="force"), ops.KernelTimer("fc_cnf_field_backward") as backward:
        first = -flow.log_prob(x).mean()
        second = -flow.log_prob(x).mean()
        grads_first = torch.autograd.grad(first, list(flow.parameters()))
        grads_second = torch.autograd.grad(second, list(flow.parameters()))
    assert len(backward.pairs) == 32
    for a, b, (name, _) in zip(grads_first, grads_second, flow.named_parameters()):
        assert torch.equal(a, b) and torch.equal(a, expected[name]), name
