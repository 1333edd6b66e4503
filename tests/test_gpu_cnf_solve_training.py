"""Continuous normalizing flows trained on the GPU with the whole fixed-step solve as ONE autograd node:
``fc_cnf_integrate_train`` forward, ``fc_cnf_integrate_backward`` backward (options ``cnf_solve_training``).

Bounds (none of them comes from what the kernels give): every entry -- ``z_t``, ``logp_t``, the gradient with respect to
``z``, ``logp`` and each parameter -- is held to ``1e-5 max(1, max|c64|) + 4 max|c32 - c64|`` (``U.assert_within``),
``c64`` the package's float64 solve and ``c32`` its float32 composition, both CNF training options off, on the same
inputs and the same preset noise.  tests/test_cnf_solve_training_host.py pins the float64 solve to an independent loop
and the kernel's reverse sweep to autograd.  The comparison with the existing per-evaluation node has no composition to
take a floor from: it is held to ``1e-5 max(1, max|expected|)`` alone.

Launch counts are those of the C-ABI entries: exactly one of each new entry per solve on the route and none of
``fc_cnf_field_train``; none off it.  Routes that decline are compared bitwise with the option off.
"""
import copy
import math

import pytest
import torch

from flowconductor_amd import distributions, flows, ops, options, transforms
from flowconductor_amd.CNF import CNF, CNFTransform
from flowconductor_amd.CNF.neural_odes.wrappers.cnf_regularization import l2_regularzation_fn

import _cnf_solve_training_util as U

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
MODES = ["approximate", "brute_force"]
KINDS = ["ignore", "concat", "concat_v2", "squash", "concatsquash"]
ACTS = ["tanh", "softplus", "swish", "identity"]
DIMS = [1, 2, 3, 7, 8, 15, 16]
ROWS = [1, 63, 64, 65, 257]
HIDDEN = [(), (5,), (17, 33), (64, 64, 64)]
# every (D, N), (D, hidden) and (N, hidden) pair occurs; the method, the step count, the direction, the residual and
# scale_output walk with the indices: (d, n, hidden, kind, act, method, steps, reverse, residual, scale)
GRID = [(d, n, HIDDEN[(i + j) % 4], KINDS[(i + 2 * j) % 5], ACTS[(3 * i + j) % 4], U.METHODS[(i + j) % 3],
         1 + (i + 2 * j) % 3, (5 * i + j) % 2 == 1, (i + j) % 2 == 1, 1 if j % 2 else 0.75)
        for i, d in enumerate(DIMS) for j, n in enumerate(ROWS)]
# relu / elu: a seed for which no hidden pre-activation of the float64 solve, at any stage input, lies within 1e-4 of the
# kink (the test asserts it); found by walking the seeds upwards on the host
KINKED = [("relu", 3, 65, (9, 5), "rk4", 2, False, 1001), ("elu", 8, 63, (5,), "midpoint", 3, True, 1000)]


def three_ways(cnf, data, logp, e, reverse=False):
    """One solve on the kernels, on the float32 composition and on the float64 one."""
    got, forward, backward, field = U.evaluate(cnf, data.y, logp, data.c1, data.c2, route="force", e=e, reverse=reverse)
    assert (forward, backward, field) == (1, 1, 0)
    evals = cnf.num_evals()
    c32, *launches = U.evaluate(cnf, data.y, logp, data.c1, data.c2, route=False, e=e, reverse=reverse)
    assert launches == [0, 0, 0] and cnf.num_evals() == evals
    c64, *_ = U.evaluate(cnf, data.y, logp, data.c1, data.c2, route=False, e=e, reverse=reverse, dtype=torch.float64)
    return got, c32, c64, evals


def build(d, hidden, kind="concatsquash", act="tanh", mode="approximate", method="rk4", steps=2, residual=False,
          scale=1, seed=0):
    func = U.make_train_func(d, hidden, layer_type=kind, nonlinearity=act, mode=mode, seed=seed, residual=residual,
                             scale_output=scale)
    return U.make_cnf(func, solver=method, steps=steps).to(DEV)


# ---- shape grid -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("d,n,hidden,kind,act,method,steps,reverse,residual,scale", GRID)
def test_solve_shape_grid(d, n, hidden, kind, act, method, steps, reverse, residual, scale, mode):
    seed = 400 + 10 * d + n
    cnf = build(d, hidden, kind, act, mode, method, steps, residual, scale, seed)
    data = U.make_data(n, d, seed=seed + 1, device=DEV)
    got, c32, c64, evals = three_ways(cnf, data, torch.flip(data.c2, [0]), data.e, reverse)
    assert evals == steps * U.STAGES[method]
    assert got["z_t"].shape == (n, d) and got["logp_t"].shape == (n, 1)
    U.assert_within(got, c32, c64, (d, n, hidden, kind, act, method, steps, reverse, mode))


@pytest.mark.parametrize("act,d,n,hidden,method,steps,reverse,seed", KINKED)
def test_solve_with_a_kinked_activation(act, d, n, hidden, method, steps, reverse, seed):
    cnf = build(d, hidden, "concat", act, "approximate", method, steps, seed=seed)
    data = U.make_data(n, d, seed=seed + 1, device=DEV)
    assert float(U.hidden_preactivations(cnf, data.y, data.e, reverse).abs().min()) > 1e-4
    got, c32, c64, evals = three_ways(cnf, data, torch.flip(data.c2, [0]), data.e, reverse)
    assert evals == steps * U.STAGES[method]
    U.assert_within(got, c32, c64, (act, seed))


# ---- bitwise ----------------------------------------------------------------------------------------------------------

def _raw_args(cnf, method, steps, t0=0.0, t1=1.0):
    func = cnf.odefunc
    kw = func._kernel_args(func._kernel_plan())
    kw.pop("evals")
    kw.update(t0=t0, t1=t1, steps=steps, method=ops.CNF_METHODS[method])
    return kw


@pytest.mark.parametrize("method", U.METHODS)
@pytest.mark.parametrize("d", [2, 16])
def test_forward_without_e_and_tape_is_cnf_integrate(d, method):
    cnf = build(d, (17, 33), method=method, steps=3, seed=71)
    data = U.make_data(65, d, seed=72, device=DEV)
    kw = _raw_args(cnf, method, 3, t0=0.2, t1=1.1)
    logp = data.c2.reshape(-1).contiguous()
    with ops.KernelTimer(U.NEW_ENTRIES[0]) as timer:
        z_t, logp_t = ops.cnf_integrate_train(data.y, logp, None, tape=False, **kw)
        z_t_taped, logp_t_taped, tape = ops.cnf_integrate_train(data.y, logp, None, tape=True, **kw)
    assert len(timer.pairs) == 2
    z_ref, logp_ref = ops.cnf_integrate(data.y, logp, **kw)
    assert torch.equal(z_t, z_ref) and torch.equal(logp_t, logp_ref)
    assert torch.equal(z_t_taped, z_ref) and torch.equal(logp_t_taped, logp_ref)
    assert tape.shape == (3 * U.STAGES[method], 65, d) and torch.equal(tape[0], data.y)


@pytest.mark.parametrize("d,hidden,hutchinson", [(2, (64, 64, 64), True), (7, (17,), False), (16, (33, 5), True)])
def test_backward_is_bitwise_reproducible_and_rows_are_independent(d, hidden, hutchinson):
    cnf = build(d, hidden, method="rk4", steps=2, seed=73)
    data = U.make_data(65, d, seed=74, device=DEV)
    kw = _raw_args(cnf, "rk4", 2)
    g_logp = data.c2.reshape(-1).contiguous()

    def sweep(rows):
        e = data.e[rows].contiguous() if hutchinson else None
        _, _, tape = ops.cnf_integrate_train(z[rows].contiguous(), None, e, tape=True, **kw)
        return ops.cnf_integrate_backward(tape, e, kw["image"], data.c1[rows].contiguous(), g_logp[rows].contiguous(),
                                          **{k: v for k, v in kw.items() if k != "image"})

    z, everything = data.y, slice(0, 65)
    with ops.KernelTimer(U.NEW_ENTRIES[1]) as timer:
        g_z, g_image = sweep(everything)
        g_z_again, g_image_again = sweep(everything)
    assert len(timer.pairs) == 2
    assert torch.equal(g_z, g_z_again) and torch.equal(g_image, g_image_again)
    assert g_image.shape == (ops.cnf_image_floats(d, hidden),) and float(g_image.abs().max()) > 0
    alone, _ = sweep(slice(64, 65))
    assert torch.equal(alone[0], g_z[64])
    z = data.y.clone()
    z[3] = float("nan")
    g_z_p, g_image_p = sweep(everything)
    keep = torch.arange(65, device=DEV) != 3
    assert torch.equal(g_z_p[keep], g_z[keep]) and torch.isnan(g_z_p[3]).all()
    assert torch.isnan(g_image_p).any()


def test_a_block_that_walks_over_several_tiles():
    d, hidden = 16, (64, 64, 64)
    per_block = ops.cnf_backward_rows(d, hidden, False)
    assert per_block == 2
    n = ops.CNF_BACKWARD_MAX_BLOCKS * per_block + 1
    cnf = build(d, hidden, mode="brute_force", method="rk4", steps=2, seed=75)
    data = U.make_data(n, d, seed=76, device=DEV)
    got, c32, c64, evals = three_ways(cnf, data, torch.flip(data.c2, [0]), data.e)
    assert evals == 8
    U.assert_within(got, c32, c64, ("tiles", n))


@pytest.mark.parametrize("hutchinson", [True, False])
def test_one_euler_step_is_the_existing_node(hutchinson):
    d, hidden, t0, t1 = 3, (17, 33), 0.25, 0.75
    cnf = build(d, hidden, kind="concatsquash", method="euler", steps=1, residual=True, scale=0.75, seed=77)
    data = U.make_data(65, d, seed=78, device=DEV)
    kw = _raw_args(cnf, "euler", 1, t0, t1)
    e = data.e if hutchinson else None
    g_logp = data.c2.reshape(-1).contiguous()
    _, _, tape = ops.cnf_integrate_train(data.y, None, e, tape=True, **kw)
    rest = {k: v for k, v in kw.items() if k != "image"}
    g_z, g_image = ops.cnf_integrate_backward(tape, e, kw["image"], data.c1, g_logp, **rest)
    h = t1 - t0
    field = {k: v for k, v in rest.items() if k not in ("t0", "t1", "steps", "method")}
    g_y, g_image_ref = ops.cnf_field_backward(t0, data.y, e, kw["image"], h * data.c1, h * g_logp, **field)
    for got, want in ((g_z - data.c1, g_y), (g_image, g_image_ref)):
        assert U.worst(got, want) <= 1e-5 * U.scale_of(want), (U.worst(got, want), U.scale_of(want))


# ---- end to end -------------------------------------------------------------------------------------------------------

class _Affine(transforms.Transform):
    """``y = x exp(log_scale) + shift`` in torch ops: a trainable layer in front of the CNF."""

    def __init__(self, features):
        super().__init__()
        self.log_scale = torch.nn.Parameter(torch.linspace(-0.2, 0.3, features))
        self.shift = torch.nn.Parameter(torch.linspace(0.1, -0.4, features))

    def forward(self, inputs, context=None):
        return inputs * self.log_scale.exp() + self.shift, self.log_scale.sum().expand(inputs.shape[0])

    def inverse(self, inputs, context=None):
        return (inputs - self.shift) * (-self.log_scale).exp(), -self.log_scale.sum().expand(inputs.shape[0])


def _flow(mode, seed, front=False):
    func = U.make_train_func(2, (16, 16), mode=mode, seed=seed)
    cnf = CNF(func, solver="rk4")
    cnf.solver_options = {"step_size": 0.25}
    layers = ([_Affine(2)] if front else []) + [CNFTransform(cnf)]
    return flows.Flow(transforms.CompositeTransform(layers), distributions.StandardNormal([2])).train().to(DEV), cnf


def _log_normal(z):
    return -0.5 * z.square().sum(dim=1) - 0.5 * z.shape[1] * math.log(2 * math.pi)


def _gradients(loss, model):
    out = {k: g for (k, _), g in zip(model.named_parameters(), torch.autograd.grad(loss, list(model.parameters())))}
    out["loss"] = loss.detach().reshape(1)
    return out


def _counted(flow, make_loss, solve=False, field=False):
    """The loss's gradients with respect to the flow's parameters and the launches of the two new entries and of
    fc_cnf_field_train."""
    with options.override(cnf_solve_training=solve, cnf_training=field), ops.KernelTimer(U.NEW_ENTRIES[0]) as forward, \
            ops.KernelTimer(U.NEW_ENTRIES[1]) as backward, ops.KernelTimer("fc_cnf_field_train") as evaluations:
        out = _gradients(make_loss(), flow)
    return out, [len(forward.pairs), len(backward.pairs), len(evaluations.pairs)]


def _flow64(flow):
    """A float64 copy of the flow's transforms (the standard normal density is written out)."""
    layers = copy.deepcopy(flow._transform._transforms).double()
    return layers


@pytest.mark.parametrize("front", [False, True])
@pytest.mark.parametrize("mode", MODES)
def test_flow_training_step(mode, front):
    flow, cnf = _flow(mode, seed=81, front=front)
    data = U.make_data(65, 2, seed=82, device=DEV)
    x = data.y / 1.5
    U.keep_noise(cnf.odefunc, data.e)
    got, launches = _counted(flow, lambda: -flow.log_prob(x).mean(), solve="force")
    assert launches == [1, 1, 0] and cnf.num_evals() == 16
    c32, none = _counted(flow, lambda: -flow.log_prob(x).mean())
    assert none == [0, 0, 0]
    layers = _flow64(flow)
    U.keep_noise(layers[-1].cnf.odefunc, data.e.double())
    z, logabsdet = x.double(), 0.0
    for layer in layers:
        z, delta = layer(z)
        logabsdet = logabsdet + delta
    loss = -(_log_normal(z) + logabsdet).mean()
    c64 = {"_transform._transforms." + k: v for k, v in _gradients(loss, layers).items() if k != "loss"}
    c64["loss"] = loss.detach().reshape(1)
    U.assert_within(got, c32, c64, (mode, front))
    if front:       # g_z of the solve reached the layer in front
        assert float(got["_transform._transforms.0.shift"].abs().max()) > 0


@pytest.mark.parametrize("mode", MODES)
def test_sample_and_log_prob_with_gradients(mode):
    flow, cnf = _flow(mode, seed=83)
    data = U.make_data(65, 2, seed=84, device=DEV)
    U.keep_noise(cnf.odefunc, data.e)

    def make_loss():
        torch.manual_seed(85)
        samples, log_prob = flow.sample_and_log_prob(65)
        return (0.1 * samples.square().sum(dim=1) + log_prob).mean()

    got, launches = _counted(flow, make_loss, solve="force")
    assert launches == [1, 1, 0] and cnf.num_evals() == 16
    c32, none = _counted(flow, make_loss)
    assert none == [0, 0, 0]
    torch.manual_seed(85)
    noise = torch.randn(65, 2, device=DEV).double()
    layers = _flow64(flow)
    U.keep_noise(layers[0].cnf.odefunc, data.e.double())
    samples, logabsdet = layers[0].inverse(noise)
    loss = (0.1 * samples.square().sum(dim=1) + _log_normal(noise) - logabsdet).mean()
    c64 = {"_transform._transforms." + k: v for k, v in _gradients(loss, layers).items() if k != "loss"}
    c64["loss"] = loss.detach().reshape(1)
    U.assert_within(got, c32, c64, mode)


def test_two_solves_then_two_backwards():
    flow, cnf = _flow("approximate", seed=86)
    data = U.make_data(65, 2, seed=87, device=DEV)
    U.keep_noise(cnf.odefunc, data.e)
    x = data.y / 1.5
    expected, _ = _counted(flow, lambda: -flow.log_prob(x).mean(), solve="force")
    with options.override(cnf_solve_training="force"), ops.KernelTimer(U.NEW_ENTRIES[0]) as forward, \
            ops.KernelTimer(U.NEW_ENTRIES[1]) as backward:
        first = -flow.log_prob(x).mean()
        second = -flow.log_prob(x).mean()
        grads_first = torch.autograd.grad(first, list(flow.parameters()))
        grads_second = torch.autograd.grad(second, list(flow.parameters()))
    assert (len(forward.pairs), len(backward.pairs)) == (2, 2)
    for a, b, (name, _) in zip(grads_first, grads_second, flow.named_parameters()):
        assert torch.equal(a, b) and torch.equal(a, expected[name]), name


def test_eval_mode_with_a_gradient_is_exact_and_uses_the_test_solver():
    cnf = build(3, (17, 33), act="softplus", method="dopri5", seed=88).eval()
    cnf.test_solver = "midpoint"
    data = U.make_data(65, 3, seed=89, device=DEV)
    got, c32, c64, evals = three_ways(cnf, data, torch.flip(data.c2, [0]), None)
    assert evals == 4 and cnf.odefunc._e is None        # two midpoint steps; no noise is drawn or used
    U.assert_within(got, c32, c64, "eval")


def test_training_mode_without_a_gradient_is_the_forward_launch_alone():
    cnf = build(3, (17, 33), seed=90)
    data = U.make_data(65, 3, seed=91, device=DEV)
    logp = torch.flip(data.c2, [0])
    got, *_ = U.evaluate(cnf, data.y, logp, data.c1, data.c2, route="force", e=data.e)
    for p in cnf.parameters():
        p.requires_grad_(False)
    with options.override(cnf_solve_training="force"), ops.KernelTimer(U.NEW_ENTRIES[0]) as forward, \
            ops.KernelTimer(U.NEW_ENTRIES[1]) as backward:
        with torch.no_grad():
            z_t, logp_t = cnf(data.y, logp)
        frozen = cnf(data.y, logp)      # grad mode on, nothing requires one
    assert (len(forward.pairs), len(backward.pairs)) == (2, 0)
    assert not z_t.requires_grad and torch.equal(z_t, got["z_t"]) and torch.equal(logp_t, got["logp_t"])
    assert not frozen[0].requires_grad and torch.equal(frozen[0], z_t) and cnf.get_regularization_states() == ()


def test_noise_is_drawn_where_the_composition_draws_it():
    drawn = {}
    for mode in MODES:      # brute_force draws it too and does not use it
        cnf = build(3, (8, 8), mode=mode, seed=92)
        data = U.make_data(9, 3, seed=93, device=DEV)
        for route in ("force", False):
            torch.manual_seed(94)
            _, forward, backward, _ = U.evaluate(cnf, data.y, data.c2, data.c1, data.c2, route=route)
            assert (forward, backward) == ((1, 1) if route else (0, 0))
            drawn[route] = (cnf.odefunc._e.clone(), torch.randn(3, device=DEV))
        assert torch.equal(drawn["force"][0], drawn[False][0]) and torch.equal(drawn["force"][1], drawn[False][1])


# ---- what keeps the route it had --------------------------------------------------------------------------------------

def _declining(what):
    """``(cnf, z, keyword arguments of evaluate, option value)`` of a call the new route has to decline."""
    kw, route, d, n, hidden, layer_type = {}, "force", 3, 9, (8, 8), "concatsquash"
    extra, solver = {}, "rk4"
    if what == "dopri5":
        solver = "dopri5"
    elif what == "train_T":
        extra = dict(train_T=True)
    elif what == "regularised":
        extra = dict(regularization_fns=[l2_regularzation_fn])
    elif what == "hyper":
        layer_type = "hyper"
    elif what == "four_hidden_layers":
        hidden = (8, 8, 8, 8)
    elif what == "beyond_the_lane_limit":
        route, n = True, ops.CNF_TRAIN_MAX_LANES // 2 + 1
    func = U.make_train_func(d, hidden, layer_type=layer_type, seed=95)
    cnf = CNF(func, solver=solver, **extra).train()
    cnf.solver_options = {"step_size": 0.5} if solver != "dopri5" else {}
    cnf = cnf.to(DEV)
    data = U.make_data(n, d, seed=96, device=DEV)
    z = data.y
    if what == "three_times":
        kw["times"] = torch.tensor([0.0, 0.5, 1.0])
    elif what == "float64_input":
        cnf, kw["dtype"] = cnf.double(), torch.float64
    elif what == "non_contiguous_input":
        z = U.make_data(d, n, seed=96, device=DEV).y.t()
        assert not z.is_contiguous()
    return cnf, data._replace(y=z), kw, (False if what == "default" else route)


@pytest.mark.parametrize("what", ["default", "dopri5", "three_times", "train_T", "regularised", "hyper",
                                  "four_hidden_layers", "float64_input", "non_contiguous_input",
                                  "beyond_the_lane_limit"])
def test_solves_that_decline(what):
    cnf, data, kw, route = _declining(what)
    if what == "default":
        assert options.get("cnf_solve_training") is False
    if what == "beyond_the_lane_limit":
        assert not ops.cnf_solve_train_rows_pay(data.y.shape[0], 3, True)
        assert ops.cnf_solve_train_rows_pay(data.y.shape[0] - 1, 3, True)
    if what == "non_contiguous_input":      # evaluate() clones its input into a contiguous one: call the CNF itself
        results = []
        for value in (route, False):
            U.keep_noise(cnf.odefunc, data.e)
            z = data.y.detach().requires_grad_(True)
            with options.override(cnf_solve_training=value), ops.KernelTimer(U.NEW_ENTRIES[0]) as forward, \
                    ops.KernelTimer(U.NEW_ENTRIES[1]) as backward:
                z_t, logp_t = cnf(z, data.c2)
                grads = torch.autograd.grad((data.c1 * z_t).sum() + logp_t.sum(), [z] + list(cnf.parameters()))
            assert (len(forward.pairs), len(backward.pairs)) == (0, 0)
            results.append([z_t.detach(), logp_t.detach()] + list(grads))
        for a, b in zip(*results):
            assert torch.equal(a, b)
        return
    if what == "three_times":       # the states at all three times come back: weigh the last
        c1, c2 = data.c1.expand(3, -1, -1) * torch.tensor([0.0, 0.0, 1.0], device=DEV).view(3, 1, 1), \
            data.c2.expand(3, -1, -1) * torch.tensor([0.0, 0.0, 1.0], device=DEV).view(3, 1, 1)
    else:
        c1, c2 = data.c1, data.c2
    tried, *launches = U.evaluate(cnf, data.y, data.c2, c1, c2, route=route, e=data.e, **kw)
    plain, *none = U.evaluate(cnf, data.y, data.c2, c1, c2, route=False, e=data.e, **kw)
    assert launches == [0, 0, 0] and none == [0, 0, 0] and set(tried) == set(plain)
    for key in plain:
        assert torch.equal(tried[key], plain[key]), key


def test_the_lane_limit_is_taken_under_true():
    cnf = build(3, (8, 8), seed=97)
    n = ops.CNF_TRAIN_MAX_LANES // 2
    data = U.make_data(n, 3, seed=98, device=DEV)
    _, forward, backward, field = U.evaluate(cnf, data.y, data.c2, data.c1, data.c2, route=True, e=data.e)
    assert (forward, backward, field) == (1, 1, 0)


def test_per_evaluation_nodes_are_unchanged_with_the_option_off():
    flow, cnf = _flow("approximate", seed=61)
    data = U.make_data(65, 2, seed=62, device=DEV)
    U.keep_noise(cnf.odefunc, data.e)
    x = data.y / 1.5
    with ops.KernelTimer("fc_cnf_field_backward") as nodes:
        _, launches = _counted(flow, lambda: -flow.log_prob(x).mean(), solve=False, field="force")
    assert launches == [0, 0, 16] and len(nodes.pairs) == 16 and cnf.num_evals() == 16


def test_double_backward_raises():
    cnf = build(3, (8, 8), seed=99)
    data = U.make_data(9, 3, seed=100, device=DEV)
    U.keep_noise(cnf.odefunc, data.e)
    z = data.y.clone().requires_grad_(True)
    with options.override(cnf_solve_training="force"):
        z_t, logp_t = cnf(z, data.c2)
        with pytest.raises(RuntimeError, match="cnf_solve_training=False"):
            torch.autograd.grad(z_t.sum() + logp_t.sum(), z, create_graph=True)
