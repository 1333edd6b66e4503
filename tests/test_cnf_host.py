"""Continuous normalizing flows off the GPU: the torch composition of ``flowconductor_amd.CNF`` and its own solver.

Bounds (none of them comes from what the code gives):

* fixtures (tests/golden/cnf_*.npz, recorded from the reference's ``ODEnet`` / ``ODEfunc``): checkpoints load with
  ``strict=True``; net, field and divergence within ``1e-5 max(1, max|expected|) + 4 floor`` of the recorded float32
  values, ``floor = max|ref32 - ref64|`` as recorded (the rule of tests/test_gpu_golden.py); the ``.double()`` copy
  within 1e-12 of the recorded float64 values;
* the affine ODE ``dz/dt = W z + b`` (``hidden_dims=()``, ``layer_type="ignore"``): ``z(T)`` from
  ``scipy.linalg.expm``, ``delta logp = -T tr(W)`` exactly for every solver (the integrand is constant: rounding only,
  1e-12 in float64); halving the step divides the error by 2 ** order within +-0.35 in the exponent; ``dopri5`` at
  ``atol = rtol = 1e-9`` within 1e-7;
* gradients through ``rk4`` against central differences in float64 (step 1e-6, so truncation ~1e-12 relative and
  rounding ~1e-10): 1e-7 relative;
* Hutchinson's estimator: the mean of 4096 seeded Rademacher draws within 3 standard errors of the exact divergence.
"""
import copy
import math

import numpy as np
import pytest
import scipy.linalg
import torch

from flowconductor_amd import transforms
from flowconductor_amd.CNF import CNF, CNFTransform
from flowconductor_amd.CNF.neural_odes import ODEfunc, ODEnet, diffeq_layers
from flowconductor_amd.CNF.neural_odes import odefunc as odefunc_module
from flowconductor_amd.CNF.neural_odes import util
from flowconductor_amd.CNF.neural_odes.wrappers import cnf_regularization as reg
from flowconductor_amd.CNF.odeint import odeint

from _cnf_util import (CASE_NAMES, build_case, fixture, load_case, make_cnf, make_func, rk_solve, scale_of,
                       state_dict_of, worst)

ORDERS = {"euler": 1, "midpoint": 2, "rk4": 4}


# ---- fixtures ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", CASE_NAMES)
def test_fixture_checkpoint_field_and_divergence(name):
    func, g = load_case(name)
    t, y, logp = (torch.from_numpy(g[k]) for k in ("t", "y", "logp"))
    func.before_odeint()        # the recorded ``_num_evals`` is the reference's count when it was saved
    with torch.no_grad():
        net = func.diffeq(t, y)
        dy, negdiv = func(t, (y, logp))
    assert negdiv.shape == (y.shape[0], 1) and func.num_evals() == 1.0
    for tag, got in (("net", net), ("dy", dy), ("negdiv", negdiv)):
        expected = torch.from_numpy(g[tag + "32"])
        bound = 1e-5 * scale_of(expected) + 4 * float(g["floor_" + tag])
        assert worst(got, expected) <= bound, (name, tag, worst(got, expected), bound)
    func64 = copy.deepcopy(func).double()
    with torch.no_grad():
        net = func64.diffeq(t.double(), y.double())
        dy, negdiv = func64(t.double(), (y.double(), logp.double()))
    for tag, got in (("net", net), ("dy", dy), ("negdiv", negdiv)):
        assert worst(got, torch.from_numpy(g[tag + "64"])) <= 1e-12, (name, tag)


def test_reference_cnf_checkpoint_loads_strict():
    g = fixture(CASE_NAMES[0])
    flow = CNF(build_case(CASE_NAMES[0]), T=2.0, train_T=True)
    flow.load_state_dict(state_dict_of(g, "cnf_sd::"), strict=True)
    assert isinstance(flow.sqrt_end_time, torch.nn.Parameter)
    assert abs(float(flow.sqrt_end_time.detach()) ** 2 - 0.5) < 1e-6
    assert "sqrt_end_time" in dict(CNF(build_case(CASE_NAMES[0])).named_buffers())


# ---- the affine known answer -----------------------------------------------------------------------------------------

def _affine(d=3, seed=5):
    func = make_func(d, (), layer_type="ignore", seed=seed).double()
    layer = func.diffeq.layers[0]._layer
    w, b = layer.weight.detach().numpy(), layer.bias.detach().numpy()
    return func, w, b


def _affine_answer(w, b, z, T):
    d = w.shape[0]
    m = np.zeros((d + 1, d + 1))
    m[:d, :d], m[:d, d] = w, b
    e = scipy.linalg.expm(T * m)
    return z.numpy() @ e[:d, :d].T + e[:d, d], -T * np.trace(w)


@pytest.mark.parametrize("method", sorted(ORDERS))
def test_affine_ode_orders_and_exact_logp(method):
    func, w, b = _affine()
    z = torch.randn(11, 3, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    T = 1.0
    z_true, dlogp = _affine_answer(w, b, z, T)
    errors = []
    for steps in (16, 32):
        flow = make_cnf(func, T=T, solver=method, steps=steps).double()
        with torch.no_grad():
            z_t, logp_t = flow(z, torch.zeros(11, 1, dtype=torch.float64))
        assert flow.num_evals() == steps * {"euler": 1, "midpoint": 2, "rk4": 4}[method]
        assert float((logp_t - dlogp).abs().max()) <= 1e-12
        errors.append(float(np.abs(z_t.numpy() - z_true).max()))
    observed = math.log2(errors[0] / errors[1])
    assert abs(observed - ORDERS[method]) <= 0.35, (method, errors, observed)


def test_affine_ode_dopri5():
    func, w, b = _affine()
    z = torch.randn(11, 3, dtype=torch.float64, generator=torch.Generator().manual_seed(2))
    flow = make_cnf(func, T=1.0, solver="dopri5", tol=1e-9).double()
    with torch.no_grad():
        z_t, logp_t = flow(z, torch.zeros(11, 1, dtype=torch.float64))
    z_true, dlogp = _affine_answer(w, b, z, 1.0)
    assert float(np.abs(z_t.numpy() - z_true).max()) <= 1e-7
    assert float((logp_t - dlogp).abs().max()) <= 1e-7
    assert flow.num_evals() >= 8 and (flow.num_evals() - 2) % 6 == 0     # initial-step probe + 6 per attempt + f0


def test_dopri5_matches_independent_rk4_and_step_cap():
    func = make_func(2, (16, 16), seed=3, gain=2.0).double()
    z = torch.randn(9, 2, dtype=torch.float64, generator=torch.Generator().manual_seed(3))
    z_true, logp_true = rk_solve(func, z, 0.0, 1.0, 512, "rk4")
    flow = make_cnf(func, solver="dopri5", tol=1e-9).double()
    with torch.no_grad():
        z_t, logp_t = flow(z, torch.zeros(9, 1, dtype=torch.float64))
    assert worst(z_t, z_true) <= 1e-7 and worst(logp_t.reshape(-1), logp_true) <= 1e-7
    with pytest.raises(RuntimeError, match="max_num_steps"):
        odeint(flow.odefunc, (z, torch.zeros(9, 1, dtype=torch.float64)), [0.0, 1.0], atol=1e-9, rtol=1e-9,
               options={"max_num_steps": 2})


def test_odeint_returns_every_time_and_takes_a_single_tensor():
    out = odeint(lambda t, y: -y, torch.ones(3, dtype=torch.float64), torch.tensor([0.0, 0.5, 1.0]), atol=1e-10,
                 rtol=1e-10, adjoint_options={"norm": "seminorm"})
    assert out.shape == (3, 3)
    assert float((out[:, 0] - torch.exp(-torch.tensor([0.0, 0.5, 1.0], dtype=torch.float64))).abs().max()) <= 1e-8
    with pytest.raises(ValueError):
        odeint(lambda t, y: -y, torch.ones(3), [0.0, 1.0], method="adams")


# ---- behaviour -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("solver", ["rk4", "dopri5"])
def test_reverse_returns_the_input(solver):
    func = make_func(2, (16, 16), seed=4, gain=1.5).double()
    flow = make_cnf(func, solver=solver, steps=64, tol=1e-10).double()
    z = torch.randn(6, 2, dtype=torch.float64, generator=torch.Generator().manual_seed(4))
    with torch.no_grad():
        z_t, logp_t = flow(z, torch.zeros(6, 1, dtype=torch.float64))
        back, logp_back = flow(z_t, logp_t, reverse=True)
        only_z = flow(z)
    assert worst(back, z) <= 1e-7 and float(logp_back.abs().max()) <= 1e-7
    assert float(logp_t.abs().max()) > 1e-4 and torch.equal(only_z, z_t)


def test_integration_times_with_three_entries_and_training_state():
    func = make_func(2, (8,), seed=6).double()
    flow = make_cnf(func, solver="rk4", steps=4).double()
    z = torch.randn(5, 2, dtype=torch.float64, generator=torch.Generator().manual_seed(6))
    with torch.no_grad():
        z_all, logp_all = flow(z, torch.zeros(5, 1, dtype=torch.float64),
                               integration_times=torch.tensor([0.0, 0.5, 1.0]))
        z_end = flow(z)
    assert z_all.shape == (3, 5, 2) and logp_all.shape == (3, 5, 1)
    assert torch.equal(z_all[0], z) and worst(z_all[2], z_end) <= 1e-12


def test_cnf_transform_is_consistent_with_inverse_transform():
    func = make_func(3, (12,), seed=7, gain=1.5).double()
    t = CNFTransform(make_cnf(func, solver="rk4", steps=32).double())
    x = torch.randn(8, 3, dtype=torch.float64, generator=torch.Generator().manual_seed(7))
    with torch.no_grad():
        y, lad = t(x)
        x_back, lad_back = t.inverse(y)
        y_inv, lad_inv = transforms.InverseTransform(t).inverse(x)
        stacked, lad_two = transforms.CompositeTransform([t, transforms.InverseTransform(t)])(x)
    assert lad.shape == (8,) and worst(x_back, x) <= 1e-6 and worst(lad_back, -lad) <= 1e-6
    assert torch.equal(y_inv, y) and torch.equal(lad_inv, lad)
    assert worst(stacked, x) <= 1e-6 and float(lad_two.abs().max()) <= 1e-6
    with pytest.raises(ValueError):
        t(x, context=x)


def _negative_log_likelihood(flow, x):
    z, delta = flow(x, torch.zeros(x.shape[0], 1, dtype=x.dtype))
    log_prob = -0.5 * z.square().sum(dim=1) - 0.5 * x.shape[1] * math.log(2 * math.pi) - delta.reshape(-1)
    return -log_prob.mean()


def test_gradients_through_rk4_match_finite_differences():
    func = make_func(2, (8, 8), seed=8, gain=1.5).double()
    flow = make_cnf(func, solver="rk4", steps=8).double()       # eval mode: the exact divergence, differentiable
    x = torch.randn(6, 2, dtype=torch.float64, generator=torch.Generator().manual_seed(8))
    weight = flow.odefunc.diffeq.layers[1]._layer.weight
    gate = flow.odefunc.diffeq.layers[0]._hyper_gate.bias
    loss = _negative_log_likelihood(flow, x)
    grads = torch.autograd.grad(loss, [weight, gate])
    for param, grad, index in ((weight, grads[0], (2, 3)), (gate, grads[1], (1,))):
        step = 1e-6
        values = []
        for sign in (1.0, -1.0):
            with torch.no_grad():
                param[index] += sign * step
                values.append(float(_negative_log_likelihood(flow, x)))
                param[index] -= sign * step
        numeric = (values[0] - values[1]) / (2 * step)
        assert abs(float(grad[index]) - numeric) <= 1e-7 * max(1.0, abs(numeric)), (index, float(grad[index]), numeric)
        assert abs(numeric) > 1e-6


def test_training_mode_uses_hutchinson_with_a_fixed_noise_vector():
    torch.manual_seed(11)
    net = ODEnet((16,), (3,), None, False, layer_type="concat", nonlinearity="tanh")
    with torch.no_grad():
        for p in net.parameters():
            p.mul_(2.0)
    func = ODEfunc(net, divergence_fn="approximate", rademacher=True).double()
    point = torch.randn(1, 3, dtype=torch.float64)
    y = point.repeat(4096, 1)
    t = torch.tensor(0.3, dtype=torch.float64)
    func.eval()
    exact = float(-func(t, (point, None))[1])
    func.train()
    func.before_odeint()
    first = func(t, (y, None))[1].detach()
    again = func(t, (y, None))[1].detach()
    assert torch.equal(first, again) and func.num_evals() == 2.0      # one e per solve
    assert set(func._e.unique().tolist()) == {-1.0, 1.0} and func._e.device == y.device
    func.before_odeint()
    assert func._e is None and func.num_evals() == 0.0
    estimates = -first.reshape(-1)
    standard_error = float(estimates.std()) / math.sqrt(4096)
    assert standard_error > 0 and abs(float(estimates.mean()) - exact) <= 3 * standard_error
    gaussian = util.sample_gaussian_like(y)
    assert gaussian.shape == y.shape and gaussian.dtype == y.dtype
    # brute force in training mode is exact and differentiable
    brute = ODEfunc(net, divergence_fn="brute_force").double().train()
    assert abs(float(-brute(t, (point, None))[1]) - exact) <= 1e-12


def test_regularizers_return_one_scalar_each():
    fns = [reg.l1_regularzation_fn, reg.l2_regularzation_fn, reg.directional_l2_regularization_fn,
           reg.jacobian_frobenius_regularization_fn, reg.jacobian_diag_frobenius_regularization_fn,
           reg.jacobian_offdiag_frobenius_regularization_fn]
    func = make_func(2, (8,), seed=9, gain=2.0)
    flow = CNF(func, T=1.0, regularization_fns=fns, solver="rk4")
    flow.solver_options = {"step_size": 0.25}
    assert isinstance(flow.odefunc, reg.RegularizedODEfunc) and flow.nreg == 6
    flow.train()
    x = torch.randn(5, 2, generator=torch.Generator().manual_seed(9))
    z, logp = flow(x, torch.zeros(5, 1))
    states = flow.get_regularization_states()
    assert len(states) == 6 and flow.get_regularization_states() is None
    assert all(s.dim() == 0 and torch.isfinite(s) and float(s) > 0 for s in states)
    (logp.mean() + sum(states)).backward()
    assert all(p.grad is not None for p in func.diffeq.parameters())
    assert flow.num_evals() == 16.0
    flow.eval()
    with torch.no_grad():
        flow(x, torch.zeros(5, 1))
    assert flow.get_regularization_states() == ()


def test_conv_and_the_parts_that_are_not_built_raise():
    with pytest.raises(NotImplementedError, match="conv=False"):
        ODEnet((8,), (3, 8, 8), (1, 1), True)
    with pytest.raises(NotImplementedError):
        ODEnet((8,), (2,), None, False, num_squeeze=1)
    assert set(odefunc_module.NONLINEARITIES) == {"tanh", "relu", "softplus", "elu", "swish", "square", "identity"}
    for name in ("IgnoreLinear", "ConcatLinear", "ConcatLinear_v2", "SquashLinear", "ConcatSquashLinear", "HyperLinear",
                 "BlendLinear", "SequentialDiffEq", "diffeq_wrapper", "reshape_wrapper"):
        assert hasattr(diffeq_layers, name), name


def test_sequential_diffeq_and_wrappers():
    torch.manual_seed(0)
    chain = diffeq_layers.SequentialDiffEq(diffeq_layers.ConcatLinear(3, 5), torch.nn.Tanh(),
                                           diffeq_layers.IgnoreLinear(5, 3))
    t, x = torch.tensor(0.4), torch.randn(4, 3)
    first, last = chain.layers[0].module, chain.layers[2].module
    assert torch.allclose(chain(t, x), last(t, torch.tanh(first(t, x))))
    shaped = diffeq_layers.reshape_wrapper((3, 1), diffeq_layers.diffeq_wrapper(torch.nn.Flatten()))
    assert shaped(t, x).shape == (4, 3)


def test_deepcopy_and_state_dict_round_trip():
    func = make_func(2, (8, 8), seed=10, residual=True, scale_output=0.5)
    flow = make_cnf(func, solver="rk4", steps=4)
    x = torch.randn(5, 2, generator=torch.Generator().manual_seed(10))
    with torch.no_grad():
        expected = flow(x, torch.zeros(5, 1))
        clone = copy.deepcopy(flow)
        got = clone(x, torch.zeros(5, 1))
        fresh = make_cnf(make_func(2, (8, 8), seed=99, residual=True, scale_output=0.5), solver="rk4", steps=4)
        fresh.load_state_dict(flow.state_dict(), strict=True)
        loaded = fresh(x, torch.zeros(5, 1))
    for a, b in zip(expected, got):
        assert torch.equal(a, b)
    for a, b in zip(expected, loaded):
        assert torch.equal(a, b)
    assert clone.odefunc.diffeq.layers[0]._layer.weight is not flow.odefunc.diffeq.layers[0]._layer.weight


def test_a_trained_end_time_gets_the_slope_at_the_end():
    """``dz(T)/dT = f(T, z(T))``: the end time enters the last step of the solve as a tensor.  ``dopri5`` at 1e-9
    differentiates a fifth-order step with respect to its length, so the two agree far below 1e-6."""
    func = make_func(2, (8,), seed=12, gain=2.0).double()
    flow = CNF(func, T=1.0, train_T=True, solver="dopri5", atol=1e-9, rtol=1e-9).double().eval()
    x = torch.randn(4, 2, dtype=torch.float64, generator=torch.Generator().manual_seed(12))
    z, _ = flow(x, torch.zeros(4, 1, dtype=torch.float64))
    grad, = torch.autograd.grad(z.sum(), flow.sqrt_end_time)
    with torch.no_grad():
        slope = func(torch.tensor(1.0, dtype=torch.float64), (z.detach(), None))[0]
    expected = 2.0 * float(flow.sqrt_end_time.detach()) * float(slope.sum())
    assert abs(float(grad) - expected) <= 1e-6 * max(1.0, abs(expected)) and abs(expected) > 1e-3
