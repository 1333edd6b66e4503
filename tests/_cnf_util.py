"""Shared by tests/test_cnf_host.py and tests/test_gpu_cnf.py: the fixtures, the builders and the float64 truth.

* The FIELD truth is this package's torch composition on ``.double()`` parameters; tests/test_cnf_host.py pins that
  composition to the reference through the fixtures of tests/golden/make_cnf_golden.py.
* The INTEGRATOR truth is independent of the package's solver: ``rk_solve`` below, a few-line fixed-step explicit
  Runge-Kutta loop in float64 over that field.
"""
import copy
import os

import numpy as np
import torch

from flowconductor_amd.CNF import CNF
from flowconductor_amd.CNF.neural_odes import ODEfunc, ODEnet
from make_cnf_golden import CASES

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASE_NAMES = [case[0] for case in CASES]
KERNEL_CASES = [case[0] for case in CASES if case[3] not in ("hyper", "blend")]

TABLEAUS = {    # nodes, strictly lower-triangular coefficients, weights
    "euler": ([0.0], [[]], [1.0]),
    "midpoint": ([0.0, 0.5], [[], [0.5]], [0.0, 1.0]),
    "rk4": ([0.0, 0.5, 0.5, 1.0], [[], [0.5], [0.0, 0.5], [0.0, 0.0, 1.0]], [1 / 6, 1 / 3, 1 / 3, 1 / 6]),
}


def fixture(name):
    return np.load(os.path.join(GOLDEN, "cnf_%s.npz" % name))


def build_case(name):
    """The package's ``ODEfunc`` of a fixture case (fresh parameters; ``load_case`` fills them)."""
    _, d, hidden, layer_type, nonlinearity, net_kw, func_kw = next(case for case in CASES if case[0] == name)
    net = ODEnet(hidden, (d,), None, False, layer_type=layer_type, nonlinearity=nonlinearity, **net_kw)
    return ODEfunc(net, divergence_fn="approximate", **func_kw)


def state_dict_of(g, prefix="sd::"):
    return {k[len(prefix):]: torch.from_numpy(np.asarray(g[k])) for k in g.files if k.startswith(prefix)}


def load_case(name):
    g = fixture(name)
    func = build_case(name)
    func.load_state_dict(state_dict_of(g), strict=True)
    return func.eval(), g


def make_func(d, hidden, layer_type="concatsquash", nonlinearity="tanh", seed=0, gain=1.0, residual=False,
              scale_output=1, act_norm=False):
    """A seeded ``ODEfunc`` in eval mode with every parameter multiplied by ``gain``."""
    torch.manual_seed(seed)
    net = ODEnet(tuple(hidden), (d,), None, False, layer_type=layer_type, nonlinearity=nonlinearity,
                 scale_output=scale_output, act_norm=act_norm)
    with torch.no_grad():
        for p in net.parameters():
            p.mul_(gain)
    return ODEfunc(net, residual=residual).eval()


def field64(func, t, y):
    """``(dy, negdiv [N])`` of the float64 composition of ``func`` (any device) at float64 copies of the inputs."""
    f64 = copy.deepcopy(func).double().eval()
    with torch.no_grad():
        dy, negdiv = f64(torch.as_tensor(float(t), dtype=torch.float64, device=y.device), (y.double(), None))[:2]
    return dy, negdiv.reshape(-1)


def rk_solve(func, z, t0, t1, steps, method):
    """``(z(t1), delta logp [N])`` in float64 by ``steps`` equal steps of ``method``: the independent truth."""
    f64 = copy.deepcopy(func).double().cpu().eval()
    nodes, rows, weights = TABLEAUS[method]
    y = z.detach().double().cpu()
    logp = torch.zeros(y.shape[0], dtype=torch.float64)
    h = (t1 - t0) / steps
    with torch.no_grad():
        for i in range(steps):
            t = t0 + i * h
            ks, ls = [], []
            for c, row in zip(nodes, rows):
                yi = y + h * sum((a * k for a, k in zip(row, ks) if a != 0.0), torch.zeros_like(y))
                k, l = f64(torch.tensor(t + c * h, dtype=torch.float64), (yi, None))[:2]
                ks.append(k)
                ls.append(l.reshape(-1))
            y = y + h * sum(b * k for b, k in zip(weights, ks))
            logp = logp + h * sum(b * l for b, l in zip(weights, ls))
    return y, logp


def make_cnf(func, T=1.0, solver="rk4", steps=8, tol=1e-5):
    flow = CNF(func, T=T, solver=solver, atol=tol, rtol=tol).eval()
    if solver != "dopri5":
        flow.solver_options = {"step_size": T / steps}
    return flow


def worst(a, b):
    return float((a.detach().double().cpu() - b.detach().double().cpu()).abs().max())


def scale_of(t):
    return max(1.0, float(t.detach().abs().max()))
