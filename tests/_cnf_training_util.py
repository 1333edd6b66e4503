"""Shared by tests/test_cnf_training_host.py and tests/test_gpu_cnf_training.py: the training-mode fixtures of
tests/golden/make_cnf_training_golden.py, seeded builders, and one evaluation of an ``ODEfunc`` with its first-order
gradients on a chosen route.

The truth of every comparison is the package's torch composition on ``.double()`` parameters (``cnf_training=False``);
tests/test_cnf_training_host.py pins that composition's training-mode gradients to the reference through the fixtures.
"""
import collections
import copy
import os

import numpy as np
import torch

from flowconductor_amd import ops, options
from flowconductor_amd.CNF.neural_odes import ODEfunc, ODEnet
from make_cnf_golden import CASES
from make_cnf_training_golden import MODES, TRAIN_CASES

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = [(name, mode) for name in TRAIN_CASES for mode in MODES]

Data = collections.namedtuple("Data", "t y e c1 c2")


def load_train_case(name, mode):
    """The package's ``ODEfunc`` of a fixture in training mode, and the fixture."""
    g = np.load(os.path.join(GOLDEN, "cnf_train_%s_%s.npz" % (name, mode)))
    _, d, hidden, layer_type, nonlinearity, net_kw, func_kw = next(case for case in CASES if case[0] == name)
    net = ODEnet(hidden, (d,), None, False, layer_type=layer_type, nonlinearity=nonlinearity, **net_kw)
    func = ODEfunc(net, divergence_fn=mode, **func_kw)
    func.load_state_dict({k[4:]: torch.from_numpy(np.asarray(g[k])) for k in g.files if k.startswith("sd::")},
                         strict=True)
    return func.train(), g


def fixture_data(g, device="cpu"):
    return Data(*(torch.from_numpy(np.asarray(g[k])).to(device) for k in ("t", "y", "e", "c1", "c2")))


def make_train_func(d, hidden, layer_type="concatsquash", nonlinearity="tanh", mode="approximate", seed=0, gain=1.5,
                    residual=False, scale_output=1, act_norm=False):
    """A seeded ``ODEfunc`` in training mode with every parameter multiplied by ``gain``."""
    torch.manual_seed(seed)
    net = ODEnet(tuple(hidden), (d,), None, False, layer_type=layer_type, nonlinearity=nonlinearity,
                 scale_output=scale_output, act_norm=act_norm)
    with torch.no_grad():
        for p in net.parameters():
            p.mul_(gain)
    return ODEfunc(net, divergence_fn=mode, residual=residual).train()


def make_data(n, d, seed, device="cpu", t=0.37):
    gen = torch.Generator().manual_seed(seed)
    y = 1.5 * torch.randn(n, d, generator=gen)
    e, c1, c2 = torch.randn(n, d, generator=gen), torch.randn(n, d, generator=gen), torch.randn(n, 1, generator=gen)
    return Data(t, y.to(device), e.to(device), c1.to(device), c2.to(device))


def evaluate(func, data, route=False, dtype=torch.float32, preset=True):
    """``({"dy", "negdiv", "g::y", "g::<parameter>"...}, launches of fc_cnf_field_train, of fc_cnf_field_backward)`` of
    one evaluation of ``func`` (float64: of a ``.double()`` copy) with option ``cnf_training=route`` and the gradients
    of ``sum(c1 * dy) + sum(c2 * negdiv)``."""
    f = func if dtype == torch.float32 else copy.deepcopy(func).to(dtype)
    f.before_odeint(e=data.e.to(dtype) if preset else None)
    y = data.y.to(dtype).clone().requires_grad_(True)
    t = data.t.to(dtype) if isinstance(data.t, torch.Tensor) else data.t
    with options.override(cnf_training=route), ops.KernelTimer("fc_cnf_field_train") as forward, \
            ops.KernelTimer("fc_cnf_field_backward") as backward:
        dy, negdiv = f(t, (y, None))[:2]
        loss = (data.c1.to(dtype) * dy).sum() + (data.c2.to(dtype) * negdiv).sum()
        names = [k for k, _ in f.named_parameters()]
        grads = torch.autograd.grad(loss, [y] + [p for _, p in f.named_parameters()])
    out = {"dy": dy.detach(), "negdiv": negdiv.detach(), "g::y": grads[0]}
    out.update({"g::" + k: g for k, g in zip(names, grads[1:])})
    return out, len(forward.pairs), len(backward.pairs)


def worst(a, b):
    return float((a.detach().double().cpu() - b.detach().double().cpu()).abs().max())


def scale_of(t):
    return max(1.0, float(t.detach().abs().max()))


def assert_within(got, c32, c64, what):
    """The project's rule for every entry: ``1e-5 max(1, max|c64|) + 4 max|c32 - c64|``."""
    assert set(got) == set(c64)
    for key in c64:
        assert got[key].shape == c64[key].shape, (what, key)
        bound = 1e-5 * scale_of(c64[key]) + 4 * worst(c32[key], c64[key])
        assert worst(got[key], c64[key]) <= bound, (what, key, worst(got[key], c64[key]), bound)


def hidden_preactivations(func, data):
    """Every hidden layer's pre-activation in the float64 composition, concatenated."""
    f = copy.deepcopy(func).double()
    seen = []
    hooks = [layer.register_forward_hook(lambda m, i, o: seen.append(o.detach().reshape(-1)))
             for layer in list(f.diffeq.layers)[:-1]]
    with torch.no_grad():
        f.diffeq(torch.as_tensor(data.t, dtype=torch.float64, device=data.y.device), data.y.double())
    for hook in hooks:
        hook.remove()
    return torch.cat(seen) if seen else torch.zeros(0, dtype=torch.float64)
