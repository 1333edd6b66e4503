"""Generate tests/golden/cnf_train_<case>_<mode>.npz (training-mode continuous normalizing flows) from the REFERENCE's own
classes.

Runs only where the reference tree exists:
    python tests/golden/make_cnf_training_golden.py
It imports the reference as make_cnf_golden.py does (the placeholder ``torchdiffeq`` module included): the fixtures pin
the ODE FUNCTION in training mode -- the net, ``divergence_fn`` with a preset noise ``before_odeint(e=e)``, ``residual``,
``scale_output`` -- and its first-order gradients, not a solver.

Files: ``cnf_train_<case>_<mode>.npz`` for ``TRAIN_CASES`` (five of make_cnf_golden's ``CASES``) and ``MODES``
(``approximate``: Hutchinson's estimator, ``brute_force``: the exact divergence).  Each holds ``sd::*`` (the ``state_dict``
of the reference's ``ODEfunc``), ``t``, ``y`` [7, D], ``e`` [7, D], the cotangents ``c1`` [7, D] and ``c2`` [7, 1], and
from the reference in float32 and from a ``.double()`` deep copy (suffix 32 / 64): ``dy``, ``negdiv`` and the gradients of
``sum(c1 * dy) + sum(c2 * negdiv)`` with respect to ``y`` (``g::y``) and every parameter (``g::<state_dict key>``), with
the float32 floors ``floor::<name> = max|32 - 64|``.
"""
import copy
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_cnf_golden  # noqa: E402

ROWS = make_cnf_golden.ROWS
SIZE_LIMIT = make_cnf_golden.SIZE_LIMIT
TRAIN_CASES = [
    "toy_d2_h64x64x64_concatsquash_tanh",
    "d3_h17x33_concat_softplus",
    "d3_h16x16_concatsquash_swish",
    "d4_h32_concat_tanh_residual",
    "d4_h32_concat_tanh_scale2p5",
]
MODES = ["approximate", "brute_force"]


def evaluate(func, t, y, e, c1, c2):
    """``dy``, ``negdiv`` and the gradients of the fixed linear functional of them, as ``{name: tensor}``."""
    func.before_odeint(e=e)
    y = y.clone().requires_grad_(True)
    dy, negdiv = func(t.clone(), (y, torch.zeros(y.shape[0], 1, dtype=y.dtype)))[:2]
    loss = (c1 * dy).sum() + (c2 * negdiv).sum()
    names = [k for k, _ in func.named_parameters()]
    grads = torch.autograd.grad(loss, [y] + [p for _, p in func.named_parameters()])
    out = {"dy": dy.detach(), "negdiv": negdiv.detach(), "g::y": grads[0]}
    out.update({"g::" + k: g for k, g in zip(names, grads[1:])})
    return out


def record(odefunc_module, index, name, mode):
    _, d, hidden, layer_type, nonlinearity, net_kw, func_kw = next(c for c in make_cnf_golden.CASES if c[0] == name)
    seed = 5200 + 17 * index + (0 if mode == "approximate" else 7)
    torch.manual_seed(seed)
    net = odefunc_module.ODEnet(hidden, (d,), None, False, layer_type=layer_type, nonlinearity=nonlinearity, **net_kw)
    func = odefunc_module.ODEfunc(net, divergence_fn=mode, **func_kw).train()
    gen = torch.Generator().manual_seed(seed)
    y = 1.5 * torch.randn(ROWS, d, generator=gen)
    e = torch.randn(ROWS, d, generator=gen)
    c1 = torch.randn(ROWS, d, generator=gen)
    c2 = torch.randn(ROWS, 1, generator=gen)
    t = torch.tensor(0.37)
    r32 = evaluate(func, t, y, e, c1, c2)
    r64 = evaluate(copy.deepcopy(func).double(), t.double(), y.double(), e.double(), c1.double(), c2.double())
    assert r32["negdiv"].shape == (ROWS, 1) and r32["dy"].shape == (ROWS, d), name
    out = {"sd::" + k: v.detach().clone().numpy() for k, v in func.state_dict().items()}
    out.update(t=t.numpy(), y=y.numpy(), e=e.numpy(), c1=c1.numpy(), c2=c2.numpy())
    worst = 0.0
    for key in r32:
        assert torch.isfinite(r32[key]).all() and torch.isfinite(r64[key]).all(), (name, key)
        out[key + "32"], out[key + "64"] = r32[key].numpy(), r64[key].numpy()
        out["floor::" + key] = np.float64((r32[key].double() - r64[key]).abs().max().item())
        if key.startswith("g::"):
            worst = max(worst, out["floor::" + key])
    path = os.path.join(HERE, "cnf_train_%s_%s.npz" % (name, mode))
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size <= SIZE_LIMIT, (name, size)
    print("%-36s %-11s floor dy %.1e negdiv %.1e gradients %.1e | max|g| %.2f | %d B"
          % (name, mode, out["floor::dy"], out["floor::negdiv"], worst,
             max(float(v.abs().max()) for k, v in r64.items() if k.startswith("g::")), size))


def main():
    _, odefunc_module = make_cnf_golden.import_reference()
    for index, name in enumerate(TRAIN_CASES):
        for mode in MODES:
            record(odefunc_module, index, name, mode)


if __name__ == "__main__":
    main()
