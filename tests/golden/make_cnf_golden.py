"""Generate tests/golden/cnf_<case>.npz (continuous normalizing flows) from the REFERENCE's own classes.

Runs only where the reference tree exists:
    python tests/golden/make_cnf_golden.py
It follows make_golden.import_reference's recipe, with a placeholder module for ``torchdiffeq`` (not installed) in
``sys.modules``: only the reference's ``CNF/cnf.py`` imports it, at module level, and nothing recorded here calls it --
the fixtures pin the ODE FUNCTION (net, exact eval-mode divergence, ``residual``, ``scale_output``) and the
``state_dict`` keys, not a solver.

Files: ``cnf_<case>.npz`` for ``CASES``.  Each holds ``sd::*`` (the ``state_dict`` of the reference's ``ODEfunc``), for
the first case also ``cnf_sd::*`` (that of a ``CNF`` with ``train_T=True`` around it), ``t``, ``y`` [7, D], ``logp``
[7, 1], the reference's ``net32 = ODEnet(t, y)``, ``dy32`` / ``negdiv32 = ODEfunc(t, (y, logp))`` in eval mode, the same
from a ``.double()`` deep copy (``net64``, ``dy64``, ``negdiv64``) and the float32 floors max|32 - 64| of the three.
"""
import copy
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import make_golden  # noqa: E402

ROWS = 7
SIZE_LIMIT = 900 * 1024
CASES = [
    # name, D, hidden, layer_type, nonlinearity, ODEnet extras, ODEfunc extras
    ("toy_d2_h64x64x64_concatsquash_tanh", 2, (64, 64, 64), "concatsquash", "tanh", {}, {}),
    ("d3_h17x33_ignore_softplus", 3, (17, 33), "ignore", "softplus", {}, {}),
    ("d3_h17x33_concat_softplus", 3, (17, 33), "concat", "softplus", {}, {}),
    ("d3_h17x33_concat_v2_softplus", 3, (17, 33), "concat_v2", "softplus", {}, {}),
    ("d3_h17x33_squash_softplus", 3, (17, 33), "squash", "softplus", {}, {}),
    ("d3_h17x33_hyper_softplus", 3, (17, 33), "hyper", "softplus", {}, {}),
    ("d3_h17x33_blend_softplus", 3, (17, 33), "blend", "softplus", {}, {}),
    ("d3_h16x16_concatsquash_relu", 3, (16, 16), "concatsquash", "relu", {}, {}),
    ("d3_h16x16_concatsquash_elu", 3, (16, 16), "concatsquash", "elu", {}, {}),
    ("d3_h16x16_concatsquash_swish", 3, (16, 16), "concatsquash", "swish", {}, {}),
    ("d3_h16x16_concatsquash_square", 3, (16, 16), "concatsquash", "square", {}, {}),
    ("d3_h16x16_concatsquash_identity", 3, (16, 16), "concatsquash", "identity", {}, {}),
    ("d4_h32_concat_tanh_residual", 4, (32,), "concat", "tanh", {}, {"residual": True}),
    ("d4_h32_concat_tanh_scale2p5", 4, (32,), "concat", "tanh", {"scale_output": 2.5}, {}),
    ("d16_h64x64_concatsquash_tanh", 16, (64, 64), "concatsquash", "tanh", {}, {}),
]


def import_reference():
    placeholder = types.ModuleType("torchdiffeq")
    placeholder.odeint_adjoint = None       # the name cnf.py imports; never called
    sys.modules["torchdiffeq"] = placeholder
    make_golden.import_reference()
    from flowcon.CNF import cnf
    from flowcon.CNF.neural_odes import odefunc
    return cnf, odefunc


def evaluate(func, t, y, logp):
    """``(net, dy, negdiv)`` of the reference's eval-mode ODE function (it marks its inputs as requiring grad)."""
    net = func.diffeq(t.clone(), y.clone()).detach()
    dy, negdiv = func(t.clone(), (y.clone(), logp.clone()))[:2]
    return net, dy.detach(), negdiv.detach()


def record(cnf_module, odefunc_module, index, name, d, hidden, layer_type, nonlinearity, net_kw, func_kw):
    seed = 4100 + 13 * index
    torch.manual_seed(seed)
    net = odefunc_module.ODEnet(hidden, (d,), None, False, layer_type=layer_type, nonlinearity=nonlinearity, **net_kw)
    with torch.no_grad():
        for key, p in net.named_parameters():
            if "_hypernet" in key:               # initialised to (near) zero: give the weights of t something to do
                p.add_(0.3 * torch.randn(p.shape))
    func = odefunc_module.ODEfunc(net, divergence_fn="approximate", **func_kw).eval()
    gen = torch.Generator().manual_seed(seed)
    y = 1.5 * torch.randn(ROWS, d, generator=gen)
    logp = torch.randn(ROWS, 1, generator=gen)
    t = torch.tensor(0.37)
    func64 = copy.deepcopy(func).double()
    net32, dy32, nd32 = evaluate(func, t, y, logp)
    net64, dy64, nd64 = evaluate(func64, t.double(), y.double(), logp.double())
    for v in (net32, dy32, nd32, net64, dy64, nd64):
        assert torch.isfinite(v).all(), name
    assert nd32.shape == (ROWS, 1) and dy32.shape == (ROWS, d), name
    out = {"sd::" + k: v.detach().clone().numpy() for k, v in func.state_dict().items()}
    if index == 0:
        flow = cnf_module.CNF(func, T=0.5, train_T=True)
        out.update({"cnf_sd::" + k: v.detach().clone().numpy() for k, v in flow.state_dict().items()})
    out.update(t=t.numpy(), y=y.numpy(), logp=logp.numpy(), net32=net32.numpy(), dy32=dy32.numpy(),
               negdiv32=nd32.numpy(), net64=net64.numpy(), dy64=dy64.numpy(), negdiv64=nd64.numpy())
    for tag, a32, a64 in (("net", net32, net64), ("dy", dy32, dy64), ("negdiv", nd32, nd64)):
        out["floor_" + tag] = np.float64((a32.double() - a64).abs().max().item())
    path = os.path.join(HERE, "cnf_%s.npz" % name)
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size <= SIZE_LIMIT, (name, size)
    print("%-36s floor net %.1e dy %.1e negdiv %.1e | max|dy| %.2f max|div| %.2f | %d B"
          % (name, out["floor_net"], out["floor_dy"], out["floor_negdiv"], float(dy64.abs().max()),
             float(nd64.abs().max()), size))


def main():
    cnf_module, odefunc_module = import_reference()
    for index, case in enumerate(CASES):
        record(cnf_module, odefunc_module, index, *case)


if __name__ == "__main__":
    main()
