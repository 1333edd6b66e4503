"""Generate tests/golden/umnn_<case>.npz (unconstrained monotonic neural networks) from the REFERENCE's own classes.

Runs only where the reference tree exists:
    python tests/golden/make_umnn_golden.py
It follows make_golden.import_reference's recipe, but in place of the empty ``UMNN`` placeholder it installs a working
stand-in for the third-party package (which is neither vendored by the reference nor installed):
``NeuralIntegral.apply(x0, xT, net, flat_params, h, nb_steps)`` (and ``ParallelNeuralIntegral``) is Clenshaw-Curtis
quadrature on the nodes cos(i pi / nb_steps) with the weights of this package's ``cc_weights``.

What each side pins.  The reference's ``MonotonicNormalizer``, ``IntegrandNet`` and the three transform classes produce
the vectors, so the fixtures pin everything the reference decides: the embedding layout, ``z0 = h[:, :, 0]``, ELU + 1, the
reshape / transpose of ``IntegrandNet.forward``, the 25-step bisection and the ``state_dict`` keys.  The quadrature rule
itself is NOT pinned by them (it is this package's on both sides); it is pinned by the exactness test of
tests/test_umnn_host.py (every monomial up to degree nb_steps).

Files: ``umnn_<case>.npz`` for ``CASES``, parameters multiplied by 1.5 after construction.  Each holds ``sd::*``, ``x``
[257, D] ~ 1.5 N(0, 1) whose first ``far_rows`` = 4 rows are +-8 and +-19, ``context`` where there is one, the reference's
``y32`` / ``lad32`` and ``y64`` / ``lad64`` (a ``.double()`` deep copy), the inverse of ``y64`` in both precisions
(``xinv32`` / ``ladinv32``, ``xinv64`` / ``ladinv64``), two more inverse rows with every target +-1e4 (``ysat``,
``xsat32`` / ``xsat64``), and the float32 floors max|32 - 64| of each, separately for the ordinary rows (``_body``), the
far rows (``_far``) and the saturated rows (``floor_xsat``).  The script asserts min f >= 0.05 over its rows (another seed
otherwise), so the inverse amplifies an error of y by at most 20.
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
from flowconductor_amd.transforms.UMNN import cc_weights  # noqa: E402

ROWS = 257
FAR = 4
SIZE_LIMIT = 900 * 1024
CASES = [
    # name, kind, kwargs
    ("made_d5_h32_c20_s20_l50x50x50", "made", dict(features=5, hidden_features=32)),
    ("made_d3_h16_c7_s8_l16_ctx4", "made", dict(features=3, hidden_features=16, context_features=4, cond_size=7,
                                                nb_steps=8, integrand_net_layers=[16])),
    ("made_d33_h24_c31_s5_l64x64", "made", dict(features=33, hidden_features=24, cond_size=31, nb_steps=5,
                                                integrand_net_layers=[64, 64])),
    ("coupling_d6_c20_s20_l50x50x50", "coupling", dict()),
    ("cond_d4_ctx3_c12_s20_l50x50", "cond", dict(features=4, hidden_features=24, context_features=3, cond_size=12,
                                                 integrand_net_layers=[50, 50])),
]


class _Quadrature:
    """The stand-in: int_{x0}^{xT} net(t, h) dt by Clenshaw-Curtis with ``cc_weights`` (plain autograd)."""

    @staticmethod
    def apply(x0, xT, net, flat_params, h, nb_steps):
        nodes, weights = cc_weights(nb_steps)
        nodes = torch.as_tensor(nodes).to(xT)
        weights = torch.as_tensor(weights).to(xT)
        half = (xT - x0) / 2
        total = torch.zeros_like(xT)
        for s, w in zip(nodes, weights):
            total = total + w * net(x0 + half * (s + 1), h)
        return half * total


def import_reference():
    """make_golden.import_reference with a working ``UMNN`` module in place of its placeholder."""
    umnn = types.ModuleType("UMNN")
    umnn.NeuralIntegral = _Quadrature
    umnn.ParallelNeuralIntegral = _Quadrature
    sys.modules["UMNN"] = umnn          # found before the placeholder directory that the recipe puts on sys.path
    return make_golden.import_reference()


def build(L, kind, kw, seed):
    torch.manual_seed(seed)
    T = L.transforms
    if kind == "made":
        module = T.MaskedUMNNAutoregressiveTransform(**kw)
    elif kind == "cond":
        module = T.ConditionalUMNNTransform(**kw)
    else:
        mask = L.utils.create_alternating_binary_mask(6, even=True)
        module = T.UMNNCouplingTransform(
            mask, lambda i, o: L.nets.ResidualNet(i, o, hidden_features=32, num_blocks=2))
    with torch.no_grad():
        for p in module.parameters():
            p.mul_(1.5)
        net = getattr(module, "autoregressive_net", None) or getattr(module, "transform_net", None) \
            or module.conditional_net
        for block in getattr(net, "blocks", []):          # the residual blocks' (near-)zero last layers
            last = block.linear_layers[-1]
            last.weight.add_(0.3 / last.in_features ** 0.5 * torch.randn(last.weight.shape))
            last.bias.add_(0.1 * torch.randn(last.bias.shape))
    return module.eval()


def min_integrand(module, kind, x, context):
    """min f over the rows, from the log-determinant's parts."""
    with torch.no_grad():
        if kind == "made":
            h = module.autoregressive_net(x, context).reshape(x.shape[0], x.shape[1], -1)
            xt = x
        elif kind == "cond":
            h = module.conditional_net(context).reshape(x.shape[0], x.shape[1], -1)
            xt = x
        else:
            xt = x[:, module.transform_features]
            h = module.transform_net(x[:, module.identity_features], None).reshape(xt.shape[0], xt.shape[1], -1)
        return float(module.transformer(xt, h)[1].min())


def floor(a32, a64, rows):
    d = (a32.double() - a64).abs()
    return np.float64(d.reshape(d.shape[0], -1)[rows].max().item()) if d.shape[0] else np.float64(0.0)


def record(L, name, kind, kw):
    features = kw.get("features", 6)
    ctx_features = kw.get("context_features")
    for attempt in range(20):
        seed = 900 + 37 * attempt + len(name)
        module = build(L, kind, kw, seed)
        gen = torch.Generator().manual_seed(seed)
        x = 1.5 * torch.randn(ROWS, features, generator=gen)
        x[:FAR] = torch.tensor([8.0, -8.0, 19.0, -19.0]).reshape(-1, 1)
        context = torch.randn(ROWS, ctx_features, generator=gen) if ctx_features else None
        m64 = copy.deepcopy(module).double()
        c64 = None if context is None else context.double()
        fmin = min(min_integrand(module, kind, x, context), min_integrand(m64, kind, x.double(), c64))
        with torch.no_grad():
            y64, lad64 = m64(x.double(), c64)
            xinv64, ladinv64 = m64.inverse(y64, c64)
        if fmin >= 0.05:
            break
    else:
        raise AssertionError("%s: no seed with min f >= 0.05" % name)
    with torch.no_grad():
        y32, lad32 = module(x, context)
        xinv32, ladinv32 = module.inverse(y64.float(), context)
        ysat = torch.stack((torch.full((features,), 1e4), torch.full((features,), -1e4))).double()
        if kind == "coupling":                            # the identity half passes through: keep it ordinary
            ysat[:, module.identity_features] = x[:2, module.identity_features].double()
        csat = None if context is None else context[:2]
        xsat32, _ = module.inverse(ysat.float(), csat)
        xsat64, _ = m64.inverse(ysat, None if csat is None else csat.double())
    for t in (y32, lad32, y64, lad64, xinv32, xinv64, ladinv32, ladinv64, xsat32, xsat64):
        assert torch.isfinite(t).all(), name
    out = {"sd::" + k: v.detach().clone().numpy() for k, v in module.state_dict().items()}
    out.update(x=x.numpy(), far_rows=np.int64(FAR), min_f=np.float64(fmin), y32=y32.numpy(), lad32=lad32.numpy(),
               y64=y64.numpy(), lad64=lad64.numpy(), xinv32=xinv32.numpy(), ladinv32=ladinv32.numpy(),
               xinv64=xinv64.numpy(), ladinv64=ladinv64.numpy(), ysat=ysat.numpy(), xsat32=xsat32.numpy(),
               xsat64=xsat64.numpy())
    if context is not None:
        out["context"] = context.numpy()
    body, far = slice(FAR, None), slice(0, FAR)
    for tag, a32, a64 in (("y", y32, y64), ("lad", lad32, lad64), ("xinv", xinv32, xinv64),
                          ("ladinv", ladinv32, ladinv64)):
        out["floor_%s_body" % tag] = floor(a32, a64, body)
        out["floor_%s_far" % tag] = floor(a32, a64, far)
    out["floor_xsat"] = floor(xsat32, xsat64, slice(None))
    path = os.path.join(HERE, "umnn_%s.npz" % name)
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size <= SIZE_LIMIT, (name, size)
    print("%-32s min f %.3f | y %.1e/%.1e lad %.1e/%.1e | xinv %.1e/%.1e ladinv %.1e/%.1e | sat %.1e | max|y| %.1f | %d B"
          % (name, fmin, out["floor_y_body"], out["floor_y_far"], out["floor_lad_body"], out["floor_lad_far"],
             out["floor_xinv_body"], out["floor_xinv_far"], out["floor_ladinv_body"], out["floor_ladinv_far"],
             out["floor_xsat"], float(np.abs(out["y64"]).max()), size))


def main():
    L = import_reference()
    for name, kind, kw in CASES:
        record(L, name, kind, kw)


if __name__ == "__main__":
    main()
