"""Shared by tests/test_deep_sigmoid_host.py and tests/test_gpu_deep_sigmoid.py: the deep-sigmoidal-flow fixtures
(tests/golden/make_deep_sigmoid_golden.py) and a torch restatement of the map (flowcon/transforms/adaptive_sigmoids.py:177-210)
that runs in
float64 (the yardstick) or float32 (what float32 autograd loses, for the gradient tolerances)."""
import copy
import glob
import math
import os
import re

import numpy as np
import torch
import torch.nn.functional as F

import flowconductor_amd.transforms as T

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = sorted(os.path.basename(p)[len("deep_sigmoid_"):-4] for p in glob.glob(os.path.join(GOLDEN, "deep_sigmoid_*.npz")))
DS_FIXTURES = [n for n in FIXTURES if n.startswith("ds_")]
MADE_FIXTURES = [n for n in FIXTURES if n.startswith("made_")]
PER_SAMPLE = "ps_f6_s8"

_loaded = {}


def fixture(name):
    if name not in _loaded:
        _loaded[name] = np.load(os.path.join(GOLDEN, "deep_sigmoid_%s.npz" % name))
    return _loaded[name]


def tensor(z, key, dtype=None):
    t = torch.from_numpy(z[key])
    return t if dtype is None else t.to(dtype)


def state(z):
    return {k[4:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd::")}


def build(name, load=True):
    """The project's module of a fixture, its ``sd::`` state loaded with ``strict=True``, in eval mode."""
    torch.manual_seed(11)
    if name.startswith("ds_"):
        f, s, m = (int(v) for v in re.match(r"ds_f(\d+)_s(\d+)_m(\d+)$", name).groups())
        module = T.DeepSigmoid(f, n_sigmoids=s, mollify=m / 100.0)
    elif name == PER_SAMPLE:
        module = T.DeepSigmoid(6, n_sigmoids=8)
    else:
        d, h, s, c = (int(v) for v in re.match(r"made_d(\d+)_h(\d+)_s(\d+)_ctx(\d+)$", name).groups())
        module = T.MaskedDeepSigmoidTransform(d, h, n_sigmoids=s, context_features=c or None)
    if load:
        module.load_state_dict(state(fixture(name)), strict=True)
    return module.eval()


def restate(x, dsparams, n_sigmoids, mollify, eps, dtype=torch.float64):
    """``(y, logabsdet per element)`` of the deep sigmoidal flow, ``dsparams`` [..., F, 3S] broadcast against ``x`` [..., F]."""
    S = n_sigmoids
    x, p = x.to(dtype), dsparams.to(dtype)
    a = F.softplus(p[..., :S]) * (1 - mollify) + mollify
    b = p[..., S:2 * S] * (1 - mollify)
    pre = a * x.unsqueeze(-1) + b
    s = (torch.softmax(p[..., 2 * S:], dim=-1) * torch.sigmoid(pre)).sum(-1)
    c = s * (1 - eps) + eps * 0.5

    # (the operation order is the reference's, down to log(v) written as log(100 v) - log(100) and 1 - c by subtraction: where
    #  the map saturates, c -> 1 - eps / 2, float64 itself only holds log(1 - c) to ~1e-11, and the fixtures are matched
    #  to 1e-12)
    def log(v):
        return torch.log(v * 1e2) - math.log(1e2)

    y = log(c) - log(1 - c)
    lj = torch.log_softmax(p[..., 2 * S:], dim=-1) + -(F.softplus(-pre) + eps) + -(F.softplus(pre) + eps) + log(a)
    return y, torch.logsumexp(lj, dim=-1) + math.log(1 - eps) - (log(c) + log(-c + 1))


def model(name, module, dtype=torch.float64):
    """``fn(x, context=None, dsparams=None) -> (y, logabsdet [N])``: the restatement under a CPU copy of ``module``'s
    parameters in ``dtype``; also returns that copy (its parameters are the leaves for gradients)."""
    twin = copy.deepcopy(module).to("cpu").to(dtype)

    if name.startswith("made_"):
        ds = twin.deep_sigmoid_module

        def fn(x, context=None, dsparams=None):
            x = x.to(dtype)
            raw = twin.autoregressive_net(x, None if context is None else context.to(dtype))
            params = raw.view(x.shape[0], twin.features, 3 * twin.n_sigmoids) / 5
            y, lad = restate(x, params, twin.n_sigmoids, ds._mollify, ds.eps, dtype)
            return y, lad.sum(-1)
    else:
        def fn(x, context=None, dsparams=None):
            params = twin.dsparams if dsparams is None else dsparams
            y, lad = restate(x, params, twin.n_sigmoids, twin._mollify, twin.eps, dtype)
            return y, lad.sum(-1)
    return fn, twin


def maxdiff(a, b):
    return float((a.detach().cpu().double() - b.detach().cpu().double()).abs().max())


def row_maxdiff(a, b):
    """max |a - b| per row, [N]."""
    d = (a.detach().cpu().double() - b.detach().cpu().double()).abs()
    return d.reshape(d.shape[0], -1).max(dim=1).values
