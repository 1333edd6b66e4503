"""Shared by tests/test_distributions_host.py and tests/test_gpu_distributions.py: the fixtures of
tests/golden/make_distributions_golden.py, the margin rule and float64 restatements of the four kernels."""
import os

import numpy as np
import torch
from torch import nn

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BERNOULLI = {"d1": [1], "d3": [3], "d64": [64], "d65": [65], "d130": [130], "d784": [784], "s2x3x5": [2, 3, 5]}
IDENTITY, FRACTIONAL = "d65", "s2x3x5"
WITH_GRADIENTS = [name for name, shape in BERNOULLI.items() if int(np.prod(shape)) <= 130]
SAMPLES = ["c5s7", "c4s1"]
BOX = [1, 3, 64, 130]
EPS = 2.0 ** -23          # spacing of float32 relative to a power of two

_loaded = {}


def fixture(name):
    """Every array of tests/golden/<name>.npz as a CPU tensor (``mean64`` restored from its stored difference); loaded
    once, never modified."""
    if name not in _loaded:
        g = np.load(os.path.join(GOLDEN, name + ".npz"))
        t = {key: torch.from_numpy(np.asarray(g[key])) for key in g.files}
        if "mean32" in t:
            t["mean64"] = t["mean32"].double() + t["mean64_minus_mean32"].double()
        _loaded[name] = t
    return _loaded[name]


def bound(reference, floor):
    """The project's golden margin (tests/test_gpu_golden.py) -- 4 x the noise floor of the reference's own float32 path --
    and never below 4 float32 ulps of the largest magnitude compared (each value is a few rounded operations per
    element)."""
    reference = torch.as_tensor(reference)
    finite = reference[torch.isfinite(reference)]
    largest = float(finite.abs().max()) if finite.numel() else 0.0
    return max(4.0 * float(floor), 4.0 * float(np.spacing(np.float32(largest))))


def check(what, got, reference, floor):
    """``got`` within ``bound`` of the float64 ``reference``; prints the figures first."""
    reference = torch.as_tensor(reference).double()
    got = got.detach().cpu().double()
    assert got.shape == reference.shape, (what, tuple(got.shape), tuple(reference.shape))
    err, limit = float((got - reference).abs().max()), bound(reference, floor)
    print("%s: err %.3g bound %.3g (floor %.3g)" % (what, err, limit, float(floor)))
    assert err <= limit, (what, err, limit)


def state_dict(name):
    return {key[4:]: v for key, v in fixture("bernoulli_" + name).items() if key.startswith("sd::")}


def build_bernoulli(name, device="cpu"):
    """The fixture's ``ConditionalIndependentBernoulli`` with the reference's checkpoint loaded (strict)."""
    from flowconductor_amd.distributions import ConditionalIndependentBernoulli

    shape = BERNOULLI[name]
    encoder = None if name == IDENTITY else nn.Linear(4, int(np.prod(shape)))
    dist = ConditionalIndependentBernoulli(shape, encoder)
    dist.load_state_dict(state_dict(name), strict=True)
    return dist.to(device)


def tap_logits(dist, context):
    """``(context, taps)``: after a ``log_prob`` call ``taps[0].grad`` is the gradient with respect to the logits -- the
    encoder's output through a forward hook, or the context itself under the identity encoder."""
    taps = []
    if isinstance(dist._context_encoder, nn.Module):
        def tap(module, args, result):
            if result.requires_grad:
                result.retain_grad()
                taps.append(result)
        dist._context_encoder.register_forward_hook(tap)
    else:
        context = context.requires_grad_(True)
        taps.append(context)
    return context, taps


# ---- float64 restatements --------------------------------------------------------------------------------------------
def bernoulli_terms(x, logits):
    """The summands of the reference's expression (distributions/discrete.py:54)."""
    return -x * nn.functional.softplus(-logits) - (1.0 - x) * nn.functional.softplus(logits)


def layout_inputs(d, rows=257, seed=11):
    """Seeded [rows, d] inputs for the layout tests: 0 / 1 ``x``, logits 4 randn, ``g``, ``noise``, a box and points of which
    about a third lie outside it.  Generated once per width."""
    key = ("layout", d, rows, seed)
    if key not in _loaded:
        gen = torch.Generator().manual_seed(seed + d)
        x = (torch.rand(rows, d, generator=gen) < 0.5).float()
        logits = torch.randn(rows, d, generator=gen) * 4.0
        g = torch.randn(rows, generator=gen)
        noise = torch.rand(rows, d, generator=gen)
        low = -1.0 - torch.rand(d, generator=gen)
        high = 1.0 + torch.rand(d, generator=gen)
        points = low + (high - low) * torch.rand(rows, d, generator=gen)
        out = torch.rand(rows, generator=gen) < 1.0 / 3.0
        points[out, 0] = high[0] + 0.5
        terms = bernoulli_terms(x.double(), logits.double())
        _loaded[key] = dict(x=x, logits=logits, g=g, noise=noise, low=low, high=high, points=points, outside=out,
                            logp64=terms.sum(1), magnitude=terms.abs().sum(1),
                            probs64=torch.sigmoid(logits.double()),
                            volume64=torch.log(high.double() - low.double()).sum())
    return _loaded[key]
