"""Shared by tests/test_mog_host.py and tests/test_gpu_mog.py: the mixture-of-Gaussians fixtures and float64 restatements of
the reference's density (flowcon/nn/nde/made.py:328-353) and of the sampler's selection rule."""
import copy
import glob
import math
import os
import re

import numpy as np
import torch
import torch.nn.functional as F

from flowconductor_amd.distributions import MADEMoG

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = sorted(os.path.basename(p)[4:-4] for p in glob.glob(os.path.join(GOLDEN, "mog_*.npz")))
FAR_ROWS = 8          # the first rows of every fixture's x sit at +-50
NEAR_TIE = 1e-5       # a row is left out when |uniform S - partial sum| / S falls below this in the float64 run

_loaded = {}


def fixture(name):
    """``(npz, (D, hidden, C, context or None, blocks))``; loaded once."""
    if name not in _loaded:
        dims = tuple(int(v) for v in re.match(r"d(\d+)_h(\d+)_c(\d+)_ctx(\d+)_b(\d+)$", name).groups())
        dims = dims[:3] + (dims[3] or None,) + dims[4:]
        _loaded[name] = (np.load(os.path.join(GOLDEN, "mog_%s.npz" % name)), dims)
    return _loaded[name]


def build(features, hidden, components, context, blocks, state=None, seed=None):
    """An eval-mode MADEMoG; ``state``: a fixture's ``sd::`` entries (strict), else custom initialisation times 1.5 with
    perturbed block outputs (the recipe of make_mog_golden.py)."""
    torch.manual_seed(features * 1000 + hidden if seed is None else seed)
    dist = MADEMoG(features, hidden, context, num_blocks=blocks, num_mixture_components=components,
                   custom_initialization=True)
    if state is not None:
        dist.load_state_dict({k[4:]: torch.from_numpy(state[k]) for k in state.files if k.startswith("sd::")}, strict=True)
    else:
        with torch.no_grad():
            for p in dist.parameters():
                p.mul_(1.5)
            for block in dist._made.blocks:
                last = block.linear_layers[-1]
                last.weight.add_(0.3 / hidden ** 0.5 * torch.randn(last.weight.shape))
                last.bias.add_(0.1 * torch.randn(last.bias.shape))
    return dist.eval()


def density64(params, x, components, epsilon):
    """The reference's expression in float64 on ``params`` [N, D * 3C] (or [N, 3C] with ``x`` [N])."""
    out = params.double().reshape(*x.shape, components, 3)
    logits, means, ustd = out[..., 0], out[..., 1], out[..., 2]
    stds = F.softplus(ustd) + epsilon
    terms = torch.logsumexp(torch.log_softmax(logits, dim=-1)
                            - 0.5 * (math.log(2 * math.pi) + 2 * torch.log(stds) + ((x.double()[..., None] - means) / stds) ** 2),
                            dim=-1)
    return terms


def sample64(dist, normal, uniform, context, margin=NEAR_TIE):
    """float64 restatement of ``_sample_from_noise``: column d takes k = min{k : u_d S < sum_{j <= k} e_j} (last component
    as the fallback), x_d = mean_k + std_k normal_d.  Returns ``(draws, kept rows, log-density of the draws)``; a row is
    not kept when some column has ``|u S - partial sum| / S < margin`` at a boundary between two components."""
    made = copy.deepcopy(dist._made).double().cpu()
    normal, uniform = normal.double().cpu(), uniform.double().cpu()
    context = None if context is None else context.double().cpu()
    n, features, components = normal.shape[0], made.features, made.num_mixture_components
    x = torch.zeros(n, features, dtype=torch.float64)
    keep = torch.ones(n, dtype=torch.bool)
    logp = torch.zeros(n, dtype=torch.float64)
    with torch.no_grad():
        for d in range(features):
            params = made.forward(x, context).reshape(n, features, 3 * components)[:, d]
            out = params.reshape(n, components, 3)
            e = torch.exp(out[:, :, 0] - out[:, :, 0].max(dim=1, keepdim=True).values)
            total = e.sum(dim=1)
            target = uniform[:, d] * total
            chosen = torch.full((n,), components - 1, dtype=torch.long)
            partial = torch.zeros(n, dtype=torch.float64)
            found = torch.zeros(n, dtype=torch.bool)
            for k in range(components):
                partial = partial + e[:, k]
                take = ~found & (target < partial)
                chosen[take] = k
                found |= take
                if k < components - 1:
                    keep &= ~((target - partial).abs() / total < margin)
            std = F.softplus(out[:, :, 2]) + made.epsilon
            rows = torch.arange(n)
            x[:, d] = out[rows, chosen, 1] + std[rows, chosen] * normal[:, d]
            logp += density64(params, x[:, d], components, made.epsilon)
    return x, keep, logp


def noise(n, features, context, seed):
    g = torch.Generator().manual_seed(seed)
    normal, uniform = torch.randn(n, features, generator=g), torch.rand(n, features, generator=g)
    return normal, uniform, (None if context is None else torch.randn(n, context, generator=g))
