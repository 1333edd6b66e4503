"""Shared by tests/test_umnn_host.py and tests/test_gpu_umnn.py: the UMNN fixtures (tests/golden/make_umnn_golden.py),
the modules they describe and the bound of tests/test_gpu_golden.py."""
import glob
import os
import re

import numpy as np
import torch

import flowconductor_amd.transforms as T
from flowconductor_amd import utils
from flowconductor_amd.nn import nets

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = sorted(os.path.basename(p)[len("umnn_"):-4] for p in glob.glob(os.path.join(GOLDEN, "umnn_*.npz")))
DEFAULT = "made_d5_h32_c20_s20_l50x50x50"

_loaded = {}


def fixture(name):
    if name not in _loaded:
        with np.load(os.path.join(GOLDEN, "umnn_%s.npz" % name)) as z:
            _loaded[name] = {k: z[k] for k in z.files}
    return _loaded[name]


def tensor(z, key, dtype=None, device=None):
    if key not in z:
        return None
    t = torch.from_numpy(z[key])              # the cached arrays stay as they are: .to() below copies
    return t.clone() if dtype is None and device is None else t.to(device=device, dtype=dtype)


def state(z):
    return {k[4:]: torch.from_numpy(z[k]) for k in z if k.startswith("sd::")}


def build(name, load=True):
    """The project's module of a fixture, its ``sd::`` state loaded with ``strict=True``, in eval mode."""
    torch.manual_seed(11)
    layers = [int(v) for v in re.search(r"_l([0-9x]+)", name).group(1).split("x")]
    cond, steps = (int(v) for v in re.search(r"_c(\d+)_s(\d+)_", name).groups())
    kw = dict(integrand_net_layers=layers, cond_size=cond, nb_steps=steps)
    if name.startswith("made_"):
        d, h = (int(v) for v in re.match(r"made_d(\d+)_h(\d+)_", name).groups())
        ctx = re.search(r"_ctx(\d+)$", name)
        module = T.MaskedUMNNAutoregressiveTransform(d, h, context_features=int(ctx.group(1)) if ctx else None, **kw)
    elif name.startswith("cond_"):
        d, ctx = (int(v) for v in re.match(r"cond_d(\d+)_ctx(\d+)_", name).groups())
        module = T.ConditionalUMNNTransform(d, 24, context_features=ctx, **kw)
    else:
        d = int(re.match(r"coupling_d(\d+)_", name).group(1))
        module = T.UMNNCouplingTransform(utils.create_alternating_binary_mask(d, even=True),
                                         lambda i, o: nets.ResidualNet(i, o, hidden_features=32, num_blocks=2), **kw)
    if load:
        module.load_state_dict(state(fixture(name)), strict=True)
    return module.eval()


def bound(ref, floor, factor=1.0):
    """tests/test_gpu_golden.py: 1e-5 max(1, |ref|max) + 4 floor."""
    ref = torch.as_tensor(ref)
    return factor * (1e-5 * max(1.0, float(ref.abs().max())) + 4.0 * float(floor))


def maxdiff(a, b):
    return float((a.detach().cpu().double() - torch.as_tensor(b).detach().cpu().double()).abs().max())


def check_rows(tag, got, z, key, floor_key, far, factor=1.0, rows=None):
    """``got`` against the fixture's float64 ``key`` within the bound, ordinary and far rows separately; prints each
    figure before it asserts."""
    ref = torch.from_numpy(z[key])[:rows]
    for part, sl in (("far", slice(0, far)), ("body", slice(far, None))):
        if ref[sl].numel() == 0:
            continue
        err = maxdiff(got[sl], ref[sl])
        lim = bound(ref[sl], z["%s_%s" % (floor_key, part)], factor)
        print("%s %s %s: err %.3e bound %.3e" % (tag, key, part, err, lim))
        assert err <= lim, (tag, key, part, err, lim)
