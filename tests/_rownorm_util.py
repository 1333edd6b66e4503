"""Shared by tests/test_rownorm_host.py and tests/test_gpu_rownorm.py: the fixtures of tests/golden/make_rownorm_golden.py
and CPU restatements (any dtype, differentiable) of the three maps."""
import math
import os
import re

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RADIAL = ["radial_d%d" % d for d in (1, 2, 5, 64, 130)]
UNIT = ["unit_vector_d%d" % d for d in (1, 2, 3, 20, 63, 130)]
NAIVE = ["naive_linear_d%d" % d for d in (1, 5, 64, 130)]
FIXTURES = RADIAL + UNIT + NAIVE
STATE_KEYS = {"radial": ["beta", "alpha", "z_0", "d"], "unit_vector": ["dim_sphere"], "naive_linear": ["bias", "_weight"]}

_loaded = {}


def fixture(name):
    """``(tensors, kind, d)``: every array as a CPU tensor, the float64 outputs restored from the float32 array plus the
    stored difference; loaded once."""
    if name not in _loaded:
        kind, d = re.match(r"(radial|unit_vector|naive_linear)_d(\d+)$", name).groups()
        g = np.load(os.path.join(GOLDEN, name + ".npz"))
        t = {key: torch.from_numpy(np.asarray(g[key])) for key in g.files}
        t["y64"] = t["y32"].double() + t["y64_minus_y32"].double()
        if "xinv32" in t:
            t["xinv64"] = t["xinv32"].double() + t["xinv64_minus_xinv32"].double()
        _loaded[name] = (t, kind, int(d))
    return _loaded[name]


def state_dict(name):
    return {key[4:]: v for key, v in fixture(name)[0].items() if key.startswith("sd::")}


def build(name, **kw):
    """The module of a fixture with the reference's checkpoint loaded (strict), in eval mode, on the CPU."""
    import flowconductor_amd.transforms as T

    t, kind, d = fixture(name)
    module = {"radial": T.RadialTransform, "unit_vector": T.UnitVector, "naive_linear": T.NaiveLinear}[kind](d, **kw)
    module.load_state_dict(state_dict(name), strict=True)
    return module.eval()


def bound(scale, floor):
    """The rule of tests/test_gpu_golden.py:21-44."""
    return 1e-5 * max(1.0, float(scale)) + 4.0 * float(floor)


# ---- restatements ---------------------------------------------------------------------------------------------------
def radial_ab(alpha, beta):
    a = torch.abs(alpha)
    return a, torch.log(1 + torch.exp(beta)) - a


def radial_forward(x, z_0, alpha, beta):
    """no_analytic_inv/planar.py:199-211 in that operation order; ``x`` [N, D], ``z_0`` [1, D]."""
    a, b = radial_ab(alpha, beta)
    dz = x - z_0
    r = torch.linalg.vector_norm(dz, dim=1, keepdim=True)
    h = b / (a + r)
    hr = -b * r / (a + r) ** 2
    lad = (x.shape[1] - 1) * torch.log(1 + h) + torch.log(1 + h + hr)
    return x + h * dz, lad.reshape(-1)


def radial_inverse(y, z_0, alpha, beta):
    """The closed form: r is the non-negative root of r^2 + (a + b - rho) r - a rho = 0 in the form that does not cancel."""
    a, b = radial_ab(alpha, beta)
    dz = y - z_0
    rho = torch.linalg.vector_norm(dz, dim=1, keepdim=True)
    q = a + b - rho
    root = torch.sqrt(q * q + 4 * a * rho)
    r = torch.where(q > 0, 2 * a * rho / (q + root), (root - q) / 2)
    h = b / (a + r)
    hr = -b * r / (a + r) ** 2
    lad = (y.shape[1] - 1) * torch.log(1 + h) + torch.log(1 + h + hr)
    return z_0 + dz / (1 + h), -lad.reshape(-1)


def unit_forward(x):
    """unitvector.py:18-27, 43-53."""
    s = torch.sum(x ** 2, dim=-1, keepdim=True)
    y = torch.cat([2 * x, s - 1], dim=-1) / (s + 1)
    return y, x.shape[-1] * (math.log(2.0) - torch.log1p(s.squeeze(-1)))


def unit_inverse(y):
    """unitvector.py:29-37 (without the domain check)."""
    x = (y / (1 - y[..., -1:]))[..., :-1]
    return x, -(x.shape[-1] * (math.log(2.0) - torch.log1p(torch.sum(x ** 2, dim=-1))))


def naive_forward(x, weight, bias):
    return x @ weight.T + bias, torch.linalg.slogdet(weight)[1] * x.new_ones(x.shape[0])


def naive_inverse(y, weight, bias):
    return torch.linalg.solve(weight, (y - bias).T).T, -torch.linalg.slogdet(weight)[1] * y.new_ones(y.shape[0])


def restate(name, x, dtype, inverse=False):
    """The fixture's map on ``x`` in ``dtype`` with the fixture's parameters: ``(outputs, logabsdet)``."""
    t, kind, d = fixture(name)
    sd = {k: v.to(dtype) if v.is_floating_point() else v for k, v in state_dict(name).items()}
    x = x.to(dtype)
    if kind == "radial":
        return (radial_inverse if inverse else radial_forward)(x, sd["z_0"], sd["alpha"], sd["beta"])
    if kind == "unit_vector":
        return unit_inverse(x) if inverse else unit_forward(x)
    return (naive_inverse if inverse else naive_forward)(x, sd["_weight"], sd["bias"])
