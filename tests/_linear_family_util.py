"""Shared by tests/test_linear_family_host.py and tests/test_gpu_linear_family.py: the SVDLinear / QRLinear fixtures of
tests/golden/make_linear_family_golden.py."""
import os
import re

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = ["svd_linear_d5_k2", "svd_linear_d64_k64", "svd_linear_d130_k6",
            "qr_linear_d5_k3", "qr_linear_d64_k16", "qr_linear_d130_k4"]
STATE_KEYS = {"svd": {"bias", "orthogonal_1.q_vectors", "unconstrained_diagonal", "orthogonal_2.q_vectors"},
              "qr": {"bias", "upper_entries", "log_upper_diag", "orthogonal.q_vectors"}}

_loaded = {}


def fixture(name):
    """``(tensors, kind, D, K)``: every array as a CPU tensor, the float64 outputs restored from the float32 array plus the
    stored difference; loaded once."""
    if name not in _loaded:
        kind, d, k = re.match(r"(svd|qr)_linear_d(\d+)_k(\d+)$", name).groups()
        g = np.load(os.path.join(GOLDEN, name + ".npz"))
        t = {key: torch.from_numpy(g[key]) for key in g.files}
        t["y64"] = t["y32"].double() + t["y64_minus_y32"].double()
        t["xinv64"] = t["xinv32"].double() + t["xinv64_minus_xinv32"].double()
        _loaded[name] = (t, kind, int(d), int(k))
    return _loaded[name]


def build(name):
    """The module of a fixture with the reference's checkpoint loaded (strict), in eval mode, on the CPU."""
    import flowconductor_amd.transforms as T

    t, kind, d, k = fixture(name)
    module = (T.SVDLinear if kind == "svd" else T.QRLinear)(d, k)
    module.load_state_dict({key[4:]: v for key, v in t.items() if key.startswith("sd::")}, strict=True)
    return module.eval()
