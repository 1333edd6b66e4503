"""Generate tests/golden/spd_*.npz (flows on SPD matrices) by importing the REFERENCE (FlowConductor) itself.

Runs only where the reference tree exists:
    python tests/golden/make_spd_golden.py
It uses make_golden.py's import (with its placeholder for the third-party ``UMNN`` package).  Each spd_m<m>.npz holds,
for FillTriangular, TransformDiagonalSoftplus and CholeskyOuterProduct(m) in both directions, the inputs, the
reference's float32 outputs / logabsdets and the same in float64 (keys ending in 64).  spd_flow_m3.npz holds a whole
flow's state_dict (``sd::`` keys), SPD data and the reference's log_prob.  These fixtures are not part of
cases.CASES.
"""
import copy
import os

import numpy as np
import torch

from make_golden import HERE, import_reference

SIZES = {1: 32, 3: 32, 4: 32, 17: 12, 53: 4, 64: 3, 128: 1}


def spd(gen, n, m, dtype=torch.float32):
    """A A^T / m + I, symmetrised exactly."""
    a = torch.randn(n, m, m, generator=gen, dtype=torch.float64)
    s = a @ a.mT / m + torch.eye(m, dtype=torch.float64)
    s = s.to(dtype)
    return 0.5 * (s + s.mT)


def lower(gen, n, m):
    low = torch.tril(torch.randn(n, m, m, generator=gen), -1) * 0.5
    diag = torch.rand(n, m, generator=gen) * 1.5 + 0.25
    return low + torch.diag_embed(diag)


def both(t, x, inverse):
    """The reference module in float32 and a float64 copy of it."""
    with torch.no_grad():
        f = t.inverse if inverse else t
        y, lad = f(x)
        t64 = copy.deepcopy(t).double()
        f64 = t64.inverse if inverse else t64
        y64, lad64 = f64(x.double())
    return [a.numpy() for a in (y, lad, y64, lad64)]


def flow_case(L):
    T = L.transforms
    torch.manual_seed(7)
    m, d = 3, 6
    flow = L.flows.Flow(T.InverseTransform(T.CompositeTransform([
        T.PiecewiseRationalQuadraticCouplingTransform(
            L.utils.create_alternating_binary_mask(d, even=True),
            lambda i, o: L.nets.ResidualNet(i, o, hidden_features=32, num_blocks=2),
            num_bins=8, tails="linear", tail_bound=5.0),
        T.FillTriangular(features=d),
        T.TransformDiagonalSoftplus(m),
        T.CholeskyOuterProduct(m)])), L.distributions.StandardNormal([d])).eval()
    # perturb the final layers so the coupling is not the identity
    with torch.no_grad():
        for p in flow.parameters():
            if p.requires_grad:
                p.add_(0.05 * torch.randn_like(p))
    gen = torch.Generator().manual_seed(11)
    x = spd(gen, 64, m)
    with torch.no_grad():
        lp = flow.log_prob(x)
    out = {"x": x.numpy(), "log_prob": lp.numpy()}
    out.update({"sd::" + k: v.detach().numpy() for k, v in flow.state_dict().items()})
    np.savez_compressed(os.path.join(HERE, "spd_flow_m3.npz"), **out)


def main():
    L = import_reference()
    T = L.transforms
    for m, n in SIZES.items():
        gen = torch.Generator().manual_seed(1000 + m)
        d = m * (m + 1) // 2
        out = {}
        fill = T.FillTriangular(features=d)
        v = torch.randn(n, d, generator=gen)
        out["fill_x"] = v.numpy()
        with torch.no_grad():
            out["fill_y"] = fill(v)[0].numpy()
            out["fill_inv"] = fill.inverse(fill(v)[0])[0].numpy()
        diag = T.TransformDiagonalSoftplus(m)
        md = torch.randn(n, m, m, generator=gen)
        out["diag_x"] = md.numpy()
        out["diag_fwd_y"], out["diag_fwd_lad"], out["diag_fwd_y64"], out["diag_fwd_lad64"] = both(diag, md, False)
        pos = torch.rand(n, m, m, generator=gen) + 0.1
        out["diag_inv_x"] = pos.numpy()
        out["diag_inv_y"], out["diag_inv_lad"], out["diag_inv_y64"], out["diag_inv_lad64"] = both(diag, pos, True)
        chol = T.CholeskyOuterProduct(m)
        lo = lower(gen, n, m)
        out["chol_fwd_x"] = lo.numpy()
        out["chol_fwd_y"], out["chol_fwd_lad"], out["chol_fwd_y64"], out["chol_fwd_lad64"] = both(chol, lo, False)
        a = spd(gen, n, m)
        out["chol_inv_x"] = a.numpy()
        out["chol_inv_y"], out["chol_inv_lad"], out["chol_inv_y64"], out["chol_inv_lad64"] = both(chol, a, True)
        for name, mod in (("chol", chol), ("diag", diag)):
            out.update({"sd::%s::%s" % (name, k): t.numpy() for k, t in mod.state_dict().items()})
        path = os.path.join(HERE, "spd_m%d.npz" % m)
        np.savez_compressed(path, **out)
        print(path, os.path.getsize(path))
    flow_case(L)


if __name__ == "__main__":
    main()
