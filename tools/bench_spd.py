"""Per-layer timing of the SPD-matrix kernels against the reference's torch composition on the same GPU; prints one
JSON line.  Kernel times come from device events around each launch (``ops.KernelTimer``); take a separate
``rocprofv3 --kernel-trace --stats`` run for the profiler's view.
    python tools/bench_spd.py [--batch 65536] [--reps 20] [--sizes 4,16,32,53,64,128]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from flowconductor_amd import ops, transforms  # noqa: E402

HBM = 6.29e12


def timed(fn, reps, name=None):
    fn()
    torch.cuda.synchronize()
    if name:
        with ops.KernelTimer(name) as t:
            for _ in range(reps):
                fn()
        torch.cuda.synchronize()
        return float(np.median(t.durations_ms()))
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / reps


def ref_forward(low, checkargs, m):
    if checkargs:
        iu = np.triu_indices(m, k=1)
        assert torch.all(low[:, iu[0], iu[1]] == 0.)
        assert torch.all(torch.diagonal(low, dim1=-2, dim2=-1) > 0)
    p = torch.bmm(low, low.mT)
    p = 0.5 * (p + p.mT)
    return p, m * np.log(2.) + (torch.arange(m, 0, -1, device=low.device) * torch.diagonal(low, dim1=-2, dim2=-1).log()).sum(-1)


def ref_inverse(a, checkargs, m):
    j = a + torch.eye(m, device=a.device).unsqueeze(0) * 1e-6
    if checkargs:
        assert torch.all(j == j.mT)
        assert torch.all(torch.linalg.eig(j)[0].real >= 0)
    c = torch.linalg.cholesky(j)
    return c, -(m * np.log(2.) + (torch.arange(m, 0, -1, device=a.device) * torch.diagonal(c, dim1=-2, dim2=-1).log()).sum(-1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1 << 16)
    ap.add_argument("--eig-batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sizes", default="4,16,32,53,64,128")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rows = []
    for m in [int(s) for s in args.sizes.split(",")]:
        n = args.batch
        gen = torch.Generator(device=dev).manual_seed(m)
        low = torch.tril(torch.randn(n, m, m, device=dev, generator=gen), -1) * 0.3 + torch.diag_embed(
            torch.rand(n, m, device=dev, generator=gen) + 0.5)
        with torch.no_grad():
            a = torch.bmm(low, low.mT)
            a = 0.5 * (a + a.mT)
        mat_bytes = 8.0 * m * m * n
        d = m * (m + 1) // 2
        for checkargs in (True, False):
            chol = transforms.CholeskyOuterProduct(m, checkargs=checkargs).to(dev)
            with torch.no_grad():
                t_f = timed(lambda: chol(low), args.reps, "fc_cholesky_outer")
                t_i = timed(lambda: chol.inverse(a), args.reps, "fc_cholesky")
                y, _ = chol(low)
                c, _ = chol.inverse(a)
                sub = slice(0, 256)
                l64 = low[sub].double()
                err_f = (y[sub].double() - l64 @ l64.mT).abs().max().item()
                c64 = torch.linalg.cholesky(a[sub].double() + 1e-6 * torch.eye(m, device=dev, dtype=torch.float64))
                err_i = (c[sub].double() - c64).abs().max().item()
                r_f = timed(lambda: ref_forward(low, checkargs, m), max(2, args.reps // 4))
                nb = n if not checkargs else min(n, args.eig_batch)
                r_i = timed(lambda: ref_inverse(a[:nb], checkargs, m), 1) * (n / nb)
            for what, t, r, err in (("cholesky_outer_forward", t_f, r_f, err_f), ("cholesky_inverse", t_i, r_i, err_i)):
                rows.append({"layer": what, "m": m, "batch": n, "checkargs": checkargs, "hip_ms": round(t, 4),
                             "bytes": mat_bytes, "hbm_share": round(mat_bytes / (t * 1e-3) / HBM, 3),
                             "max_err_vs_f64": err, "torch_ms": round(r, 4),
                             "torch_batch": nb if (what == "cholesky_inverse" and checkargs) else n})
        diag = transforms.TransformDiagonalSoftplus(m).to(dev)
        v = torch.randn(n, d, device=dev, generator=gen)
        fill = transforms.FillTriangular(features=d).to(dev)
        with torch.no_grad():
            t_d = timed(lambda: diag(low), args.reps)
            t_fill = timed(lambda: fill(v), args.reps, "fc_tril_pack")
            t_gather = timed(lambda: fill.inverse(low), args.reps, "fc_tril_pack")
            iu = np.tril_indices(m)

            def ref_fill():
                out = v.new_zeros((n, m, m))
                out[:, iu[0], iu[1]] = v
                return out

            r_fill = timed(ref_fill, args.reps)
            r_gather = timed(lambda: low[:, iu[0], iu[1]], args.reps)
        for what, t, r, b in (("transform_diagonal_softplus", t_d, None, 8.0 * m * m * n),
                              ("fill_triangular_forward", t_fill, r_fill, 4.0 * (m * m + d) * n),
                              ("fill_triangular_inverse", t_gather, r_gather, 4.0 * (m * m + d) * n)):
            rows.append({"layer": what, "m": m, "batch": n, "hip_ms": round(t, 4), "bytes": b,
                         "hbm_share": round(b / (t * 1e-3) / HBM, 3), "torch_ms": None if r is None else round(r, 4)})
        print("[bench_spd] m=%d done" % m, file=sys.stderr, flush=True)
    print(json.dumps({"bench": "spd_layers", "device": torch.cuda.get_device_name(0), "rows": rows}))


if __name__ == "__main__":
    main()
