"""Per-layer timing of the image-flow kernels against the reference's torch composition on the same GPU; prints one
JSON line.  Both sides are timed the same way: the median of device events around one call of the layer, queued behind
a GPU spin (``timed``); take a separate ``rocprofv3 --kernel-trace --stats`` run for the profiler's view.  The reference's compositions are restated here.
    python tools/bench_image.py [--batch 256] [--reps 20] [--channels 3,12,48,96,128] [--sizes 32,64]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
from flowconductor_amd import distributions, flows, ops, transforms, utils  # noqa: E402
from flowconductor_amd.nn import nets  # noqa: E402

HBM = 6.29e12
SPIN_CYCLES = 200_000   # about 80 us of GPU spin before each timed call


def timed(fn, reps):
    """Median device time of one call of ``fn``: events recorded on the stream right before and after the call, behind
    a GPU spin so that the host has queued the whole call before the first event runs.  Both sides of every comparison
    are timed this way, so host launch overhead and per-launch event placement count for neither."""
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda._sleep(SPIN_CYCLES)
        start.record()
        fn()
        end.record()
        torch.cuda.synchronize()
        times.append(start.elapsed_time(end))
    return float(np.median(times))


# ---- the reference's compositions (reshape.py, conv.py + lu.py), restated ----

def ref_squeeze(x, f):
    b, c, h, w = x.shape
    y = x.view(b, c, h // f, f, w // f, f).permute(0, 1, 3, 5, 2, 4).contiguous()
    return y.view(b, c * f * f, h // f, w // f)


def ref_unsqueeze(x, f):
    b, c, h, w = x.shape
    y = x.view(b, c // f ** 2, f, f, h, w).permute(0, 1, 4, 2, 5, 3).contiguous()
    return y.view(b, c // f ** 2, h * f, w * f)


def ref_conv(x, perm, lower, upper, bias, logdiag):
    b, c, h, w = x.shape
    rows = torch.index_select(x, 1, perm).permute(0, 2, 3, 1).reshape(b * h * w, c)
    out = torch.nn.functional.linear(torch.nn.functional.linear(rows, upper), lower, bias)
    lad = (logdiag * rows.new_ones(b * h * w)).reshape(b, h, w).sum(dim=(1, 2))
    return out.reshape(b, h, w, c).permute(0, 3, 1, 2), lad


TRSM_COLUMNS = 1 << 16   # rocBLAS's trsm refuses C = 128 x 2^18 columns (too small a workspace): solved in chunks


def ref_conv_inverse(x, inv_perm, lower, upper, bias, logdiag):
    b, c, h, w = x.shape
    rows = (x.permute(0, 2, 3, 1).reshape(b * h * w, c) - bias).t()
    parts = []
    for j in range(0, rows.shape[1], TRSM_COLUMNS):
        part = torch.linalg.solve_triangular(lower, rows[:, j:j + TRSM_COLUMNS], upper=False, unitriangular=True)
        parts.append(torch.linalg.solve_triangular(upper, part, upper=True))
    rows = torch.cat(parts, dim=1).t()
    lad = (-logdiag * rows.new_ones(b * h * w)).reshape(b, h, w).sum(dim=(1, 2))
    out = rows.reshape(b, h, w, c).permute(0, 3, 1, 2)
    return torch.index_select(out, 1, inv_perm), lad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--channels", default="3,12,48,96,128")
    ap.add_argument("--sizes", default="32,64")
    ap.add_argument("--flow-batch", type=int, default=256)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rows = []
    n = args.batch
    for s in [int(v) for v in args.sizes.split(",")]:
        for c in [int(v) for v in args.channels.split(",")]:
            x = torch.randn(n, c, s, s, device=dev)
            elem_bytes = 8.0 * x.numel()
            sq = transforms.SqueezeTransform(2)
            conv = transforms.OneByOneConvolution(c, identity_init=False).to(dev).eval()
            with torch.no_grad():
                conv.bias.uniform_(-0.5, 0.5)
                y = sq(x)[0]
                t_sf = timed(lambda: ops.squeeze(x, 2), args.reps)      # the kernel against the composition's copy
                t_si = timed(lambda: ops.squeeze(y, 2, inverse=True), args.reps)
                r_sf = timed(lambda: ref_squeeze(x, 2), args.reps)
                r_si = timed(lambda: ref_unsqueeze(y, 2), args.reps)
                t_cf = timed(lambda: conv(x), args.reps)
                t_ci = timed(lambda: conv.inverse(x), args.reps)
                lower, upper = conv._create_lower_upper()
                perm = conv.permutation._permutation.to(dev)
                inv_perm = torch.argsort(perm)
                logdiag = conv.upper_diag.log().sum()
                r_cf = timed(lambda: ref_conv(x, perm, lower, upper, conv.bias, logdiag), args.reps)
                r_ci = timed(lambda: ref_conv_inverse(x, inv_perm, lower, upper, conv.bias, logdiag), args.reps)
                sub = x[:4]
                got = conv(sub)[0].double()
                w64 = (lower.double() @ upper.double())[:, inv_perm]
                want = torch.einsum("ik,bkhw->bihw", w64, sub.double()) + conv.bias.double().view(1, c, 1, 1)
                err = (got - want).abs().max().item()
            for what, t, r in (("squeeze_forward", t_sf, r_sf), ("squeeze_inverse", t_si, r_si),
                               ("conv1x1_forward", t_cf, r_cf), ("conv1x1_inverse", t_ci, r_ci)):
                row = {"layer": what, "batch": n, "c": c, "hw": s, "hip_ms": round(t, 4), "torch_ms": round(r, 4),
                       "speedup": round(r / t, 2), "bytes": elem_bytes,
                       "hbm_share": round(elem_bytes / (t * 1e-3) / HBM, 3)}
                if what == "conv1x1_forward":
                    row["max_err_vs_f64"] = err
                rows.append(row)
            print("[bench_image] %dx%d c=%d done" % (s, s, c), file=sys.stderr, flush=True)

    # one whole two-level multiscale flow (tests/golden/make_image_golden.py): log_prob and sample
    from make_image_golden import build_image_flow

    class Lib:
        pass

    Lib.transforms, Lib.nets, Lib.utils, Lib.flows, Lib.distributions = transforms, nets, utils, flows, distributions
    torch.manual_seed(0)
    flow = build_image_flow(Lib).to(dev)
    xb = torch.randn(args.flow_batch, 3, 16, 16, device=dev)
    with torch.no_grad():
        flow.train()
        flow.log_prob(xb)          # ActNorm initialisation
        flow.eval()
        t_lp = timed(lambda: flow.log_prob(xb), args.reps)
        noise = torch.randn(args.flow_batch, 768, device=dev)
        t_smp = timed(lambda: flow._transform.inverse(noise), args.reps)
    rows.append({"layer": "multiscale_flow_log_prob", "batch": args.flow_batch, "shape": [3, 16, 16],
                 "ms": round(t_lp, 4)})
    rows.append({"layer": "multiscale_flow_sample", "batch": args.flow_batch, "shape": [3, 16, 16],
                 "ms": round(t_smp, 4)})
    print(json.dumps({"bench": "image_layers", "device": torch.cuda.get_device_name(0), "rows": rows}))


if __name__ == "__main__":
    main()
