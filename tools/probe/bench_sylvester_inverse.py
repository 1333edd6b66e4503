"""SylvesterTransform.inverse: the back-substitution kernel (fc_sylvester_inverse) alone, the whole ``inverse`` call (the
two applications of Q around it), the forward direction on the same device beside them, and the torch composition of the
same algorithm on the same inputs.

    python tools/probe/bench_sylvester_inverse.py [--out result.json] [--repeats 9] [--calls 10]

Cases: D = 128 / M = 32 at N = 2^18 and N = 4096, D = 16 / M = 8 at N = 2^16; parameters N(0, 0.15) (0.4 at D = 16), inputs
the forward images of standard-normal points.  Warm-up, then ``repeats`` rounds alternating the routes, each round timing
``calls`` back-to-back calls between two device events (the composition: one call per round); reported are the median per
call and the spread (max - min over the rounds).  The kernels alone come from ``ops.KernelTimer`` over the same rounds.  The
evaluations of the scalar residual per solve (mean, max) come from a float32 host replay of the kernel's stopping rule on
the first 4096 rows.  The kernel's result is checked at the timed size: float64 forward of its z against y.  A device is
required."""
import argparse
import copy
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from flowconductor_amd import _hip, ops, options, transforms as T  # noqa: E402

CASES = ((128, 32, 1 << 18), (128, 32, 4096), (16, 8, 1 << 16))
MAX_EVALUATIONS = 16


def timed(fn, calls):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(calls):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / calls


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "spread_ms": max(ms) - min(ms),
            "samples": len(ms)}


def replay_evaluations(t, y):
    """Evaluations of the residual per scalar solve (float32, CPU): the kernel's stopping rule, element by element."""
    t = t.cpu()
    with torch.no_grad():
        q, r1, r2, bias = t.Q_orth.q_vectors, t._create_R1(), t._create_R2(), t.bias
        c = y.cpu()
        for qv in q.flip(0):
            c = c - (c @ qv).unsqueeze(-1) * ((2.0 / (qv @ qv)) * qv)
        v, th = torch.zeros_like(c), torch.zeros_like(c)
        counts = torch.zeros_like(c)
        for j in range(c.shape[1] - 1, -1, -1):
            s = bias[j] + v[:, j + 1:] @ r1[j, j + 1:]
            tt = c[:, j] - th[:, j + 1:] @ r2[j, j + 1:]
            a, b = r1[j, j], r2[j, j]
            tol = 2.0 ** -22 * (tt.abs() + b.abs())
            lo, hi, x = tt - b.abs(), tt + b.abs(), tt.clone()
            active = torch.ones_like(tt, dtype=torch.bool)
            for it in range(MAX_EVALUATIONS):
                counts[:, j] += active
                h = torch.tanh(a * x + s)
                g = (x + b * h) - tt
                active = active & (g.abs() > tol)
                if it == MAX_EVALUATIONS - 1 or not bool(active.any()):
                    break
                lo = torch.where(active & (g < 0), x, lo)
                hi = torch.where(active & (g > 0), x, hi)
                xn = x - g / (1 + a * b * (1 - h * h))
                xn = torch.where((xn >= lo) & (xn <= hi), xn, 0.5 * (lo + hi))
                active = active & (xn != x)
                x = torch.where(active, xn, x)
            v[:, j], th[:, j] = x, h
    return {"mean": float(counts.mean()), "max": int(counts.max())}


def forward64(t, z):
    t64 = copy.deepcopy(t).cpu().double()
    with torch.no_grad():
        q, r1, r2, bias = t64.Q_orth.q_vectors, t64._create_R1(), t64._create_R2(), t64.bias
        x = z.cpu().double()
        c = x
        for qv in q.flip(0):
            c = c - (c @ qv).unsqueeze(-1) * ((2.0 / (qv @ qv)) * qv)
        out = torch.tanh(c @ r1.T + bias) @ r2.T
        for qv in q:
            out = out - (out @ qv).unsqueeze(-1) * ((2.0 / (qv @ qv)) * qv)
        return x + out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--calls", type=int, default=10)
    args = ap.parse_args()
    if args.repeats < 5:
        ap.error("at least 5 repeats")
    if not torch.cuda.is_available():
        raise SystemExit("bench_sylvester_inverse: no HIP device")
    dev = torch.device("cuda:0")
    result = {"library": _hip.library_info(), "device": torch.cuda.get_device_name(0), "repeats": args.repeats,
              "calls_per_round": args.calls, "cases": []}
    for d, m, n in CASES:
        torch.manual_seed(d + n)
        t = T.SylvesterTransform(d, num_householder=m, device="cpu").eval()
        with torch.no_grad():
            for prm in t.parameters():
                prm.copy_(torch.randn(prm.shape) * (0.15 if d > 16 else 0.4))
        t = t.to(dev)
        x = torch.randn(n, d, device=dev)
        with torch.no_grad():
            y, _ = t(x)
            z, _ = t.inverse(y)
        check = 4096
        entry = {"features": d, "num_householder": m, "rows": n,
                 "y_space_residual_vs_float64": float((forward64(t, z[:check]) - y[:check].cpu().double()).abs().max()),
                 "evaluations_per_solve": replay_evaluations(copy.deepcopy(t), y[:check])}
        forward_kernel = "fc_sylvester_mm" if ops.sylvester_mm_supported(n, d) else "fc_sylvester"
        with torch.no_grad():
            routes = {"inverse": lambda: t.inverse(y), "forward": lambda: t(x)}
            for fn in routes.values():
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            times = {name: [] for name in routes}
            with ops.KernelTimer("fc_sylvester_inverse") as k_inv, ops.KernelTimer(forward_kernel) as k_fwd:
                for _ in range(args.repeats):
                    for name, fn in routes.items():
                        times[name].append(timed(fn, args.calls))
            torch.cuda.synchronize()
            entry["inverse_call"], entry["forward_call"] = summary(times["inverse"]), summary(times["forward"])
            entry["fc_sylvester_inverse"] = summary(k_inv.durations_ms())
            entry[forward_kernel] = summary(k_fwd.durations_ms())
            if forward_kernel != "fc_sylvester":            # the row-per-wavefront forward beside the matrix-core one
                with options.override(sylvester_mm=False), ops.KernelTimer("fc_sylvester") as k_row:
                    for _ in range(3 + args.repeats):
                        t(x)
                torch.cuda.synchronize()
                entry["fc_sylvester"] = summary(k_row.durations_ms()[3:])
            t._inverse_composition(y)
            torch.cuda.synchronize()
            entry["torch_composition"] = summary([timed(lambda: t._inverse_composition(y), 1) for _ in range(args.repeats)])
        result["cases"].append(entry)
        print("D %d M %d N %d: fc_sylvester_inverse %.3f ms (spread %.3f) | inverse call %.3f ms (spread %.3f) | %s %.3f ms | "
              "forward call %.3f ms | torch composition %.1f ms | evaluations per solve mean %.2f max %d | y residual %.3g"
              % (d, m, n, entry["fc_sylvester_inverse"]["median_ms"], entry["fc_sylvester_inverse"]["spread_ms"],
                 entry["inverse_call"]["median_ms"], entry["inverse_call"]["spread_ms"], forward_kernel,
                 entry[forward_kernel]["median_ms"], entry["forward_call"]["median_ms"],
                 entry["torch_composition"]["median_ms"], entry["evaluations_per_solve"]["mean"],
                 entry["evaluations_per_solve"]["max"], entry["y_space_residual_vs_float64"]), flush=True)
        if "fc_sylvester" in entry and forward_kernel != "fc_sylvester":
            print("    fc_sylvester (row per wavefront) %.3f ms" % entry["fc_sylvester"]["median_ms"], flush=True)
        del x, y, z
        torch.cuda.empty_cache()
    print(json.dumps(result))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
