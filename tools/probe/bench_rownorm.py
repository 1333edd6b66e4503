"""The row-norm kernels (fc_radial, fc_unit_vector and their backward kernels) against the same maps written in torch ops on
the device, following the reference's op sequence (no_analytic_inv/planar.py:199-211, unitvector.py:18-53).

    python tools/probe/bench_rownorm.py [--out result.json] [--repeats 9] [--calls 10]

N = 2^20 rows, D = 64: the two forward kernels (no grad) and one training step of each (forward + backward of
``(y * gy).sum() + lad.sum()``, gradients to the input and, for radial, to alpha / beta / z_0).  Warm-up, then ``repeats``
rounds alternating the two routes, each round timing ``calls`` back-to-back calls between two device events; reported are the
median per call, the spread (max - min over the rounds), the ratio of the medians and, for the forward kernels, the HBM
traffic they must move (row in, row out, 4 bytes of logabsdet per sample) per second.  The two routes' outputs are compared
at the timed size.  A device is required."""
import argparse
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from flowconductor_amd import _hip, ops  # noqa: E402

ROWS, FEATURES = 1 << 20, 64


def radial_torch(x, z_0, alpha, beta, features):
    b = torch.log(1 + torch.exp(beta)) - torch.abs(alpha)
    dz = x - z_0
    r = torch.linalg.vector_norm(dz, dim=[1], keepdim=True)
    h = b / (torch.abs(alpha) + r)
    h_ = -b * r / (torch.abs(alpha) + r) ** 2
    return x + h * dz, ((features - 1) * torch.log(1 + h) + torch.log(1 + h + h_)).reshape(-1)


def radial_hip(x, z_0, alpha, beta, features):
    a = torch.abs(alpha)
    return ops.radial_autograd(x, z_0.reshape(-1), a, torch.log(1 + torch.exp(beta)) - a)


def unit_torch(x, features):
    s = torch.sum(x ** 2, dim=-1, keepdim=True)
    y = torch.concatenate([2 * x, s - 1], dim=-1) / (s + 1)
    return y, features * (math.log(2.0) - torch.log1p(torch.sum(x ** 2, dim=-1, keepdim=True).squeeze()))


def unit_hip(x, features):
    return ops.unit_vector_autograd(x, features)


def timed(fn, calls):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(calls):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / calls


def compare(routes, repeats, calls):
    for fn in routes.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in routes}
    for _ in range(repeats):
        for name, fn in routes.items():
            times[name].append(timed(fn, calls))
    stats = {name: {"median_ms": statistics.median(t), "min_ms": min(t), "max_ms": max(t), "spread_ms": max(t) - min(t)}
             for name, t in times.items()}
    stats["ratio_torch_over_hip"] = stats["torch"]["median_ms"] / stats["hip"]["median_ms"]
    return stats


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--calls", type=int, default=10)
    args = ap.parse_args()
    if args.repeats < 5:
        ap.error("at least 5 repeats")
    if not torch.cuda.is_available():
        raise SystemExit("bench_rownorm: no HIP device")
    dev = torch.device("cuda:0")
    n, d = ROWS, FEATURES
    result = {"library": _hip.library_info(), "device": torch.cuda.get_device_name(0), "repeats": args.repeats,
              "calls_per_round": args.calls, "rows": n, "features": d, "cases": {}}
    torch.manual_seed(7)
    x = torch.randn(n, d, device=dev)
    z_0, alpha, beta = torch.randn(1, d, device=dev), torch.tensor([0.3], device=dev), torch.tensor([-0.8], device=dev)
    maps = {"radial": (lambda route, inp, leaves: route(inp, *leaves, d), (radial_hip, radial_torch), [z_0, alpha, beta],
                       2 * n * d * 4 + n * 4),
            "unit_vector": (lambda route, inp, leaves: route(inp, d), (unit_hip, unit_torch), [], n * (2 * d + 1) * 4 + n * 4)}
    for name, (call, (hip, ref), params, forward_bytes) in maps.items():
        entry = {}
        with torch.no_grad():
            (y_h, lad_h), (y_t, lad_t) = call(hip, x, params), call(ref, x, params)
            entry["forward_max_abs_difference"] = max(float((y_h - y_t).abs().max()), float((lad_h - lad_t).abs().max()))
            del y_h, lad_h, y_t, lad_t
            entry["forward"] = compare({"hip": lambda: call(hip, x, params), "torch": lambda: call(ref, x, params)},
                                       args.repeats, args.calls)
        entry["forward"]["hip_bytes"] = forward_bytes
        entry["forward"]["hip_gb_per_s"] = forward_bytes / (entry["forward"]["hip"]["median_ms"] * 1e-3) / 1e9
        xg = x.clone().requires_grad_(True)
        leaves = [p.clone().requires_grad_(True) for p in params]
        gy = torch.randn(n, d + (1 if name == "unit_vector" else 0), device=dev)

        def step(route):
            for t in [xg] + leaves:
                t.grad = None
            y, lad = call(route, xg, leaves)
            ((y * gy).sum() + lad.sum()).backward()

        step(hip)
        grads = [t.grad.clone() for t in [xg] + leaves]
        step(ref)
        entry["train_max_rel_gradient_difference"] = max(
            float((g - t.grad).abs().max() / t.grad.abs().max().clamp_min(1e-30)) for g, t in zip(grads, [xg] + leaves))
        del grads
        entry["train"] = compare({"hip": lambda: step(hip), "torch": lambda: step(ref)}, args.repeats, args.calls)
        del xg, leaves, gy
        torch.cuda.empty_cache()
        result["cases"][name] = entry
        for which in ("forward", "train"):
            s = entry[which]
            print("%-11s %-7s hip %.3f ms (spread %.3f) torch %.3f ms (spread %.3f) ratio %.2f%s"
                  % (name, which, s["hip"]["median_ms"], s["hip"]["spread_ms"], s["torch"]["median_ms"], s["torch"]["spread_ms"],
                     s["ratio_torch_over_hip"], "  %.0f GB/s" % s["hip_gb_per_s"] if which == "forward" else ""), flush=True)
        print("%-11s forward diff %.3g | gradient rel diff %.3g"
              % (name, entry["forward_max_abs_difference"], entry["train_max_rel_gradient_difference"]), flush=True)
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
