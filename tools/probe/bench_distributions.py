"""The Bernoulli likelihood kernels (fc_bernoulli_log_prob and its backward) against the reference's torch expression
(distributions/discrete.py:54-55) on the same device, in one process.

    python tools/probe/bench_distributions.py [--out result.json] [--repeats 9] [--calls 10]

Two shapes: N = 2^18 rows of D = 784 (one wave per row) and N = 2^20 rows of D = 16 (four lanes per row).  Timed are the
forward pass without a graph and one training step (forward + backward of ``(log_prob * g).sum()`` with the gradient going to
the logits, as in a decoder likelihood).  Warm-up, then ``repeats`` rounds alternating the two routes, each round timing
``calls`` back-to-back calls between two device events; reported are the median per call, the spread (max - min over the
rounds), the ratio of the medians, and for the HIP route the algorithmic HBM traffic per second and its share of the 8 TB/s
peak: 8 N D + 4 N bytes forward; the same read again plus 4 N D written backward.  The two routes' outputs are compared at the
timed size.  Also timed, forward only: the sampler and the box density against their expressions.  A device is required."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from flowconductor_amd import _hip, ops  # noqa: E402
from flowconductor_amd.ops import discrete  # noqa: E402

SHAPES = [(1 << 18, 784), (1 << 20, 16)]
HBM_PEAK = 8.0e12


def timed(fn, calls):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(calls):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / calls


def compare(routes, repeats, calls, hip_bytes):
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
    stats["hip_bytes"] = hip_bytes
    stats["hip_tb_per_s"] = hip_bytes / (stats["hip"]["median_ms"] * 1e-3) / 1e12
    stats["hip_share_of_hbm_peak"] = hip_bytes / (stats["hip"]["median_ms"] * 1e-3) / HBM_PEAK
    return stats


def report(label, which, s):
    print("%-22s %-8s hip %.3f ms (spread %.3f) torch %.3f ms (spread %.3f) ratio %.2f  %.2f TB/s = %.2f of the HBM peak"
          % (label, which, s["hip"]["median_ms"], s["hip"]["spread_ms"], s["torch"]["median_ms"], s["torch"]["spread_ms"],
             s["ratio_torch_over_hip"], s["hip_tb_per_s"], s["hip_share_of_hbm_peak"]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--calls", type=int, default=10)
    args = ap.parse_args()
    if args.repeats < 5:
        ap.error("at least 5 repeats")
    if not torch.cuda.is_available():
        raise SystemExit("bench_distributions: no HIP device")
    dev = torch.device("cuda:0")
    result = {"library": _hip.library_info(), "device": torch.cuda.get_device_name(0), "repeats": args.repeats,
              "calls_per_round": args.calls, "cases": {}}
    for n, d in SHAPES:
        label = "bernoulli %dx%d" % (n, d)
        entry = {"rows": n, "features": d}
        torch.manual_seed(7)
        x = (torch.rand(n, d, device=dev) < 0.5).float()
        logits = torch.randn(n, d, device=dev) * 4.0
        g = torch.randn(n, device=dev)
        with torch.no_grad():
            hip, ref = ops.bernoulli_log_prob(x, logits), discrete._bernoulli_log_prob_torch(x, logits, None)
            entry["forward_max_abs_difference"] = float((hip - ref).abs().max())
            entry["forward_max_abs_value"] = float(ref.abs().max())
            del hip, ref
            entry["forward"] = compare({"hip": lambda: ops.bernoulli_log_prob(x, logits),
                                        "torch": lambda: discrete._bernoulli_log_prob_torch(x, logits, None)},
                                       args.repeats, args.calls, 8 * n * d + 4 * n)
        leaf = logits.clone().requires_grad_(True)

        def step(route):
            leaf.grad = None
            (route(x, leaf) * g).sum().backward()

        step(ops.bernoulli_log_prob)
        grad = leaf.grad.clone()
        step(lambda a, b: discrete._bernoulli_log_prob_torch(a, b, None))
        entry["train_max_abs_gradient_difference"] = float((grad - leaf.grad).abs().max())
        del grad
        entry["train"] = compare({"hip": lambda: step(ops.bernoulli_log_prob),
                                  "torch": lambda: step(lambda a, b: discrete._bernoulli_log_prob_torch(a, b, None))},
                                 args.repeats, args.calls, 2 * (8 * n * d + 4 * n) + 4 * n * d)
        leaf.grad = None
        for which in ("forward", "train"):
            report(label, which, entry[which])
        print("%-22s forward diff %.3g (max |value| %.3g) | gradient diff %.3g"
              % (label, entry["forward_max_abs_difference"], entry["forward_max_abs_value"],
                 entry["train_max_abs_gradient_difference"]), flush=True)
        with torch.no_grad():
            # the sampler: S = 4 draws per context row, against sigmoid + repeat_interleave + compare + cast
            draws = 4
            noise = torch.rand(n, d, device=dev)
            few = logits[: n // draws]
            entry["sample"] = compare(
                {"hip": lambda: ops.bernoulli_sample(few, noise, draws),
                 "torch": lambda: (noise < torch.sigmoid(few).repeat_interleave(draws, dim=0)).float()},
                args.repeats, args.calls, 8 * n * d + 4 * (n // draws) * d)
            report(label, "sample", entry["sample"])
            low, high = -torch.rand(d, device=dev) - 3.0, torch.rand(d, device=dev) + 3.0
            entry["box"] = compare({"hip": lambda: ops.box_log_prob(logits, low, high),
                                    "torch": lambda: discrete._box_log_prob_torch(logits, low, high)},
                                   args.repeats, args.calls, 4 * n * d + 4 * n)
            report(label, "box", entry["box"])
            del noise, few
        del x, logits, g, leaf
        torch.cuda.empty_cache()
        result["cases"]["%dx%d" % (n, d)] = entry
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
