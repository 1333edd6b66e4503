"""The fused Householder-diagonal-Householder map (fc_hdh_linear / fc_hdh_linear_backward, what SVDLinear runs) against the
same map composed from the ops that existed before it, each with its own autograd node: householder_autograd,
pointwise_affine_autograd, householder_autograd, + bias.  The composition's kernels are untouched by the fused entry, so it
is the earlier code path, not the new code compared with itself.

    python tools/probe/bench_svd_linear.py [--out result.json] [--repeats 9] [--calls 10]

Shapes: D = 64 with K = 8 and K = 64 reflections per sequence, D = 128 with K = 32; N = 2^20 rows forward (no grad),
N = 2^19 rows for a training step (forward + backward, gradients to the input and every parameter).  Per shape and
direction: warm-up, then ``repeats`` rounds alternating the two routes, each round timing ``calls`` back-to-back calls
between two device events; reported are the median per call, the spread (max - min over the rounds) and the ratio of the
medians.  ``faster`` is true when the composition's median exceeds the fused median by more than the larger of the two
spreads.  Training also records the peak allocated memory of one step above the resident operands.  The two routes'
outputs are compared at the timed size.  A device is required."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from flowconductor_amd import _hip, ops  # noqa: E402

SHAPES = [(64, 8), (64, 64), (128, 32)]
ROWS_FORWARD, ROWS_TRAIN = 1 << 20, 1 << 19


def fused(x, q2, q1, diagonal, bias):
    return ops.hdh_linear_autograd(x, q2, q1, diagonal, None, bias)


def composition(x, q2, q1, diagonal, bias):
    out, _ = ops.householder_autograd(x, q2)
    out = ops.pointwise_affine_autograd(out, diagonal, torch.zeros(1, device=x.device))
    out, _ = ops.householder_autograd(out, q1)
    return out + bias


def timed(fn, calls):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(calls):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / calls


def compare(routes, repeats, calls):
    """{name: {"median_ms", "min_ms", "max_ms", "spread_ms"}} with the routes alternated round by round."""
    for fn in routes.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in routes}
    for _ in range(repeats):
        for name, fn in routes.items():
            times[name].append(timed(fn, calls))
    return {name: {"median_ms": statistics.median(t), "min_ms": min(t), "max_ms": max(t), "spread_ms": max(t) - min(t)}
            for name, t in times.items()}


def verdict(stats):
    gap = stats["composition"]["median_ms"] - stats["fused"]["median_ms"]
    stats["ratio_composition_over_fused"] = stats["composition"]["median_ms"] / stats["fused"]["median_ms"]
    stats["faster"] = gap > max(stats["fused"]["spread_ms"], stats["composition"]["spread_ms"])
    return stats


def peak_of(step):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    step()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - before


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--calls", type=int, default=10)
    args = ap.parse_args()
    if args.repeats < 5:
        ap.error("at least 5 repeats")
    if not torch.cuda.is_available():
        raise SystemExit("bench_svd_linear: no HIP device")
    dev = torch.device("cuda:0")
    result = {"library": _hip.library_info(), "device": torch.cuda.get_device_name(0), "repeats": args.repeats,
              "calls_per_round": args.calls, "rows_forward": ROWS_FORWARD, "rows_train": ROWS_TRAIN, "shapes": []}
    for d, k in SHAPES:
        torch.manual_seed(d + k)
        params = [torch.randn(k, d, device=dev), torch.randn(k, d, device=dev), torch.exp(0.3 * torch.randn(d, device=dev)),
                  torch.randn(d, device=dev)]
        entry = {"features": d, "num_householder": k}
        x = torch.randn(ROWS_FORWARD, d, device=dev)
        with torch.no_grad():
            y_f, y_c = fused(x, *params), composition(x, *params)
            entry["forward_max_abs_difference"] = float((y_f - y_c).abs().max())
            entry["forward_max_abs_value"] = float(y_c.abs().max())
            del y_f, y_c
            entry["forward"] = verdict(compare({"fused": lambda: fused(x, *params),
                                                "composition": lambda: composition(x, *params)}, args.repeats, args.calls))
        del x
        x = torch.randn(ROWS_TRAIN, d, device=dev, requires_grad=True)
        gy = torch.randn(ROWS_TRAIN, d, device=dev)
        leaves = [p.clone().requires_grad_(True) for p in params]

        def step(route):
            for t in [x] + leaves:
                t.grad = None
            route(x, *leaves).backward(gy)

        step(fused)
        grads_f = [t.grad.clone() for t in [x] + leaves]
        step(composition)
        entry["train_max_rel_gradient_difference"] = max(
            float((a - t.grad).abs().max() / t.grad.abs().max().clamp_min(1e-30)) for a, t in zip(grads_f, [x] + leaves))
        del grads_f
        entry["train"] = verdict(compare({"fused": lambda: step(fused), "composition": lambda: step(composition)},
                                         args.repeats, args.calls))
        entry["train"]["fused"]["peak_step_bytes"] = peak_of(lambda: step(fused))
        entry["train"]["composition"]["peak_step_bytes"] = peak_of(lambda: step(composition))
        entry["train"]["less_memory"] = entry["train"]["fused"]["peak_step_bytes"] < entry["train"]["composition"]["peak_step_bytes"]
        del x, gy, leaves
        torch.cuda.empty_cache()
        result["shapes"].append(entry)
        for which in ("forward", "train"):
            s = entry[which]
            print("D=%d K=%d %-7s fused %.3f ms (spread %.3f) composition %.3f ms (spread %.3f) ratio %.2f faster=%s"
                  % (d, k, which, s["fused"]["median_ms"], s["fused"]["spread_ms"], s["composition"]["median_ms"],
                     s["composition"]["spread_ms"], s["ratio_composition_over_fused"], s["faster"]), flush=True)
        print("D=%d K=%d train peak bytes fused %d composition %d | forward diff %.3g of %.3g | gradient rel diff %.3g"
              % (d, k, entry["train"]["fused"]["peak_step_bytes"], entry["train"]["composition"]["peak_step_bytes"],
                 entry["forward_max_abs_difference"], entry["forward_max_abs_value"],
                 entry["train_max_rel_gradient_difference"]), flush=True)
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
