"""The batch-statistics kernels (fc_batchnorm_train, fc_batchnorm_train_backward, fc_column_sums) against the torch
expressions they replace, both routes in one process (``options.override(batch_statistics_kernels=...)``).

    python tools/probe/bench_batch_statistics.py [--out result.json] [--repeats 9] [--calls 10]

Timed, forward + backward of ``(y * gy).sum() + logabsdet.sum()`` (the flows: of ``-log_prob.mean()``):

    batchnorm   a stand-alone training-mode BatchNorm at (2^20, 64) and (4096, 2)
    maf         a 5-layer MaskedAutoregressiveFlow with batch_norm_between_layers at D = 16, N = 2^16 and D = 2, N = 4096
    actnorm     ActNorm at (2^20, 64)

Every case is warmed up, then ``repeats`` rounds alternate the two routes, each round timing ``calls`` back-to-back steps
between two device events with a synchronise; reported are the median per step, the spread (max - min over the rounds), the
ratio of the medians and how often a step enters each of the three launches (``KernelTimer``).  For the (2^20, 64) rows the
launches are also timed one by one and set against the HBM roof: the forward must move x twice and y once (12 B per element),
the BatchNorm backward gy and x twice each and gx once (20 B), ActNorm's column sums gy and x once (8 B).  All of these
kernels are bound by HBM bandwidth (a handful of flops per byte).  A device is required."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from flowconductor_amd import _hip, flows, ops, options, transforms  # noqa: E402

LAUNCHES = ("fc_batchnorm_train", "fc_batchnorm_train_backward", "fc_column_sums")
HBM_PEAK_SPEC, HBM_PEAK_COPY = 8.0e12, 6.29e12        # bytes/s: data sheet, and a float4 copy measured on this part


def timed(fn, calls):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(calls):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / calls


def routed(step, kernels):
    def run():
        with options.override(batch_statistics_kernels=kernels):
            step()
    return run


def launch_counts(step):
    timers = [ops.KernelTimer(name) for name in LAUNCHES]
    for t in timers:
        t.__enter__()
    try:
        step()
    finally:
        for t in timers:
            t.__exit__(None, None, None)
    torch.cuda.synchronize()
    return {t.name: len(t.pairs) for t in timers}, {t.name: t.durations_ms() for t in timers}


def compare(step, repeats, calls):
    routes = {"hip": routed(step, True), "torch": routed(step, False)}
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
    stats["launches_per_step"] = {name: launch_counts(fn)[0] for name, fn in routes.items()}
    return stats


def kernel_roof(step, repeats, bytes_per_launch):
    """Median duration of each named launch inside ``step`` and the share of the HBM roof its algorithmic bytes reach."""
    run = routed(step, True)
    samples = {name: [] for name in bytes_per_launch}
    for _ in range(repeats):
        durations = launch_counts(run)[1]
        for name in samples:
            samples[name] += durations[name]
    out = {}
    for name, nbytes in bytes_per_launch.items():
        ms = statistics.median(samples[name])
        rate = nbytes / (ms * 1e-3)
        out[name] = {"median_ms": ms, "spread_ms": max(samples[name]) - min(samples[name]), "bytes": nbytes,
                     "tb_per_s": rate / 1e12, "of_spec_peak": rate / HBM_PEAK_SPEC, "of_copy_peak": rate / HBM_PEAK_COPY,
                     "bound_by": "HBM bandwidth"}
    return out


def layer_step(layer, n, d, dev):
    x = torch.randn(n, d, device=dev, requires_grad=True)
    gy = torch.randn(n, d, device=dev)

    def step():
        x.grad = None
        layer.zero_grad(set_to_none=True)
        y, lad = layer(x)
        ((y * gy).sum() + lad.sum()).backward()
    return step


def maf_step(n, d, dev):
    torch.manual_seed(3)
    flow = flows.MaskedAutoregressiveFlow(features=d, hidden_features=64, num_layers=5, num_blocks_per_layer=2,
                                          batch_norm_between_layers=True).to(dev).train()
    x = torch.randn(n, d, device=dev)

    def step():
        flow.zero_grad(set_to_none=True)
        (-flow.log_prob(x).mean()).backward()
    return step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--calls", type=int, default=10)
    args = ap.parse_args()
    if args.repeats < 5:
        ap.error("at least 5 repeats")
    if not torch.cuda.is_available():
        raise SystemExit("bench_batch_statistics: no HIP device")
    dev = torch.device("cuda:0")
    result = {"library": _hip.library_info(), "device": torch.cuda.get_device_name(0), "repeats": args.repeats,
              "calls_per_round": args.calls, "cases": {}}
    torch.manual_seed(11)
    big = (1 << 20, 64)
    cases = []
    for n, d in (big, (4096, 2)):
        cases.append(("batchnorm %dx%d" % (n, d), layer_step(transforms.BatchNorm(d).to(dev).train(), n, d, dev),
                      {"fc_batchnorm_train": 12 * n * d, "fc_batchnorm_train_backward": 20 * n * d} if (n, d) == big else None))
    for n, d in ((1 << 16, 16), (4096, 2)):
        cases.append(("maf5+bn %dx%d" % (n, d), maf_step(n, d, dev), None))
    act = transforms.ActNorm(big[1]).to(dev).train()
    with torch.no_grad():
        act(torch.randn(*big, device=dev))
    cases.append(("actnorm %dx%d" % big, layer_step(act, *big, dev), {"fc_column_sums": 8 * big[0] * big[1]}))
    for name, step, roof in cases:
        entry = compare(step, args.repeats, args.calls)
        if roof:
            entry["kernels"] = kernel_roof(step, args.repeats, roof)
        result["cases"][name] = entry
        print("%-22s hip %.4f ms (spread %.4f) torch %.4f ms (spread %.4f) ratio %.2f  launches/step %s"
              % (name, entry["hip"]["median_ms"], entry["hip"]["spread_ms"], entry["torch"]["median_ms"],
                 entry["torch"]["spread_ms"], entry["ratio_torch_over_hip"],
                 {k: v for k, v in entry["launches_per_step"]["hip"].items() if v}), flush=True)
        for kernel, k in entry.get("kernels", {}).items():
            print("    %-28s %.4f ms (spread %.4f)  %.2f TB/s = %.0f %% of the %.1f TB/s peak, %.0f %% of a copy"
                  % (kernel, k["median_ms"], k["spread_ms"], k["tb_per_s"], 100 * k["of_spec_peak"], HBM_PEAK_SPEC / 1e12,
                     100 * k["of_copy_peak"]), flush=True)
        torch.cuda.empty_cache()
    print(json.dumps(result))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
