"""Time MADEMoG's kernel routes against the torch composition of the same build.

    python tools/bench_mog.py [--out FILE.json] [--repeats R]

An sbi-sized estimator: D = 8, C = 10 components, hidden 50, 2 blocks, a 16-feature context, at N = 2^16 and 2^20 rows.
Per size (i) ``log_prob`` (inference), (ii) ``log_prob(...).sum().backward()`` and (iii) the sampler on fixed noise, each on
the kernel route (fc_mog_log_prob / fc_mog_log_prob_backward / fc_made_mog_sample_context) and as the torch composition
(``log_prob_composition``, torch autograd through it, ``_sample_host_loop``), with the largest difference between the two
routes' results.  Every path is warmed up first; the routes are alternated within one process, three rounds, device
events around each call; each round's median and the spread between rounds are reported.  Prints one JSON document."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from flowconductor_amd import _hip, distributions  # noqa: E402

DEV = torch.device("cuda:0")
ROUNDS = 3
D, C, HIDDEN, BLOCKS, CONTEXT = 8, 10, 50, 2, 16


def once(fn):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end)


def alternate(paths, repeats):
    for fn in paths.values():
        fn()
    torch.cuda.synchronize()
    rounds = {name: [] for name in paths}
    for _ in range(ROUNDS):
        for name, fn in paths.items():
            rounds[name].append(statistics.median(once(fn) for _ in range(repeats)))
    return {name: {"ms": statistics.median(r), "rounds": r, "spread": (max(r) - min(r)) / statistics.median(r)}
            for name, r in rounds.items()}


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--out")
    parser.add_argument("--repeats", type=int, default=9)
    args = parser.parse_args()
    result = {"date": time.strftime("%Y-%m-%d"), "device": torch.cuda.get_device_name(0), "library": _hip.library_info(),
              "model": {"features": D, "components": C, "hidden": HIDDEN, "blocks": BLOCKS, "context": CONTEXT},
              "repeats": args.repeats, "rounds": ROUNDS, "cases": []}
    torch.manual_seed(0)
    dist = distributions.MADEMoG(D, HIDDEN, CONTEXT, num_blocks=BLOCKS, num_mixture_components=C,
                                 custom_initialization=True).to(DEV).eval()
    made = dist._made
    for n in (2 ** 16, 2 ** 20):
        x = torch.randn(n, D, device=DEV)
        c = torch.randn(n, CONTEXT, device=DEV)
        normal, uniform = torch.randn(n, D, device=DEV), torch.rand(n, D, device=DEV)

        def no_grad(fn):
            def run():
                with torch.no_grad():
                    return fn()
            return run

        def backward(fn):
            def run():
                made.zero_grad(set_to_none=True)
                fn().sum().backward()
            return run

        with torch.no_grad():
            lp_kernel, lp_torch = made.log_prob(x, c), made.log_prob_composition(x, c)
            s_kernel, sl_kernel = made._sample_device_loop(normal, uniform, c)
            s_torch, sl_torch = made._sample_host_loop(normal, uniform, c)
        assert made._sample_kernel_ok(normal, c)
        backward(lambda: made.log_prob(x, c))()
        g_kernel = made.final_layer.weight.grad.clone()
        backward(lambda: made.log_prob_composition(x, c))()
        g_torch = made.final_layer.weight.grad.clone()
        same = (s_kernel - s_torch).abs().amax(dim=1) < 1e-3        # (rows where float32 rounding flipped no component)
        entry = {"n": n, "max_abs_dlog_prob": float((lp_kernel - lp_torch).abs().max()),
                 "max_rel_dgrad_final_weight": float((g_kernel - g_torch).abs().max() / g_torch.abs().max()),
                 "sample_rows_with_the_same_components": float(same.float().mean()),
                 "max_abs_dsample_on_those": float((s_kernel - s_torch)[same].abs().max()),
                 "max_abs_dsample_log_prob_on_those": float((sl_kernel - sl_torch)[same].abs().max())}
        timing = alternate({
            "log_prob_kernel": no_grad(lambda: made.log_prob(x, c)),
            "log_prob_torch": no_grad(lambda: made.log_prob_composition(x, c)),
            "log_prob_backward_kernel": backward(lambda: made.log_prob(x, c)),
            "log_prob_backward_torch": backward(lambda: made.log_prob_composition(x, c)),
            "sample_kernel": no_grad(lambda: made._sample_device_loop(normal, uniform, c)),
            "sample_torch": no_grad(lambda: made._sample_host_loop(normal, uniform, c)),
        }, args.repeats)
        for what in ("log_prob", "log_prob_backward", "sample"):
            entry[what + "_kernel_ms"] = timing[what + "_kernel"]["ms"]
            entry[what + "_torch_ms"] = timing[what + "_torch"]["ms"]
            entry[what + "_speedup"] = timing[what + "_torch"]["ms"] / timing[what + "_kernel"]["ms"]
        print(json.dumps(entry), file=sys.stderr, flush=True)
        entry["rounds"] = timing
        result["cases"].append(entry)
    text = json.dumps(result, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
