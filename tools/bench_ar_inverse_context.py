"""Time the conditional device loop (fc_made_inverse_context) against the host loop of the same build and against the
unconditional device loop of the same layer built without context features.

    python tools/bench_ar_inverse_context.py [--out FILE.json] [--repeats R]

Layers: MAF and RQ-AR (K = 8, linear tails), hidden 64, two blocks, a 16-feature context, at (D, N) = (64, 2^16),
(16, 2^18), (8, 2^20); flows: 5 x [MAF(D 8, hidden 50, 2 blocks, context 10), reverse permutation], ``flow.sample`` of
10 000 draws for one context row and of 1 000 draws for each of 64 rows.  Per case (i) the conditional device loop, (ii) the
host loop (``options.override(ar_device_loop=False)``: D passes of fc_resnet_hidden_context + final layer + element-wise
inverse), (iii) the unconditional device loop, and max |dy| / |dlogabsdet| between (i) and (ii).  Every path is warmed up
first; the paths are alternated within one process, three rounds, device events around each call; each round's median and
the spread between rounds are reported.  Prints one JSON document."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from flowconductor_amd import _hip, distributions, flows, options, transforms  # noqa: E402

DEV = torch.device("cuda:0")
ROUNDS = 3


def once(fn):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end)


def alternate(paths, repeats):
    """``paths``: name -> (callable, repeats divisor).  Returns name -> {"ms": median of round medians, "rounds": [...]}."""
    for fn, _ in paths.values():
        fn()
    torch.cuda.synchronize()
    rounds = {name: [] for name in paths}
    for _ in range(ROUNDS):
        for name, (fn, divisor) in paths.items():
            rounds[name].append(statistics.median(once(fn) for _ in range(max(3, repeats // divisor))))
    return {name: {"ms": statistics.median(r), "rounds": r, "spread": (max(r) - min(r)) / statistics.median(r)}
            for name, r in rounds.items()}


def layer(kind, d, context_features):
    if kind == "maf":
        t = transforms.MaskedAffineAutoregressiveTransform(d, 64, context_features=context_features, num_blocks=2)
    else:
        t = transforms.MaskedPiecewiseRationalQuadraticAutoregressiveTransform(
            d, 64, context_features=context_features, num_bins=8, tails="linear", tail_bound=3.0, num_blocks=2)
    return t.eval().to(DEV)


def host_loop(fn):
    def run():
        with options.override(ar_device_loop=False):
            return fn()
    return run


def report(entry, timing):
    entry.update({"device_loop_ms": timing["device"]["ms"], "host_loop_ms": timing["host"]["ms"],
                  "speedup_over_host_loop": timing["host"]["ms"] / timing["device"]["ms"], "rounds": timing})
    if "unconditional" in timing:
        entry["unconditional_device_loop_ms"] = timing["unconditional"]["ms"]
        entry["conditional_over_unconditional"] = timing["device"]["ms"] / timing["unconditional"]["ms"]
    print(json.dumps({k: v for k, v in entry.items() if k != "rounds"}), file=sys.stderr, flush=True)
    return entry


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--out")
    parser.add_argument("--repeats", type=int, default=12)
    args = parser.parse_args()
    result = {"date": time.strftime("%Y-%m-%d"), "device": torch.cuda.get_device_name(0), "library": _hip.library_info(),
              "repeats": args.repeats, "rounds": ROUNDS, "layers": [], "flows": []}
    with torch.no_grad():
        for kind in ("maf", "rq_k8"):
            for d, n in ((64, 2 ** 16), (16, 2 ** 18), (8, 2 ** 20)):
                torch.manual_seed(d)
                t, plain = layer(kind, d, 16), layer(kind, d, None)
                z = torch.randn(n, d, device=DEV)
                c = torch.randn(n, 16, device=DEV)
                y, lad = t.inverse(z, c)
                y_host, lad_host = host_loop(lambda: t.inverse(z, c))()
                entry = {"layer": kind, "d": d, "n": n, "context_features": 16,
                         "max_abs_y": float(y_host.abs().max()), "max_abs_dy": float((y - y_host).abs().max()),
                         "max_abs_dlogabsdet": float((lad - lad_host).abs().max())}
                timing = alternate({"device": (lambda: t.inverse(z, c), 1), "host": (host_loop(lambda: t.inverse(z, c)), 4),
                                    "unconditional": (lambda: plain.inverse(z), 1)}, args.repeats)
                result["layers"].append(report(entry, timing))
        for rows, draws in ((1, 10000), (64, 1000)):
            torch.manual_seed(3)

            def stack(context_features):
                parts = []
                for _ in range(5):
                    parts += [transforms.MaskedAffineAutoregressiveTransform(8, 50, context_features=context_features, num_blocks=2),
                              transforms.ReversePermutation(8)]
                for part in parts[0::2]:        # scale = softplus(u) + 1e-3 = 1 at u = 0.5403: five inverses that do not compound
                    part.autoregressive_net.final_layer.bias[0::2] = 0.5403
                return flows.Flow(transforms.CompositeTransform(parts), distributions.StandardNormal([8])).eval().to(DEV)

            flow, plain = stack(10), stack(None)
            c = torch.randn(rows, 10, device=DEV)
            noise = torch.randn(rows * draws, 8, device=DEV)
            rows_c = c.repeat_interleave(draws, dim=0)
            y, lad = flow._transform.inverse(noise, rows_c)
            y_host, lad_host = host_loop(lambda: flow._transform.inverse(noise, rows_c))()
            entry = {"flow": "5 x [MAF(8, hidden 50, 2 blocks, context 10), reverse]", "context_rows": rows, "draws": draws,
                     "max_abs_y": float(y_host.abs().max()), "max_abs_dy": float((y - y_host).abs().max()),
                     "max_abs_dlogabsdet": float((lad - lad_host).abs().max())}
            timing = alternate({"device": (lambda: flow.sample(draws, context=c), 1),
                                "host": (host_loop(lambda: flow.sample(draws, context=c)), 4),
                                "unconditional": (lambda: plain.sample(rows * draws), 1)}, args.repeats)
            result["flows"].append(report(entry, timing))
    text = json.dumps(result, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
