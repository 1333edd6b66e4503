"""Eval-mode ``dopri5`` solves of a continuous normalizing flow: the one-launch kernel with per-row step control against
the two routes the package had.

    python tools/probe/bench_cnf_dopri5.py [--out result.json] [--repeats 5] [--nets toy,limit] [--max-lanes 131072]
                                           [--gain 1.0]

Nets: the FFJORD toy net (D = 2, hidden 3 x 64, concatsquash / tanh) and the net at the kernels' limits (D = 16, hidden
4 x 64, concatsquash / tanh), every parameter multiplied by ``--gain``; T = 1, standard-normal rows, tolerances 1e-5,
N in powers of two from 2^6 while ``N * G <= --max-lanes``.  Per case, alternating rounds of

* ``kernel``        ``CNF.forward`` with ``cnf_dopri5_kernel="force"``: one ``fc_cnf_dopri5`` launch,
* ``field_loop``    the route without the option: the host loop of ``odeint`` over ``fc_cnf_field``
  (``cnf_kernels="force"``, so that it is timed beyond the dispatch's row limit too),
* ``composition``   the same loop in torch ops (``cnf_kernels=False``),

each round timing ``calls`` back-to-back calls between two device events (one call for the composition); reported are
the median per call and the spread (max - min over the rounds), the attempts per row of the kernel (mean, max) against
the attempts of the batch-wide loop, and the largest difference between the kernel's result and the field loop's.
Every route is warmed up at the timed shape first.  A device is required."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from flowconductor_amd import _hip, ops, options  # noqa: E402
from flowconductor_amd.CNF import CNF  # noqa: E402
from flowconductor_amd.CNF.neural_odes import ODEfunc, ODEnet  # noqa: E402

NETS = {"toy": (2, (64, 64, 64)), "limit": (16, (64, 64, 64, 64))}
TOL = 1e-5


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


def route(fn, **values):
    def run():
        with options.override(**values):
            return fn()
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--nets", default=",".join(NETS))
    ap.add_argument("--max-lanes", type=int, default=1 << 17)
    ap.add_argument("--gain", type=float, default=1.0)
    args = ap.parse_args()
    if args.repeats < 5:
        ap.error("at least 5 repeats")
    if not torch.cuda.is_available():
        raise SystemExit("bench_cnf_dopri5: no HIP device")
    dev = torch.device("cuda:0")
    result = {"library": _hip.library_info(), "device": torch.cuda.get_device_name(0), "repeats": args.repeats,
              "calls_per_round": args.calls, "tol": TOL, "gain": args.gain, "cases": []}
    for name in args.nets.split(","):
        d, hidden = NETS[name]
        lanes = ops.cnf_group_lanes(d)
        torch.manual_seed(d)
        net = ODEnet(hidden, (d,), None, False, layer_type="concatsquash", nonlinearity="tanh")
        with torch.no_grad():
            for p in net.parameters():
                p.mul_(args.gain)
        func = ODEfunc(net).eval().to(dev)
        flow = CNF(func, T=1.0, solver="dopri5", atol=TOL, rtol=TOL).eval().to(dev)
        n = 64
        while n * lanes <= args.max_lanes:
            torch.manual_seed(d + n)
            z = torch.randn(n, d, device=dev)
            logp = torch.zeros(n, 1, device=dev)
            solve = lambda: flow(z, logp)  # noqa: E731
            routes = {
                "kernel": (route(solve, cnf_kernels="force", cnf_dopri5_kernel="force"), args.calls),
                "field_loop": (route(solve, cnf_kernels="force", cnf_dopri5_kernel=False), args.calls),
                "composition": (route(solve, cnf_kernels=False, cnf_dopri5_kernel=False), 1),
            }
            entry = {"net": name, "features": d, "rows": n, "lanes": n * lanes}
            with torch.no_grad():
                with ops.KernelTimer("fc_cnf_dopri5") as whole:
                    got = routes["kernel"][0]()
                assert len(whole.pairs) == 1, "the kernel route did not reach fc_cnf_dopri5"
                entry["kernel_evals"] = flow.num_evals()
                want = routes["field_loop"][0]()
                entry["loop_attempts"] = (flow.num_evals() - 2) / 6
                entry["kernel_vs_field_loop"] = {"z": float((got[0] - want[0]).abs().max()),
                                                 "logp": float((got[1] - want[1]).abs().max())}
                plan = func._plan_for(z)
                attempts = ops.cnf_dopri5(z, None, t0=0.0, t1=1.0, atol=TOL, rtol=TOL, **func._kernel_args(plan))[2]
                entry["row_attempts_mean"] = float(attempts.float().mean())
                entry["row_attempts_max"] = int(attempts.max())
                for fn, _ in routes.values():       # warm-up of every route at this shape
                    fn()
                torch.cuda.synchronize()
                times = {key: [] for key in routes}
                for _ in range(args.repeats):
                    for key, (fn, calls) in routes.items():
                        times[key].append(timed(fn, calls))
            for key in routes:
                entry[key] = summary(times[key])
            result["cases"].append(entry)
            print("%s (D %d, N %d, lanes %d): " % (name, d, n, n * lanes) + " | ".join(
                "%s %.3f ms (spread %.3f)" % (key, entry[key]["median_ms"], entry[key]["spread_ms"]) for key in routes)
                + " | attempts per row mean %.2f max %d, batch-wide loop %.0f | max diff z %.2g logp %.2g"
                % (entry["row_attempts_mean"], entry["row_attempts_max"], entry["loop_attempts"],
                   entry["kernel_vs_field_loop"]["z"], entry["kernel_vs_field_loop"]["logp"]), flush=True)
            del z, logp, got, want
            n *= 2
        torch.cuda.empty_cache()
    print(json.dumps(result))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
