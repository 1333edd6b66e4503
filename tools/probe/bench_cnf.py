"""Eval-mode continuous normalizing flows: the kernel routes against the torch composition.

    python tools/probe/bench_cnf.py [--out result.json] [--repeats 5] [--cases toy_4096,toy_65536,...]

Cases: the FFJORD toy net (D = 2, hidden 3 x 64, concatsquash / tanh) at N = 4096, 2^16 and 2^20, and D = 16 (hidden
3 x 64) at N = 2^16, plus both at the dispatch's row limit (2^14 and 2048 rows: ``ops.CNF_KERNEL_MAX_LANES`` lanes);
T = 1, standard-normal rows.  The kernel routes are forced (``cnf_kernels="force"``), so they are timed beyond that
limit too.  Per case, alternating rounds of

* ``solve_one_launch``   ``CNF.forward`` with ``rk4``, 8 steps: one ``fc_cnf_integrate`` launch,
* ``solve_field_loop``   the same steps as the host loop of ``odeint`` over ``fc_cnf_field`` (32 launches),
* ``solve_composition``  the same steps in torch ops (``cnf_kernels=False``),
* ``dopri5_field_loop`` / ``dopri5_composition``   ``CNF.forward`` with ``dopri5`` at 1e-5 (what the dispatch gives),
* ``field_kernel`` / ``field_composition``   one evaluation of the ODE function,

each round timing ``calls`` back-to-back calls between two device events (one call for the composition routes);
reported are the median per call and the spread (max - min over the rounds).  The one-launch result is checked at the
timed size against the composition's.  A device is required."""
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
from flowconductor_amd.CNF.odeint import odeint  # noqa: E402

CASES = {"toy_4096": (2, 4096), "toy_16384": (2, 1 << 14), "toy_65536": (2, 1 << 16), "toy_1048576": (2, 1 << 20),
         "d16_2048": (16, 2048), "d16_65536": (16, 1 << 16)}
STEPS = 8


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


def route(fn, value):
    def run():
        with options.override(cnf_kernels=value):
            return fn()
    return run


def off(fn):
    return route(fn, False)


def on(fn):
    return route(fn, "force")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--cases", default=",".join(CASES))
    args = ap.parse_args()
    if args.repeats < 5:
        ap.error("at least 5 repeats")
    if not torch.cuda.is_available():
        raise SystemExit("bench_cnf: no HIP device")
    dev = torch.device("cuda:0")
    result = {"library": _hip.library_info(), "device": torch.cuda.get_device_name(0), "repeats": args.repeats,
              "calls_per_round": args.calls, "rk4_steps": STEPS, "cases": []}
    for name in args.cases.split(","):
        d, n = CASES[name]
        torch.manual_seed(d + n)
        net = ODEnet((64, 64, 64), (d,), None, False, layer_type="concatsquash", nonlinearity="tanh")
        func = ODEfunc(net).eval().to(dev)
        fixed = CNF(func, T=1.0, solver="rk4").eval().to(dev)
        fixed.solver_options = {"step_size": 1.0 / STEPS}
        adaptive = CNF(func, T=1.0, solver="dopri5", atol=1e-5, rtol=1e-5).eval().to(dev)
        z = torch.randn(n, d, device=dev)
        logp = torch.zeros(n, 1, device=dev)

        def field_loop():
            func.before_odeint()
            return odeint(func, (z, logp), [0.0, 1.0], method="rk4", options=fixed.solver_options)

        routes = {
            "solve_one_launch": (on(lambda: fixed(z, logp)), args.calls),
            "solve_field_loop": (on(field_loop), args.calls),
            "solve_composition": (off(lambda: fixed(z, logp)), 1),
            "dopri5_field_loop": (on(lambda: adaptive(z, logp)), 1),
            "dopri5_composition": (off(lambda: adaptive(z, logp)), 1),
            "field_kernel": (on(lambda: func(0.5, (z, logp))), args.calls),
            "field_composition": (off(lambda: func(0.5, (z, logp))), 1),
        }
        entry = {"case": name, "features": d, "rows": n}
        with torch.no_grad():
            got, want = on(lambda: fixed(z, logp))(), off(lambda: fixed(z, logp))()
            entry["one_launch_vs_composition"] = {"z": float((got[0] - want[0]).abs().max()),
                                                  "logp": float((got[1] - want[1]).abs().max())}
            on(lambda: adaptive(z, logp))()
            entry["dopri5_evals_field_loop"] = adaptive.num_evals()
            off(lambda: adaptive(z, logp))()
            entry["dopri5_evals_composition"] = adaptive.num_evals()
            for fn, _ in routes.values():
                fn()
            torch.cuda.synchronize()
            times = {key: [] for key in routes}
            for _ in range(args.repeats):
                for key, (fn, calls) in routes.items():
                    times[key].append(timed(fn, calls))
        for key in routes:
            entry[key] = summary(times[key])
        result["cases"].append(entry)
        print("%s (D %d, N %d): " % (name, d, n) + " | ".join(
            "%s %.3f ms (spread %.3f)" % (key, entry[key]["median_ms"], entry[key]["spread_ms"]) for key in routes)
            + " | dopri5 evals %d / %d | max diff z %.2g logp %.2g"
            % (entry["dopri5_evals_field_loop"], entry["dopri5_evals_composition"],
               entry["one_launch_vs_composition"]["z"], entry["one_launch_vs_composition"]["logp"]), flush=True)
        del z, logp, got, want
        torch.cuda.empty_cache()
    print(json.dumps(result))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
