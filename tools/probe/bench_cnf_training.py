"""A training step of a continuous normalizing flow: the kernel route (options ``cnf_training``) against the torch
composition.

    python tools/probe/bench_cnf_training.py [--out result.json] [--repeats 5] [--cases toy_4096,...] [--solvers rk4]

One step is the forward solve in training mode, the loss ``mean(0.5 |z|^2 + delta logp)`` and its backward to the
parameters; no optimiser.  Cases: the FFJORD toy net (D = 2, hidden 3 x 64, concatsquash / tanh) at N = 1024, 4096,
2^14 and 2^16, and D = 16 (hidden 3 x 64) at N = 2048 and 2^14; T = 1, standard-normal rows; ``rk4`` with 8 steps and
``dopri5`` at 1e-5; ``divergence_fn`` ``approximate`` (Hutchinson, the noise fixed over the rounds) and ``brute_force``
(exact).  Per case, solver and divergence, alternating rounds of

* ``kernels``       ``cnf_training="force"``: one ``fc_cnf_field_train`` and one ``fc_cnf_field_backward`` launch per
                    evaluation of the ODE function,
* ``composition``   ``cnf_training=False``: the net in torch ops, the divergence by autograd, a double backward,

each round timing one step between two device events; reported are the median and the spread (max - min over the
rounds), the peak device memory of a step on each route, the evaluations of a solve, and the largest difference of the
two routes' parameter gradients relative to the largest gradient.  A device is required."""
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

CASES = {"toy_1024": (2, 1024), "toy_4096": (2, 4096), "toy_16384": (2, 1 << 14), "toy_65536": (2, 1 << 16),
         "d16_2048": (16, 2048), "d16_16384": (16, 1 << 14)}
STEPS = 8


def timed(fn):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop)


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "spread_ms": max(ms) - min(ms),
            "samples": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--solvers", default="rk4,dopri5")
    ap.add_argument("--divergences", default="approximate,brute_force")
    args = ap.parse_args()
    if args.repeats < 5:
        ap.error("at least 5 repeats")
    if not torch.cuda.is_available():
        raise SystemExit("bench_cnf_training: no HIP device")
    dev = torch.device("cuda:0")
    result = {"library": _hip.library_info(), "device": torch.cuda.get_device_name(0), "repeats": args.repeats,
              "rk4_steps": STEPS, "cases": []}
    for name in args.cases.split(","):
        d, n = CASES[name]
        for solver in args.solvers.split(","):
            for divergence in args.divergences.split(","):
                torch.manual_seed(d + n)
                net = ODEnet((64, 64, 64), (d,), None, False, layer_type="concatsquash", nonlinearity="tanh")
                func = ODEfunc(net, divergence_fn=divergence).to(dev)
                flow = CNF(func, T=1.0, solver=solver, atol=1e-5, rtol=1e-5).to(dev).train()
                if solver != "dopri5":
                    flow.solver_options = {"step_size": 1.0 / STEPS}
                z = torch.randn(n, d, device=dev)
                logp = torch.zeros(n, 1, device=dev)
                noise = torch.randn(n, d, device=dev)
                original = func.before_odeint
                func.before_odeint = lambda *a, **k: original(e=noise)      # the same estimate on both routes
                params = list(flow.parameters())

                def step(value):
                    def run():
                        with options.override(cnf_training=value):
                            z_t, logp_t = flow(z, logp)
                            loss = (0.5 * z_t.square().sum(dim=1) + logp_t.reshape(-1)).mean()
                            return torch.autograd.grad(loss, params)
                    return run

                routes = {"kernels": step("force"), "composition": step(False)}
                entry = {"case": name, "features": d, "rows": n, "solver": solver, "divergence": divergence,
                         "lanes": ops.cnf_train_lanes(n, d, divergence == "approximate")}
                grads = {}
                for key, fn in routes.items():
                    torch.cuda.synchronize()
                    torch.cuda.reset_peak_memory_stats()
                    before = torch.cuda.memory_allocated()
                    grads[key] = fn()
                    torch.cuda.synchronize()
                    entry[key + "_peak_mib"] = (torch.cuda.max_memory_allocated() - before) / 2 ** 20
                    entry[key + "_evals"] = flow.num_evals()
                largest = max(float(g.abs().max()) for g in grads["composition"])
                entry["gradient_difference"] = max(
                    float((a - b).abs().max()) for a, b in zip(grads["kernels"], grads["composition"])) / largest
                del grads
                times = {key: [] for key in routes}
                for _ in range(args.repeats):
                    for key, fn in routes.items():
                        times[key].append(timed(fn))
                for key in routes:
                    entry[key] = summary(times[key])
                entry["speedup"] = entry["composition"]["median_ms"] / entry["kernels"]["median_ms"]
                result["cases"].append(entry)
                print("%-10s %-6s %-11s kernels %8.3f ms (spread %.3f, peak %.1f MiB, %d evals) | composition %8.3f ms "
                      "(spread %.3f, peak %.1f MiB, %d evals) | x%.2f | rel. gradient difference %.1e"
                      % (name, solver, divergence, entry["kernels"]["median_ms"], entry["kernels"]["spread_ms"],
                         entry["kernels_peak_mib"], entry["kernels_evals"], entry["composition"]["median_ms"],
                         entry["composition"]["spread_ms"], entry["composition_peak_mib"], entry["composition_evals"],
                         entry["speedup"], entry["gradient_difference"]), flush=True)
                del z, logp, noise, flow, func, net, params
                torch.cuda.empty_cache()
    print(json.dumps(result))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
