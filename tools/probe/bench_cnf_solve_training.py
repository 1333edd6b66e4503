"""A training step of a continuous normalizing flow under a fixed-step solver on three routes: the torch composition,
one autograd node per evaluation (options ``cnf_training``) and one node for the whole solve (options
``cnf_solve_training``).

    python tools/probe/bench_cnf_solve_training.py [--out result.json] [--repeats 5] [--cases toy_4096,...]

One step is the forward solve in training mode, the loss ``mean(0.5 |z|^2 + delta logp)`` and its backward to the
parameters; no optimiser.  Cases: those of tools/probe/bench_cnf_training.py (the FFJORD toy net, D = 2, hidden 3 x 64,
concatsquash / tanh, at N = 1024, 4096, 2^14 and 2^16, and D = 16 at N = 2048 and 2^14); T = 1, standard-normal rows;
``rk4`` with 8 steps (32 evaluations); ``divergence_fn`` ``approximate`` (Hutchinson, the noise fixed over the rounds) and
``brute_force`` (exact).  Per case and divergence, alternating rounds of

* ``composition``   both options off: the net in torch ops, the divergence by autograd, a double backward,
* ``evaluation``    ``cnf_training="force"``: one ``fc_cnf_field_train`` and one ``fc_cnf_field_backward`` launch per
                    evaluation of the ODE function, the Runge-Kutta combination in torch ops between them,
* ``solve``         ``cnf_solve_training="force"``: one ``fc_cnf_integrate_train`` and one ``fc_cnf_integrate_backward``
                    launch per solve,

each round timing one step between two device events; reported are the median and the spread (max - min over the
rounds), the peak device memory of a step on each route, and the largest difference of a kernel route's parameter
gradients from the composition's relative to the largest gradient.  The new route is compared with the two others, never
with itself.  A device is required."""
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
ROUTES = {"composition": dict(cnf_training=False, cnf_solve_training=False),
          "evaluation": dict(cnf_training="force", cnf_solve_training=False),
          "solve": dict(cnf_training=False, cnf_solve_training="force")}
LAUNCHES = {"composition": (0, 0, 0), "evaluation": (4 * STEPS, 0, 0), "solve": (0, 1, 1)}


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
    ap.add_argument("--divergences", default="approximate,brute_force")
    args = ap.parse_args()
    if args.repeats < 5:
        ap.error("at least 5 repeats")
    if not torch.cuda.is_available():
        raise SystemExit("bench_cnf_solve_training: no HIP device")
    dev = torch.device("cuda:0")
    result = {"library": _hip.library_info(), "device": torch.cuda.get_device_name(0), "repeats": args.repeats,
              "rk4_steps": STEPS, "cases": []}
    for name in args.cases.split(","):
        d, n = CASES[name]
        for divergence in args.divergences.split(","):
            torch.manual_seed(d + n)
            net = ODEnet((64, 64, 64), (d,), None, False, layer_type="concatsquash", nonlinearity="tanh")
            func = ODEfunc(net, divergence_fn=divergence).to(dev)
            flow = CNF(func, T=1.0, solver="rk4").to(dev).train()
            flow.solver_options = {"step_size": 1.0 / STEPS}
            z = torch.randn(n, d, device=dev)
            logp = torch.zeros(n, 1, device=dev)
            noise = torch.randn(n, d, device=dev)
            original = func.before_odeint
            func.before_odeint = lambda *a, **k: original(e=noise)      # the same estimate on every route
            params = list(flow.parameters())

            def step(values):
                def run():
                    with options.override(**values):
                        z_t, logp_t = flow(z, logp)
                        loss = (0.5 * z_t.square().sum(dim=1) + logp_t.reshape(-1)).mean()
                        return torch.autograd.grad(loss, params)
                return run

            routes = {key: step(values) for key, values in ROUTES.items()}
            hutchinson = divergence == "approximate"
            entry = {"case": name, "features": d, "rows": n, "divergence": divergence,
                     "lanes": ops.cnf_train_lanes(n, d, hutchinson),
                     "tape_mib": 4.0 * 4 * STEPS * n * d / 2 ** 20}
            grads = {}
            for key, fn in routes.items():
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                before = torch.cuda.memory_allocated()
                with ops.KernelTimer("fc_cnf_field_train") as evaluations, \
                        ops.KernelTimer("fc_cnf_integrate_train") as solves, \
                        ops.KernelTimer("fc_cnf_integrate_backward") as sweeps:
                    grads[key] = fn()
                torch.cuda.synchronize()
                entry[key + "_peak_mib"] = (torch.cuda.max_memory_allocated() - before) / 2 ** 20
                launched = (len(evaluations.pairs), len(solves.pairs), len(sweeps.pairs))
                if launched != LAUNCHES[key] or flow.num_evals() != 4 * STEPS:
                    raise SystemExit("bench_cnf_solve_training: route %s launched %r" % (key, launched))
            largest = max(float(g.abs().max()) for g in grads["composition"])
            for key in ("evaluation", "solve"):
                entry[key + "_gradient_difference"] = max(
                    float((a - b).abs().max()) for a, b in zip(grads[key], grads["composition"])) / largest
            del grads
            times = {key: [] for key in routes}
            for _ in range(args.repeats):
                for key, fn in routes.items():
                    times[key].append(timed(fn))
            for key in routes:
                entry[key] = summary(times[key])
            entry["solve_over_composition"] = entry["composition"]["median_ms"] / entry["solve"]["median_ms"]
            entry["solve_over_evaluation"] = entry["evaluation"]["median_ms"] / entry["solve"]["median_ms"]
            result["cases"].append(entry)
            print("%-10s %-11s " % (name, divergence) + " | ".join(
                "%s %8.3f ms (spread %.3f, peak %.1f MiB)" % (key, entry[key]["median_ms"], entry[key]["spread_ms"],
                                                              entry[key + "_peak_mib"]) for key in routes)
                + " | solve x%.2f composition, x%.2f evaluation | rel. gradient difference %.1e / %.1e"
                % (entry["solve_over_composition"], entry["solve_over_evaluation"],
                   entry["evaluation_gradient_difference"], entry["solve_gradient_difference"]), flush=True)
            del z, logp, noise, flow, func, net, params
            torch.cuda.empty_cache()
    print(json.dumps(result))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
