"""Sampling direction of the sum-of-sigmoids and sibling-spline autoregressive layers: the one-kernel device loop
(fc_made_inverse_sos / fc_made_inverse_spline) against another build of this package (the parent commit) and against this
build's own host loop.

    python tools/probe/bench_ar_device_loop_forms.py --old PATH_TO_OLD_TREE [--repeats 2] [--calls 20] [--out FILE.json]
    python tools/probe/bench_ar_device_loop_forms.py --sweep [--calls 20] [--out FILE.json]
    python tools/probe/bench_ar_device_loop_forms.py --float64 [--out FILE.json]

--sweep times the sum-of-sigmoids kernel against this build's host loop over S x D x N (the table ``ops.MADE_SOS_ROW_SIGMOIDS``
is read from); --float64 holds both routes of the spline shapes, at the timed size, against the float64 oracle on the CPU.
Both run in this process, on this tree alone.

The driver never touches the GPU: it starts one fresh child process per (tree, repeat), alternating old and new, so that
clock and thermal drift hit both alike; the spread of a shape is the largest difference between repeats of the same build.
A child (--tree PATH) imports the package from PATH, times ``inverse`` of every shape with device events (median of
--calls calls after warm-up; the host loop is launch-bound, so the span between events around the whole call is what a
caller waits for), and writes the outputs of seeded inputs so that the driver can compare old and new at the timed sizes
against the bounds of tests/test_gpu_ar_device_loop_forms.py."""
import argparse
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# (name, kind, bins / sigmoids, D, N)
SHAPES = [("sos S=30 D=8 N=2^18", "sos", 30, 8, 1 << 18), ("sos S=30 D=64 N=2^16", "sos", 30, 64, 1 << 16),
          ("sos S=30 D=8 N=4096", "sos", 30, 8, 4096), ("cubic K=10 D=16 N=2^18", "cubic", 10, 16, 1 << 18),
          ("quadratic K=10 tails D=16 N=2^18", "quadratic_tails", 10, 16, 1 << 18),
          ("linear K=10 D=16 N=2^18", "linear", 10, 16, 1 << 18), ("linear K=10 D=16 N=4096", "linear", 10, 16, 4096)]
FLOW = "flow 3 x sos S=30 D=8 sample(2^16)"


def _layer(T, kind, k, features):
    if kind == "sos":
        return T.MaskedSumOfSigmoidsTransform(features, 64, n_sigmoids=k)
    if kind == "linear":
        return T.MaskedPiecewiseLinearAutoregressiveTransform(k, features, 64)
    if kind == "quadratic_tails":
        return T.MaskedPiecewiseQuadraticAutoregressiveTransform(k, features, 64, tails="linear", tail_bound=3.0)
    return T.MaskedPiecewiseCubicAutoregressiveTransform(k, features, 64)


def _inputs(torch, kind, n, features):
    g = torch.Generator().manual_seed(5)
    if kind == "sos":
        return torch.randn(n, features, generator=g) * 0.6
    if kind == "quadratic_tails":
        return torch.randn(n, features, generator=g) * 1.2
    return torch.rand(n, features, generator=g) * 0.98 + 0.01


def child(tree, calls, dump):
    sys.path.insert(0, tree)
    import numpy as np
    import torch

    import flowconductor_amd
    from flowconductor_amd import distributions, flows, options
    from flowconductor_amd import transforms as T

    assert os.path.realpath(flowconductor_amd.__file__).startswith(os.path.realpath(tree))
    dev = torch.device("cuda:0")

    def median_ms(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        times = []
        for _ in range(calls):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            times.append(a.elapsed_time(b))
        return float(np.median(times))

    result = {}
    with torch.no_grad():
        for name, kind, k, features, n in SHAPES:
            torch.manual_seed(features + k)
            t = _layer(T, kind, k, features).eval()
            for p in t.parameters():
                p.mul_(1.5)
            t = t.to(dev)
            x = _inputs(torch, kind, n, features).to(dev)
            row = {"default_ms": median_ms(lambda: t.inverse(x)),
                   "device_loop": bool(t._device_loop_ok(x, None))}
            y, lad = t.inverse(x)
            with options.override(ar_device_loop=False):
                row["host_loop_ms"] = median_ms(lambda: t.inverse(x))
            np.save(os.path.join(dump, name.replace(" ", "_").replace("^", "") + ".y.npy"), y.cpu().numpy())
            np.save(os.path.join(dump, name.replace(" ", "_").replace("^", "") + ".lad.npy"), lad.cpu().numpy())
            result[name] = row
        torch.manual_seed(11)
        layers = []
        for _ in range(3):
            layers += [T.MaskedSumOfSigmoidsTransform(8, 64), T.ReversePermutation(8)]
        flow = flows.Flow(T.CompositeTransform(layers), distributions.StandardNormal([8])).eval().to(dev)
        row = {"default_ms": median_ms(lambda: flow.sample(1 << 16))}
        with options.override(ar_device_loop=False):
            row["host_loop_ms"] = median_ms(lambda: flow.sample(1 << 16))
        result[FLOW] = row
    print("RESULT " + json.dumps(result), flush=True)


def driver(old, repeats, calls, out):
    import numpy as np

    runs = {"old": [], "new": []}
    dumps = {}
    with tempfile.TemporaryDirectory() as tmp:
        for r in range(repeats):
            for which, tree in (("old", old), ("new", HERE)):
                dump = os.path.join(tmp, "%s%d" % (which, r))
                os.makedirs(dump)
                done = subprocess.run([sys.executable, os.path.abspath(__file__), "--tree", tree, "--calls", str(calls),
                                       "--dump", dump], capture_output=True, text=True, timeout=900)
                if done.returncode != 0:
                    sys.stderr.write(done.stdout[-2000:] + done.stderr[-4000:])
                    raise SystemExit("the %s build's run ended with status %d: nothing more is started" % (which, done.returncode))
                line = [l for l in done.stdout.splitlines() if l.startswith("RESULT ")][-1]
                runs[which].append(json.loads(line[7:]))
                dumps[which] = dump
        table = {}
        for name in list(runs["new"][0]):
            old_ms = [r[name]["default_ms"] for r in runs["old"]]
            new_ms = [r[name]["default_ms"] for r in runs["new"]]
            host_ms = [r[name]["host_loop_ms"] for r in runs["new"]]
            row = {"old_ms": float(np.median(old_ms)), "new_ms": float(np.median(new_ms)),
                   "new_host_loop_ms": float(np.median(host_ms)),
                   "spread_ms": float(max(max(v) - min(v) for v in (old_ms, new_ms, host_ms))),
                   "device_loop": runs["new"][0][name].get("device_loop")}
            row["speedup"] = row["old_ms"] / row["new_ms"]
            stem = name.replace(" ", "_").replace("^", "")
            if os.path.exists(os.path.join(dumps["new"], stem + ".y.npy")):
                yo, yn = (np.load(os.path.join(dumps[w], stem + ".y.npy")).astype(np.float64) for w in ("old", "new"))
                lo, ln = (np.load(os.path.join(dumps[w], stem + ".lad.npy")).astype(np.float64) for w in ("old", "new"))
                # the floor terms of the tests' bounds (no float64 oracle at these sizes: the old build is the reference)
                # (rows that are not finite in either build are counted, not compared: a float32 discriminant that rounding
                #  pushed below zero is a NaN in the reference as well, splines/quadratic.py:139)
                good = np.isfinite(yo).all(axis=1) & np.isfinite(yn).all(axis=1) & np.isfinite(lo) & np.isfinite(ln)
                row["rows_not_finite_old"] = int((~(np.isfinite(yo).all(axis=1) & np.isfinite(lo))).sum())
                row["rows_not_finite_new"] = int((~(np.isfinite(yn).all(axis=1) & np.isfinite(ln))).sum())
                yo, yn, lo, ln = yo[good], yn[good], lo[good], ln[good]
                row["y_diff_over_bound"] = float(np.abs(yo - yn).max() / (1e-4 * max(1.0, np.abs(yo).max())))
                row["lad_diff_over_bound"] = float(np.abs(lo - ln).max() / (1e-3 * max(1.0, np.abs(lo).max() / 10)))
            table[name] = row
            print("%-36s old %8.3f ms  new %8.3f ms  (x%.2f)  new host loop %8.3f ms  spread %.3f ms  dy/bound %s dlad/bound %s"
                  % (name, row["old_ms"], row["new_ms"], row["speedup"], row["new_host_loop_ms"], row["spread_ms"],
                     "%.3f" % row["y_diff_over_bound"] if "y_diff_over_bound" in row else "-",
                     "%.3f" % row["lad_diff_over_bound"] if "lad_diff_over_bound" in row else "-")
                  + ("  rows not finite old %d new %d" % (row["rows_not_finite_old"], row["rows_not_finite_new"])
                     if row.get("rows_not_finite_old") or row.get("rows_not_finite_new") else ""), flush=True)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            json.dump({"runs": runs, "table": table}, f, indent=1)


def _median_ms(torch, np, fn, calls):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times))


def sweep(calls, out):
    """The table behind ``ops.MADE_SOS_ROW_SIGMOIDS``: fc_made_inverse_sos (``_inverse_device_loop``, which knows no row
    limit) against this build's host loop over S x D x N; prints host / device per cell."""
    sys.path.insert(0, HERE)
    import numpy as np
    import torch

    from flowconductor_amd import options
    from flowconductor_amd import transforms as T

    dev = torch.device("cuda:0")
    rows = [1 << 12, 1 << 14, 1 << 15, 1 << 16, 1 << 17, 1 << 18]
    table = {}
    print("S, D | host / device at N = " + " | ".join(str(n) for n in rows), flush=True)
    with torch.no_grad():
        for s in (6, 15, 30):
            for features in (8, 32, 64):
                torch.manual_seed(features + s)
                t = _layer(T, "sos", s, features).eval()
                for p in t.parameters():
                    p.mul_(1.5)
                t = t.to(dev)
                cells = []
                for n in rows:
                    x = _inputs(torch, "sos", n, features).to(dev)
                    device_ms = _median_ms(torch, np, lambda: t._inverse_device_loop(x), calls)
                    with options.override(ar_device_loop=False):
                        host_ms = _median_ms(torch, np, lambda: t.inverse(x), calls)
                    cells.append({"rows": n, "device_ms": device_ms, "host_ms": host_ms, "host_over_device": host_ms / device_ms})
                table["%d, %d" % (s, features)] = cells
                print("%d, %d | " % (s, features) + " | ".join("%.2f" % c["host_over_device"] for c in cells), flush=True)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            json.dump(table, f, indent=1)


def against_float64(out):
    """The two routes of every spline shape of SHAPES against the oracle's D full passes in float64 and float32 on the CPU,
    at the timed size: per route the largest error over the tests' bound (floor + 4 x the float32 oracle's own error, taken
    over the rows the float32 oracle keeps finite), and what the rows that are not finite on a route are in the oracles."""
    sys.path[:0] = [HERE, os.path.join(HERE, "tests", "golden")]
    import copy

    import torch

    from flowconductor_amd import options
    from flowconductor_amd import transforms as T
    from oracle import torch_oracle as O

    dev = torch.device("cuda:0")
    result = {}
    with torch.no_grad():
        for name, kind, k, features, n in SHAPES:
            if kind == "sos" or n < (1 << 18):
                continue
            torch.manual_seed(features + k)
            t = _layer(T, kind, k, features).eval()
            for p in t.parameters():
                p.mul_(1.5)
            x = _inputs(torch, kind, n, features)
            y64, l64 = O.transform_apply(copy.deepcopy(t).double(), x.double(), None, inverse=True)
            y32, l32 = O.transform_apply(t, x.clone(), None, inverse=True)
            t = t.to(dev)
            xd = x.to(dev)
            assert t._device_loop_ok(xd, None)
            routes = {"device loop": tuple(v.cpu() for v in t.inverse(xd))}
            with options.override(ar_device_loop=False):
                routes["host loop"] = tuple(v.cpu() for v in t.inverse(xd))

            def finite(y, lad):
                return torch.isfinite(y).all(dim=1) & torch.isfinite(lad)

            ok64, ok32 = finite(y64, l64), finite(y32, l32)
            both = ok64 & ok32
            err32_y = float((y32.double() - y64)[both].abs().max())
            err32_l = float((l32.double() - l64)[both].abs().max())
            tol_y = 1e-4 * max(1.0, float(y32[both].abs().max())) + 4 * err32_y
            tol_l = 1e-3 * max(1.0, float(l32[both].abs().max()) / 10) + 4 * err32_l
            row = {"rows": n, "rows_not_finite_float64": int((~ok64).sum()), "rows_not_finite_float32_oracle": int((~ok32).sum()),
                   "float32_oracle_max_dy": err32_y, "float32_oracle_max_dlad": err32_l, "tol_y": tol_y, "tol_l": tol_l}
            for route, (y, lad) in routes.items():
                ok = finite(y, lad)
                good = ok & ok64
                dy = (y.double() - y64)[good].abs().amax(dim=1)
                dl = (lad.double() - l64)[good].abs()
                bad = (~ok & ok64).nonzero().flatten().tolist()
                row[route] = {"rows_not_finite": int((~ok).sum()), "max_dy": float(dy.max()), "max_dlad": float(dl.max()),
                              "dy_over_bound": float(dy.max()) / tol_y, "dlad_over_bound": float(dl.max()) / tol_l,
                              "rows_over_floor_y": int((dy > 1e-4 * max(1.0, float(y64[both].abs().max()))).sum()),
                              # rows this route loses that float64 keeps: is the float32 oracle far off there as well?
                              "lost_rows": [{"row": r, "float32_oracle_finite": bool(ok32[r]),
                                             "float32_oracle_dy": float((y32[r].double() - y64[r]).abs().max())}
                                            for r in bad[:8]]}
            floor = 1e-4 * max(1.0, float(y64[both].abs().max()))
            row["float32_oracle_rows_over_floor_y"] = int(((y32.double() - y64)[both].abs().amax(dim=1) > floor).sum())
            yd, yh = routes["device loop"][0].double(), routes["host loop"][0].double()
            good = finite(*routes["device loop"]) & finite(*routes["host loop"]) & ok64
            worst = int((yd - yh)[good].abs().amax(dim=1).argmax())
            idx = good.nonzero().flatten()[worst]
            row["largest_route_difference"] = {
                "row": int(idx), "dy_routes": float((yd[idx] - yh[idx]).abs().max()),
                "device_loop_dy_float64": float((yd[idx] - y64[idx]).abs().max()),
                "host_loop_dy_float64": float((yh[idx] - y64[idx]).abs().max()),
                "float32_oracle_dy_float64": float((y32[idx].double() - y64[idx]).abs().max())}
            result[name] = row
            print(name + " " + json.dumps(row), flush=True)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--sweep", action="store_true", help="S x D x N sweep of the sum-of-sigmoids kernel against the host loop")
    ap.add_argument("--float64", action="store_true", help="both routes of the spline shapes against the float64 oracle")
    ap.add_argument("--old")
    ap.add_argument("--tree")
    ap.add_argument("--dump")
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.sweep:
        sweep(a.calls, a.out)
    elif a.float64:
        against_float64(a.out)
    elif a.tree:
        child(a.tree, a.calls, a.dump)
    else:
        driver(a.old, a.repeats, a.calls, a.out)
