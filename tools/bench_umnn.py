"""Time the UMNN map on the GPU: ``fc_umnn`` forward and inverse, the torch composition, and the reference-style inverse
(25 bisections + both ends + the closing forward = 28 integrals on the composition), same device, same inputs; and one
training step (forward + backward of a loss on outputs and logabsdet, gradients to x, h and the integrand's parameters) on
the kernel route (``fc_umnn`` + ``fc_umnn_backward``, options ``umnn_training``) and on the composition in one piece, each
with its device-event time and its peak ``torch.cuda.max_memory_allocated``.

    python tools/bench_umnn.py [--rows 65536] [--features 8] [--repeats 20]

Prints one JSON line: milliseconds per call and the share of the split-f16 matrix peak the kernel's MFMA work amounts to
(3 terms x 2 flop x rows x features x (nb_steps + 2) points x the padded 64 x 64 products of the hidden layers, plus the
once-per-element 64 x 32 product).  The roof of this kernel is compute, not HBM: ~90 bytes per element against ~0.5
Mflop of matrix work."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from flowconductor_amd import ops, options  # noqa: E402
from flowconductor_amd.transforms.UMNN import MonotonicNormalizer  # noqa: E402

F16_DENSE_PEAK = 2.5e15      # flop/s, MI355X matrix cores, f16 dense


def timed(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(repeats):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / repeats


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=65536)
    ap.add_argument("--features", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--chunk", type=int, default=8192, help="rows per call of the torch composition (inference rows)")
    ap.add_argument("--train-repeats", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    norm = MonotonicNormalizer([50, 50, 50], 20, nb_steps=20).to(dev).eval()
    with torch.no_grad():
        for p in norm.parameters():
            p.mul_(1.5)
    n, d = args.rows, args.features
    x = 1.5 * torch.randn(n, d, device=dev)
    h = torch.randn(n, d, 20, device=dev)

    def compose(v, inverse):
        outs = []
        for i in range(0, n, args.chunk):
            vv, hh = v[i:i + args.chunk], h[i:i + args.chunk]
            if inverse:
                xx = norm._compose_inverse(vv, hh)
                outs.append((xx, -norm._compose(xx, hh)[1].log().sum(1)))
            else:
                zz, jac = norm._compose(vv, hh)
                outs.append((zz, jac.log().sum(1)))
        return torch.cat([o[0] for o in outs]), torch.cat([o[1] for o in outs])

    with torch.no_grad():
        z, lad = norm.apply_with_logabsdet(x, h)
        zc, ladc = compose(x, False)
        xr, ladr = norm.apply_with_logabsdet(z, h, inverse=True)
        res = {
            "rows": n, "features": d,
            "max_abs_z_kernel_vs_composition": float((z - zc).abs().max()),
            "max_abs_lad_kernel_vs_composition": float((lad - ladc).abs().max()),
            "max_abs_roundtrip_x": float((xr - x).abs().max()),
            "kernel_forward_ms": timed(lambda: norm.apply_with_logabsdet(x, h), 3, args.repeats),
            "kernel_inverse_ms": timed(lambda: norm.apply_with_logabsdet(z, h, inverse=True), 3, args.repeats),
            "composition_forward_ms": timed(lambda: compose(x, False), 1, 3),
            "reference_style_inverse_28_integrals_ms": timed(lambda: compose(z, True), 1, 2),
        }
        with ops.KernelTimer("fc_umnn") as timer:
            for _ in range(5):
                norm.apply_with_logabsdet(x, h)
        torch.cuda.synchronize()
        res["fc_umnn_forward_entry_ms"] = min(timer.durations_ms())
    # ---- one training step on each route -----------------------------------------------------------------------------
    gy, gl = torch.randn(n, d, device=dev), torch.randn(n, device=dev)

    def step():
        xl, hl = x.detach().requires_grad_(True), h.detach().requires_grad_(True)
        for p in norm.parameters():
            p.grad = None
        out, logabsdet = norm.apply_with_logabsdet(xl, hl)
        ((out * gy).sum() + (logabsdet * gl).sum()).backward()
        return xl.grad, hl.grad

    grads = {}
    for route, on in (("kernel", True), ("composition", False)):
        with options.override(umnn_training=on):
            step()                                                   # images, workspaces, allocator pools
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            before = torch.cuda.memory_allocated()
            res["training_step_%s_ms" % route] = timed(step, 0, args.train_repeats)
            res["training_step_%s_peak_bytes" % route] = torch.cuda.max_memory_allocated()
            res["training_step_%s_peak_bytes_above_inputs" % route] = torch.cuda.max_memory_allocated() - before
            grads[route] = [g.clone() for g in step()] + [p.grad.clone() for p in norm.parameters()]
    res["training_max_grad_diff_kernel_vs_composition_over_largest_entry"] = max(
        float((a - b).abs().max() / b.abs().max()) for a, b in zip(grads["kernel"], grads["composition"]))
    with options.override(umnn_training=True), ops.KernelTimer("fc_umnn_backward") as timer:
        for _ in range(3):
            step()
    torch.cuda.synchronize()
    res["fc_umnn_backward_entry_ms"] = min(timer.durations_ms())
    flop = 3 * 2 * n * d * (22 * 2 * 64 * 64 + 64 * 32)
    res["mfma_flop_forward"] = flop
    res["split_f16_peak_fraction_forward"] = flop / (res["fc_umnn_forward_entry_ms"] * 1e-3) / F16_DENSE_PEAK
    print(json.dumps(res))


if __name__ == "__main__":
    main()
