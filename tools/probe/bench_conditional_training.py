"""Forward + backward of ConditionalLUTransform and ConditionalSVDTransform (the per-sample backward kernels) against the
differentiable torch composition of the same layer on the same GPU: ``_create_lower_upper`` + two ``bmm`` for LU, the
reflections as torch ops for SVD.  Both sides run the same hyper-network; the two are timed alternately.

    python tools/probe/bench_conditional_training.py [log2 rows] [repeats] [out.json]

Per shape: step time (device events around forward + backward, median over the repeats), the launches of the new backward
entry alone (ops.KernelTimer) and the bytes that entry has to move, computed from the shapes (LU: two reads of M and one
write of gM per row plus the [N, D] rows; Householder: q in and gq out per launch plus three rows)."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from flowconductor_amd import ops  # noqa: E402
from flowconductor_amd import transforms as T  # noqa: E402

LOG2_ROWS = int(sys.argv[1]) if len(sys.argv) > 1 else 16
REPEATS = int(sys.argv[2]) if len(sys.argv) > 2 else 10
OUT = sys.argv[3] if len(sys.argv) > 3 else None
N = 1 << LOG2_ROWS
CONTEXT = 8
dev = torch.device("cuda")


def reflect(x, q):
    """K per-sample reflections as torch ops (q [N, K, D], index order)."""
    sq = (q * q).sum(-1)
    for k in range(q.shape[1]):
        qk = q[:, k]
        x = x - (x * qk).sum(-1, keepdim=True) * ((2.0 / sq[:, k:k + 1]) * qk)
    return x


def lu_composed(t, x, c):
    params = t.conditional_net(c)
    lower, upper = t._create_lower_upper(params)
    y = torch.bmm(lower, torch.bmm(upper, x.unsqueeze(-1))).squeeze(-1)
    return y, upper.diagonal(0, -1, -2).log().sum(-1)


def svd_composed(t, x, c):
    q_u, q_v, s, bias = t._parts(t.conditional_net(c))
    y = reflect(reflect(x, q_v) * s, q_u)
    return (y + bias if bias is not None else y), s.log().sum(-1)


def step(fn, t, x, c, gy, gl):
    for p in t.parameters():
        p.grad = None
    y, lad = fn(t, x, c)
    ((y * gy).sum() + (lad * gl).sum()).backward()


def timed(fn, t, x, c, gy, gl):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    step(fn, t, x, c, gy, gl)
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end)


def median(v):
    return sorted(v)[len(v) // 2]


results = []
for kind, cls, composed, entry in (("lu", T.ConditionalLUTransform, lu_composed, "fc_linear_per_sample_backward"),
                                   ("svd", T.ConditionalSVDTransform, svd_composed, "fc_householder_backward_per_sample")):
    for d in (8, 16, 64):
        torch.manual_seed(d)
        t = cls(d, 64, CONTEXT).to(dev).train()
        x, c = torch.randn(N, d, device=dev), torch.randn(N, CONTEXT, device=dev)
        gy, gl = torch.randn(N, d, device=dev), torch.randn(N, device=dev)
        hip = lambda t_, x_, c_: t_(x_, c_)      # noqa: E731
        for _ in range(3):                       # warm up both sides at this shape
            step(hip, t, x, c, gy, gl)
            step(composed, t, x, c, gy, gl)
        torch.cuda.synchronize()
        hip_ms, torch_ms = [], []
        with ops.KernelTimer(entry) as kt:
            for _ in range(REPEATS):             # alternate the two
                hip_ms.append(timed(hip, t, x, c, gy, gl))
                torch_ms.append(timed(composed, t, x, c, gy, gl))
        torch.cuda.synchronize()
        launches = kt.durations_ms()
        per_step = len(launches) // REPEATS
        kernel_ms = median([sum(launches[i * per_step:(i + 1) * per_step]) for i in range(REPEATS)])
        row = dict(layer=kind, d=d, n=N, hip_step_ms=median(hip_ms), torch_step_ms=median(torch_ms),
                   hip_step_min_max=[min(hip_ms), max(hip_ms)], torch_step_min_max=[min(torch_ms), max(torch_ms)],
                   backward_entry=entry, backward_launches_per_step=per_step, backward_kernel_ms=kernel_ms)
        if kind == "lu":
            byts = N * (3 * d * d + 4 * d + 2) * 4      # M twice in, gM once out; x, gy, gx, diag; gl, g_sp
            row.update(backward_bytes=byts, backward_tb_per_s=byts / kernel_ms / 1e9)
        else:
            byts = N * (2 * d * d + 3 * d) * 4          # per launch: q in, gq out; y, gy in, gx out
            row.update(backward_bytes_per_launch=byts, backward_tb_per_s=per_step * byts / kernel_ms / 1e9)
        results.append(row)
        print(json.dumps(row), flush=True)
        del t, x, c, gy, gl
        torch.cuda.empty_cache()
if OUT:
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(results, f, indent=1)
