"""Truth for the per-sample backward kernels (fc_linear_per_sample_backward, fc_householder_backward_per_sample,
fc_planar_backward_per_sample): the forward maps as differentiable torch expressions (walked by torch.autograd in float64
for the truth, in float32 for the rounding floor of the tolerance) and the written-out gradient formulas the kernels
implement, restated in torch.  test_per_sample_backward_host.py shows on the CPU that the two agree."""
import torch
from torch.nn import functional as F

LINEAR_SHAPES = [(37, 2), (37, 5), (50, 16), (37, 17), (21, 64), (21, 65), (9, 130), (5, 260)]
HOUSEHOLDER_SHAPES = [(5, 5), (16, 3), (17, 17), (64, 8), (100, 11), (200, 9), (260, 2)]
PLANAR_WIDTHS = [2, 7, 16, 30, 64, 100, 130, 300]
OFFDIAG_SCALE, EPS = 0.3, 1e-3


def lower_upper(m, sp, eps):
    """L = sp tril(M, -1) + I, U = sp triu(M, 1) + diag(softplus(diag M) + eps) and the diagonal dg."""
    d = m.shape[-1]
    dg = F.softplus(torch.diagonal(m, dim1=-2, dim2=-1)) + eps
    lower = sp * torch.tril(m, -1) + torch.eye(d, dtype=m.dtype)
    upper = sp * torch.triu(m, 1) + torch.diag_embed(dg)
    return lower, upper, dg


def linear_forward(x, m, mode, sp, eps):
    """The four modes of fc_linear_per_sample as torch expressions -> (outputs, logabsdet)."""
    col = x.unsqueeze(-1)
    if mode == 0:
        return (m @ col).squeeze(-1), x.new_zeros(x.shape[0])
    if mode == 1:
        return (m.transpose(-2, -1) @ col).squeeze(-1), x.new_zeros(x.shape[0])
    lower, upper, dg = lower_upper(m, sp, eps)
    if mode == 2:
        return (lower @ (upper @ col)).squeeze(-1), dg.log().sum(-1)
    t = torch.linalg.solve_triangular(lower, col, upper=False, unitriangular=True)
    return torch.linalg.solve_triangular(upper, t, upper=True).squeeze(-1), -dg.log().sum(-1)


def autograd_grads(forward, operands, gy, gl, dtype):
    """Gradients of ``(y * gy).sum() + (lad * gl).sum()`` wrt every operand, by torch.autograd in ``dtype`` on the CPU."""
    leaves = [t.detach().to(dtype).requires_grad_(True) for t in operands]
    y, lad = forward(*leaves)
    loss = (y * gy.to(dtype)).sum()
    if lad is not None and lad.requires_grad:
        loss = loss + (lad * gl.to(dtype)).sum()
    grads = torch.autograd.grad(loss, leaves, allow_unused=True)
    return [torch.zeros_like(t) if g is None else g for g, t in zip(grads, leaves)]


def linear_truth(x, m, gy, gl, mode, dtype, sp=OFFDIAG_SCALE, eps=EPS):
    """(gx, gM, g_sp rows) of ``linear_forward`` by autograd in ``dtype``; the offdiag scale is a leaf per row [N, 1, 1],
    so its gradient is each row's share of the gradient of the shared scalar."""
    scale = torch.full((x.shape[0], 1, 1), sp, dtype=dtype)
    gx, gm, gs = autograd_grads(lambda a, b, s: linear_forward(a, b, mode, s, eps), (x, m, scale), gy, gl, dtype)
    return gx, gm, gs


def _mode2_parameter_grads(x, gy, gl, m, sp, dg):
    """gM and the per-row g_sp of y = L U x, lad = sum log dg, for upstream (gy, gl)."""
    d = m.shape[-1]
    lo = torch.tril(torch.ones(d, d, dtype=m.dtype), -1)
    hi = torch.triu(torch.ones(d, d, dtype=m.dtype), 1)
    upper = sp * torch.triu(m, 1) + torch.diag_embed(dg)
    lower = sp * torch.tril(m, -1) + torch.eye(d, dtype=m.dtype)
    t = (upper @ x.unsqueeze(-1)).squeeze(-1)
    g_t = (lower.transpose(-2, -1) @ gy.unsqueeze(-1)).squeeze(-1)
    below = gy.unsqueeze(-1) * t.unsqueeze(-2)          # gy_i t_j
    above = g_t.unsqueeze(-1) * x.unsqueeze(-2)         # g_t_i x_j
    sig = torch.sigmoid(torch.diagonal(m, dim1=-2, dim2=-1))
    gm = sp * below * lo + sp * above * hi + torch.diag_embed((g_t * x + gl.unsqueeze(-1) / dg) * sig)
    g_sp = (m * below * lo).sum((-2, -1)) + (m * above * hi).sum((-2, -1))
    gx = (upper.transpose(-2, -1) @ g_t.unsqueeze(-1)).squeeze(-1)
    return gx, gm, g_sp


def linear_backward_formula(x_or_out, gy, gl, m, mode, sp=OFFDIAG_SCALE, eps=EPS):
    """What fc_linear_per_sample_backward computes -> (grad_in, grad_m, grad_sp_rows)."""
    zeros = x_or_out.new_zeros(x_or_out.shape[0])
    if mode == 0:
        return (m.transpose(-2, -1) @ gy.unsqueeze(-1)).squeeze(-1), gy.unsqueeze(-1) * x_or_out.unsqueeze(-2), zeros
    if mode == 1:
        return (m @ gy.unsqueeze(-1)).squeeze(-1), x_or_out.unsqueeze(-1) * gy.unsqueeze(-2), zeros
    lower, upper, dg = lower_upper(m, sp, eps)
    if mode == 2:
        return _mode2_parameter_grads(x_or_out, gy, gl, m, sp, dg)
    # mode 3: x_or_out is the OUTPUT x = U^-1 L^-1 y; gin = L^-T U^-T gy
    s = torch.linalg.solve_triangular(upper.transpose(-2, -1), gy.unsqueeze(-1), upper=False)
    gin = torch.linalg.solve_triangular(lower.transpose(-2, -1), s, upper=True, unitriangular=True).squeeze(-1)
    _, gm, g_sp = _mode2_parameter_grads(x_or_out, -gin, -gl, m, sp, dg)
    return gin, gm, g_sp


def householder_forward(x, q, reverse):
    """K per-sample reflections, q [N, K, D], in index order or reversed -> (outputs, None)."""
    out = x
    order = range(q.shape[1] - 1, -1, -1) if reverse else range(q.shape[1])
    for k in order:
        qk = q[:, k]
        out = out - (out * qk).sum(-1, keepdim=True) * ((2.0 / (qk * qk).sum(-1, keepdim=True)) * qk)
    return out, None


def householder_backward_formula(y, gy, q, reverse):
    """What fc_householder_backward_per_sample computes from the saved OUTPUT -> (gx, gq)."""
    k_count = q.shape[1]
    v, g, gq = y, gy, torch.zeros_like(q)
    for p in range(k_count - 1, -1, -1):
        idx = k_count - 1 - p if reverse else p
        qk = q[:, idx]
        alpha = 2.0 / (qk * qk).sum(-1, keepdim=True)
        a_out, c = (v * qk).sum(-1, keepdim=True), (g * qk).sum(-1, keepdim=True)
        a = -a_out
        v = v - a_out * alpha * qk
        gq[:, idx] = -alpha * (c * v + a * g) + alpha * alpha * (a * c) * qk
        g = g - c * alpha * qk
    return g, gq


def planar_forward(x, w, u, b):
    """Per-sample planar flow from u_hat on -> (outputs, logabsdet)."""
    t = torch.tanh((x * w).sum(-1) + b)
    psi = 1 + (1 - t * t) * (u * w).sum(-1)
    return x + u * t.unsqueeze(-1), torch.log(1e-7 + psi.abs())


def planar_backward_formula(x, gy, gl, w, u, b):
    """What fc_planar_backward_per_sample computes -> (gx, gw, gu, gb)."""
    uw = (u * w).sum(-1)
    t = torch.tanh((x * w).sum(-1) + b)
    dt = 1 - t * t
    psi = 1 + dt * uw
    dl = gl * torch.where(psi >= 0, 1.0, -1.0) / (1e-7 + psi.abs())
    g_t = (gy * u).sum(-1) - dl * (2 * t * uw)
    g_a = g_t * dt
    c = dl * dt
    col = lambda v: v.unsqueeze(-1)      # noqa: E731
    return gy + col(g_a) * w, col(g_a) * x + col(c) * u, col(t) * gy + col(c) * w, g_a


def linear_case(n, d, seed):
    """Operands of one kernel-level linear case (the scaling of test_per_sample_lu_round_trip)."""
    gen = torch.Generator().manual_seed(seed)
    m = torch.randn(n, d, d, generator=gen) / d ** 0.5
    x, gy, gl = torch.randn(n, d, generator=gen), torch.randn(n, d, generator=gen), torch.randn(n, generator=gen)
    return x, m, gy, gl
