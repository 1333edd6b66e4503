"""Float64 truth for the Sylvester-inverse tests, written independently of the package's back substitution: the forward
map is the oracle's, the inverse a plain bisection of every scalar equation run until the bracket stops shrinking."""
import copy

import numpy as np
import torch

from oracle import torch_oracle as O


def params64(t):
    """(q, R1, R2, bias) of a SylvesterTransform as float64 CPU tensors."""
    t64 = copy.deepcopy(t).cpu().double()
    with torch.no_grad():
        return (t64.Q_orth.q_vectors.detach().clone(), t64._create_R1().detach().clone(),
                t64._create_R2().detach().clone(), t64.bias.detach().clone())


def forward64(p, z):
    """(y, logabsdet) of the oracle's forward on float64 parameters ``p = params64(t)``."""
    with torch.no_grad():
        return O.sylvester_forward(z.detach().cpu().double(), *p)


def inverse64(p, y):
    """z [N, D] float64 with forward64(p, z) == y to rounding: D back-substitution steps, each a bisection of
    v + r2 tanh(r1 v + s) = t over [t - |r2|, t + |r2|] (the function is increasing: |r1 r2| < 1), 80 halvings."""
    q, r1, r2, bias = p
    y = y.detach().cpu().double()
    d = y.shape[1]
    c = O.householder_apply(y, q.flip(-2))
    v = torch.zeros_like(c)
    th = torch.zeros_like(c)
    for j in range(d - 1, -1, -1):
        s = bias[j] + v[:, j + 1:] @ r1[j, j + 1:]
        t = c[:, j] - th[:, j + 1:] @ r2[j, j + 1:]
        a, b = r1[j, j], r2[j, j]
        lo, hi = t - b.abs(), t + b.abs()
        for _ in range(80):
            mid = 0.5 * (lo + hi)
            below = mid + b * torch.tanh(a * mid + s) < t
            lo = torch.where(below, mid, lo)
            hi = torch.where(below, hi, mid)
        v[:, j] = 0.5 * (lo + hi)
        th[:, j] = torch.tanh(a * v[:, j] + s)
    return O.householder_apply(v, q)


def sigma_min(p, z):
    """Smallest singular value over the batch of the float64 Jacobian I + Q R2 diag(1 - tanh^2) R1 Q^T at ``z``."""
    q, r1, r2, bias = p
    z = z.detach().cpu().double()
    d = z.shape[1]
    eye = torch.eye(d, dtype=torch.float64)
    qm = O.householder_apply(eye, q.flip(-2))          # rows as vectors: x @ qm is Q^T x, so qm = Q
    pre = O.householder_apply(z, q.flip(-2)) @ r1.T + bias
    h = 1 - torch.tanh(pre) ** 2
    jac = eye + qm @ (r2 * h.unsqueeze(-2)) @ r1 @ qm.T     # [N, D, D]
    return float(torch.linalg.svdvals(jac).min())


def scale_of(expected):
    e = expected.detach().cpu().double() if isinstance(expected, torch.Tensor) else torch.as_tensor(np.asarray(expected))
    return max(1.0, float(e.abs().max())) if e.numel() else 1.0


def bound(expected, floor):
    """The rule of tests/test_gpu_golden.py: 1e-5 * max(1, max|expected|) + 4 * floor."""
    return 1e-5 * scale_of(expected) + 4.0 * floor


def randomize(t, sigma, seed):
    """Every parameter entry ~ N(0, sigma), as tests/golden/cases.py draws them."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for prm in t.parameters():
            prm.copy_(torch.randn(prm.shape, generator=g) * sigma)
    return t
