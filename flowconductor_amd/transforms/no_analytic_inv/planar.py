"""Planar, Sylvester and radial flows (API of flowcon/transforms/no_analytic_inv/planar.py:13-214).

Planar: forward direction only, like the reference.  Radial: forward as the reference, plus a closed-form inverse the
reference does not have.  Each forward is one fused row-per-wavefront HIP kernel.

Sylvester: forward as the reference, plus an inverse the reference does not have (its ``inverse`` raises; a deliberate
extension, so that flows with a Sylvester layer can sample).  With ``v = Q^T z`` and ``c = Q^T y`` the map is
``c = v + R2 tanh(R1 v + b)`` with upper-triangular R1 / R2, so v follows by back substitution: for j = D-1 .. 0, with
``s = b_j + sum_{k>j} R1[j,k] v_k`` and ``t = c_j - sum_{k>j} R2[j,k] tanh(.)_k`` known from the later columns, v_j is the
root of the strictly increasing scalar function ``v + r2 tanh(r1 v + s) - t`` (slope in ``[1 - |r1 r2|, 1 + |r1 r2|]``,
``|r1 r2| < 1``), which lies in ``[t - |r2|, t + |r2|]`` and is found by a bracketed Newton search with a fixed cap of
evaluations.  ``z = Q v`` and logabsdet is minus the forward's expression at the solution.  Float32 device inputs with at
most 128 features take ``ops.sylvester_inverse`` (one ``fc_sylvester_inverse`` launch, one lane per row, between the two
applications of Q); CPU tensors, other dtypes and wider layers take the same algorithm as torch ops.  The inverse has no
gradient: a call that needs one raises and asks for ``torch.no_grad()``.
"""
import math

import numpy as np
import torch
from torch import nn
from torch.nn import init

from flowconductor_amd import _hip, ops, options
from flowconductor_amd.transforms.base import Transform
from flowconductor_amd.transforms.orthogonal import HouseholderSequence


class PlanarTransform(Transform):
    """f(z) = z + u_hat * tanh(w.z + b) with u constrained so that w.u_hat >= -1 (invertibility)."""

    def __init__(self, features: int = 2, num_iterations=25, lim=50):
        super().__init__()
        self.w = nn.Parameter(torch.randn(1, features).normal_(0, 0.1))
        self.b = nn.Parameter(torch.randn(1).normal_(0, 0.1))
        self.u = nn.Parameter(torch.randn(1, features).normal_(0, 0.1))

    _HIP_AUTOGRAD = True

    def forward(self, inputs, context=None):
        return ops.planar_autograd(inputs, self.w, self.get_constrained_u(), self.b)

    def forward_logabsdet(self, inputs, context=None):
        return self.forward(inputs, context)[1].unsqueeze(-1)

    def get_constrained_u(self):
        """u + (softplus(w.u) - 1 - w.u) * w / |w|^2   (a [1, D] host-side expression)."""
        wtu = torch.mm(self.u, self.w.T)
        m_wtu = -1 + torch.nn.functional.softplus(wtu)
        w_direction = self.w / (torch.norm(self.w, p=2, dim=1) ** 2)
        return self.u + (m_wtu - wtu) * w_direction


class SylvesterTransform(Transform):
    """z + Q R2 tanh(R1 Q^T z + b), Q from ``num_householder`` reflections, R1/R2 upper triangular with
    tanh-squashed diagonals.  Parameter names follow the reference (``upper_entries1/2``,
    ``log_upper_diag1/2``, ``Q_orth.q_vectors``, ``bias``).  ``device`` defaults to "cuda" as there."""

    def __init__(self, features: int = 2, num_householder=None, device="cuda"):
        super().__init__()
        self.n_diag_entries = features
        self.n_triangular_entries = ((features - 1) * features) // 2
        self.features = features
        if num_householder is None:
            num_householder = self.features
        self.num_householder = num_householder
        self.upper_indices = np.triu_indices(features, k=1)
        self.diag_indices = np.diag_indices(features)
        self.upper_entries1 = nn.Parameter(torch.zeros(self.n_triangular_entries))
        self.log_upper_diag1 = nn.Parameter(torch.zeros(features))
        self.upper_entries2 = nn.Parameter(torch.zeros(self.n_triangular_entries))
        self.log_upper_diag2 = nn.Parameter(torch.zeros(features))
        self.Q_orth = HouseholderSequence(features=features, num_transforms=self.num_householder)
        if device is not None and (torch.device(device).type != "cuda" or torch.cuda.is_available()):
            self.Q_orth = self.Q_orth.to(device=device)
        self.bias = nn.Parameter(torch.zeros(features))
        self._initialize()

    def _initialize(self):
        stdv = 1.0 / np.sqrt(self.features)
        init.uniform_(self.upper_entries1, -stdv, stdv)
        init.uniform_(self.upper_entries2, -stdv, stdv)
        init.uniform_(self.log_upper_diag1, -stdv, stdv)
        init.uniform_(self.log_upper_diag2, -stdv, stdv)
        init.constant_(self.bias, 0.0)

    def _create_R(self, entries, log_diag):
        upper = entries.new_zeros(self.features, self.features)
        upper[self.upper_indices[0], self.upper_indices[1]] = entries
        upper[self.diag_indices[0], self.diag_indices[1]] = torch.tanh(log_diag)
        return upper

    def _create_R1(self):
        return self._create_R(self.upper_entries1, self.log_upper_diag1)

    def _create_R2(self):
        return self._create_R(self.upper_entries2, self.log_upper_diag2)

    def dh_dx(self, x):
        return 1 - torch.tanh(x) ** 2

    def h(self, x):
        return torch.tanh(x)

    def _mm_weights(self):
        """(W1, W2, r_diag_prod) for the matrix-core kernel, recomputed only when a parameter changed."""
        params = (self.Q_orth.q_vectors, self.upper_entries1, self.log_upper_diag1, self.upper_entries2,
                  self.log_upper_diag2)
        return ops.memo(self, "mm_weights", ops.cache_key(*params),
                        lambda: ops.pack_sylvester(self.Q_orth.q_vectors, self._create_R1(), self._create_R2()))

    _HIP_AUTOGRAD = True

    def forward(self, inputs, context=None):
        if torch.is_grad_enabled() and (inputs.requires_grad or any(p.requires_grad for p in self.parameters())):
            return ops.sylvester_autograd(inputs, self.Q_orth.q_vectors, self._create_R1(), self._create_R2(), self.bias)
        with torch.no_grad():
            n = inputs.shape[0]
            if (inputs.dim() == 2 and inputs.is_cuda and ops.sylvester_mm_supported(n, self.features)
                    and options.get("sylvester_mm")):
                # batch-independent parameters: the Householder / triangular chains fold into two dense
                # [D, D] matrices and the batch goes through the matrix cores
                w1, w2, rdiag = self._mm_weights()
                body = n - n % ops.SYLVESTER_MM_ROWS
                y, lad = ops.sylvester_mm(inputs[:body], w1, w2, self.bias, rdiag)
                if body < n:
                    y2, lad2 = ops.sylvester(inputs[body:], self.Q_orth.q_vectors, self._create_R1(),
                                             self._create_R2(), self.bias)
                    y, lad = torch.cat((y, y2)), torch.cat((lad, lad2))
                return y, lad
            return ops.sylvester(inputs, self.Q_orth.q_vectors, self._create_R1(), self._create_R2(), self.bias)

    def _q_matrices(self):
        """The dense_mm weights of Q^T and Q (the reflections folded in float64), recomputed only when q changed."""
        q = self.Q_orth.q_vectors
        return ops.memo(self, "inverse_q", ops.cache_key(q),
                        lambda: tuple(ops.householder_matrix(q, reverse=r).T.float().contiguous() for r in (True, False)))

    def inverse(self, inputs, context=None):
        """The z with ``forward(z) == inputs`` and minus the forward's logabsdet there (the reference has no inverse):
        see the module docstring.  Runs without a graph; a call that needs a gradient is refused."""
        params = (self.Q_orth.q_vectors, self.upper_entries1, self.log_upper_diag1, self.upper_entries2,
                  self.log_upper_diag2, self.bias)
        _hip.require_no_grad(inputs, *params)
        if inputs.dim() != 2 or inputs.shape[1] != self.features:
            raise ValueError("SylvesterTransform: inputs must be [batch, %d], got %s" % (self.features, tuple(inputs.shape)))
        with torch.no_grad():
            n = inputs.shape[0]
            if inputs.is_cuda and inputs.dtype == torch.float32 and ops.sylvester_inverse_supported(n, self.features):
                dense = ops.sylvester_mm_supported(n, self.features) and options.get("sylvester_mm")
                return ops.sylvester_inverse(inputs, self.Q_orth.q_vectors, self._create_R1(), self._create_R2(), self.bias,
                                             q_matrices=self._q_matrices() if dense else None)
            return self._inverse_composition(inputs)

    def _inverse_composition(self, inputs):
        """The same back substitution as ``fc_sylvester_inverse`` in torch ops, in the inputs' dtype and on their device
        (vectorised over the batch, D sequential columns): CPU tensors, other dtypes, more features than the kernel takes."""
        kw = dict(dtype=inputs.dtype, device=inputs.device)
        q = self.Q_orth.q_vectors.to(**kw)
        r1 = self._create_R(self.upper_entries1.to(**kw), self.log_upper_diag1.to(**kw))     # tanh in that dtype too
        r2 = self._create_R(self.upper_entries2.to(**kw), self.log_upper_diag2.to(**kw))
        bias = self.bias.to(**kw)
        rd = torch.diagonal(r1) * torch.diagonal(r2)
        c = _reflect(inputs, q.flip(0))                     # Q^T y
        v, th = torch.zeros_like(c), torch.zeros_like(c)
        for j in range(self.features - 1, -1, -1):
            s = bias[j] + v[:, j + 1:] @ r1[j, j + 1:]
            t = c[:, j] - th[:, j + 1:] @ r2[j, j + 1:]
            v[:, j], th[:, j] = _solve_column(r1[j, j], r2[j, j], rd[j], s, t)
        logabsdet = -torch.log(1 + (1 - th ** 2) * rd).sum(-1)
        return _reflect(v, q), logabsdet                    # Q v


def _reflect(x, q_vectors):
    """The Householder reflections ``q_vectors [K, D]`` applied to the rows of ``x`` in index order."""
    for q in q_vectors:
        x = x - (x @ q).unsqueeze(-1) * ((2.0 / (q @ q)) * q)
    return x


def _solve_column(r1, r2, rd, s, t):
    """Roots v [N] of ``v + r2 tanh(r1 v + s) - t = 0`` and ``tanh(r1 v + s)`` there, for scalars r1, r2 (|r1 r2| < 1: the
    residual is strictly increasing, its root lies in ``[t - |r2|, t + |r2|]``) and batches s, t.

    Bracketed Newton: every evaluation moves one end of the bracket to the current point by the sign of the residual; the next
    point is the Newton iterate when it lies in the CLOSED bracket, else the midpoint.  An element stops when its residual
    is at the rounding level of its own evaluation, ``2 eps (|t| + |r2|)``, when the step no longer moves it, or at the
    cap of evaluations; a NaN element stops at once and stays NaN."""
    eps = torch.finfo(t.dtype).eps
    cap = 16 if t.dtype == torch.float32 else 48      # float32: the cap of fc_sylvester_inverse
    ar2 = r2.abs()
    tol = 2 * eps * (t.abs() + ar2)
    lo, hi = t - ar2, t + ar2
    v = t.clone()
    active = torch.ones_like(t, dtype=torch.bool)
    for it in range(cap):
        th = torch.tanh(r1 * v + s)
        g = (v + r2 * th) - t
        active = active & (g.abs() > tol)
        if it == cap - 1 or not bool(active.any()):
            break
        lo = torch.where(active & (g < 0), v, lo)
        hi = torch.where(active & (g > 0), v, hi)
        vn = v - g / (1 + rd * (1 - th * th))
        vn = torch.where((vn >= lo) & (vn <= hi), vn, 0.5 * (lo + hi))
        active = active & (vn != v)
        v = torch.where(active, vn, v)
    return v, th


class RadialTransform(Transform):
    """f(z) = z + beta_hat / (|alpha| + r) (z - z_0), r = |z - z_0|, beta_hat = softplus(beta) - |alpha| >= -|alpha|
    (https://arxiv.org/abs/1505.05770; parameters ``beta`` [1], ``alpha`` [1], ``z_0`` and the int64 buffer ``d`` as in the
    reference, whose checkpoints load).  One ``fc_radial`` launch per direction.

    Deliberate differences from the reference: ``inverse`` exists (the reference raises) -- r is the non-negative root of
    ``r^2 + (|alpha| + beta_hat - rho) r - |alpha| rho = 0`` for ``rho = |y - z_0|``; and a ``z_0`` must carry a leading
    batch dimension of 1 (``[1, D]``, or ``[1, ...]`` for a norm over all non-batch dimensions, flattened to rows of at most
    ``ops.MAX_ROW_FEATURES`` values) -- without it the reference's ``vector_norm(dim=[])`` is an accident, here a
    ``ValueError``."""

    _HIP_AUTOGRAD = True

    def __init__(self, features: int = 2, z_0=None):
        super().__init__()
        self.features = features
        self.register_buffer("d", torch.tensor(self.features))
        lim = 1.0 / self.features
        self.beta = nn.Parameter(torch.empty(1))
        init.uniform_(self.beta, -lim - 1.0, lim - 1.0)
        self.alpha = nn.Parameter(torch.empty(1))
        init.uniform_(self.alpha, -lim, lim)
        if z_0 is not None:
            if z_0.dim() < 2 or z_0.shape[0] != 1:
                raise ValueError("RadialTransform: z_0 must have shape [1, ...], got %s" % (tuple(z_0.shape),))
            if math.prod(z_0.shape[1:]) != features:      # the log-determinant's (d - 1) is the norm's dimension
                raise ValueError("RadialTransform: z_0 of shape %s does not hold %d features" % (tuple(z_0.shape), features))
            if math.prod(z_0.shape[1:]) > ops.MAX_ROW_FEATURES:
                raise ValueError("RadialTransform: z_0 with %d values per sample exceeds the %d supported by the row kernels"
                                 % (math.prod(z_0.shape[1:]), ops.MAX_ROW_FEATURES))
            self.z_0 = nn.Parameter(z_0)
        else:
            self.z_0 = nn.Parameter(torch.randn(self.features)[None])

    def _map(self, inputs, inverse):
        if inputs.shape[1:] != self.z_0.shape[1:]:
            raise ValueError("RadialTransform: inputs of shape %s do not match z_0 of shape %s"
                             % (tuple(inputs.shape), tuple(self.z_0.shape)))
        a = torch.abs(self.alpha)
        b = torch.log(1 + torch.exp(self.beta)) - a
        if inputs.dim() == 2:
            return ops.radial_autograd(inputs, self.z_0.reshape(-1), a, b, inverse=inverse)
        outputs, logabsdet = ops.radial_autograd(inputs.reshape(inputs.shape[0], -1), self.z_0.reshape(-1), a, b, inverse=inverse)
        return outputs.reshape(inputs.shape), logabsdet

    def forward(self, inputs, context=None):
        return self._map(inputs, False)

    def inverse(self, inputs, context=None):
        return self._map(inputs, True)
