"""Cholesky outer product: a bijection between lower-triangular matrices with a positive diagonal and symmetric
positive definite matrices (flowcon/transforms/matrix/cholesky.py; Conditional Matrix Flows, arXiv 2306.07255)."""
import numpy as np
import torch
from torch import nn

from flowconductor_amd import ops
from flowconductor_amd.transforms.base import Transform


class CholeskyOuterProduct(Transform):
    """``forward(L) = 0.5 (L L^T + (L L^T)^T)`` with ``logabsdet = N log 2 + sum_i (N - i) log L_ii``;
    ``inverse(A) = chol(A + eps I)`` with the negated logabsdet.

    For ``N <= ops.SPD_MAX_DIM`` (128) both directions are HIP kernels: ``fc_cholesky_outer`` (with its backward
    ``fc_cholesky_outer_backward``, over the full input as the reference's autograd has it) and ``fc_cholesky``.  With
    ``checkargs`` the reference's assertions are raised with its messages: not square, not lower triangular, a
    non-positive diagonal (forward); not symmetric, not positive definite (inverse).

    The reference tests positive semi-definiteness with ``torch.linalg.eig`` before factorising; here the pivot test
    inside the factorisation stands in for it (a pivot <= 0 raises the reference's assertion).  The two disagree only
    when an eigenvalue of ``A + eps I`` is within rounding of 0, where the reference's own ``torch.linalg.cholesky``
    raises as well.  Without ``checkargs`` a failed pivot raises ``torch.linalg.LinAlgError``, as
    ``torch.linalg.cholesky`` does.

    The reference's torch composition (``torch.bmm`` / ``torch.linalg.cholesky``) runs instead for ``N > 128``, and for
    the inverse when its input requires a gradient (the factorisation has no HIP backward)."""

    _HIP_AUTOGRAD = True

    def __init__(self, N, checkargs=True, eps=1e-6):
        super().__init__()
        self.eps = eps
        self.N = N
        self.eye = nn.Parameter(torch.diag_embed(torch.ones(self.N)).unsqueeze(0), requires_grad=False)
        self.powers = nn.Parameter(torch.arange(self.N, 0, -1).unsqueeze(0), requires_grad=False)
        self.checkargs = checkargs

    def _hip_path(self, inputs):
        if inputs.dim() != 3 or inputs.shape[-2] != inputs.shape[-1]:
            if self.checkargs:
                raise AssertionError(ops.MSG_NOT_SQUARE)
            raise ValueError("CholeskyOuterProduct expects [B, N, N] inputs, got %s" % (tuple(inputs.shape),))
        if inputs.shape[-1] != self.N:
            raise ValueError("CholeskyOuterProduct(N=%d) got %s matrices" % (self.N, tuple(inputs.shape[1:])))
        return self.N <= ops.SPD_MAX_DIM

    def _logabsdet(self, diagonal):
        return self.N * np.log(2.) + (self.powers * diagonal.log()).sum(-1)

    def forward(self, inputs, context=None):
        if self._hip_path(inputs):
            return ops.cholesky_outer(inputs, self.checkargs)
        # step-aside path, N > 128: the reference's composition
        if self.checkargs:
            self.check_pos_low_triang(inputs)
        outputs = torch.bmm(inputs, inputs.mT)
        outputs = 0.5 * (outputs + outputs.mT)
        return outputs, self._logabsdet(torch.diagonal(inputs, dim1=-2, dim2=-1))

    def inverse(self, inputs, context=None):
        wants_grad = torch.is_grad_enabled() and inputs.requires_grad
        if self._hip_path(inputs) and not wants_grad:
            return ops.cholesky(inputs, self.eps, self.checkargs)
        # the reference's composition: N > 128, or a gradient with respect to the SPD input is due
        inputs_jitter = inputs + self.eye * self.eps
        if self.checkargs:
            self.check_pos_def(inputs_jitter)
        outputs = torch.linalg.cholesky(inputs_jitter, upper=False)
        return outputs, -self._logabsdet(torch.diagonal(outputs, dim1=-2, dim2=-1))

    def check_pos_low_triang(self, inputs):
        assert inputs.shape[-2] == inputs.shape[-1], ops.MSG_NOT_SQUARE
        upper_indices = np.triu_indices(self.N, k=1)
        assert torch.all(inputs[:, upper_indices[0], upper_indices[1]] == 0.), ops.MSG_NOT_LOWER_TRIANGULAR
        assert torch.all(torch.diagonal(inputs, dim1=-2, dim2=-1) > 0), ops.MSG_DIAGONAL_NONPOSITIVE

    def check_pos_def(self, inputs):
        assert torch.all(inputs == inputs.mT), ops.MSG_NOT_SYMMETRIC
        assert torch.all(torch.linalg.eig(inputs)[0].real >= 0), ops.MSG_NOT_POSITIVE_DEFINITE
