"""QR-parameterised linear transform: class name, constructor arguments, parameter names and shapes of
flowcon/transforms/qr.py:11-114 (reference checkpoints load); the triangular product runs in ``fc_linear``, the
reflections in ``fc_householder``, wide no-grad batches as one matrix-core product."""
import torch
from torch import nn

from flowconductor_amd import ops
from flowconductor_amd.transforms.linear import Linear
from flowconductor_amd.transforms.orthogonal import HouseholderSequence
from flowconductor_amd.transforms.svd import folded_mm, reflect, wide_rows


class QRLinear(Linear):
    """``y = Q (R x) + bias`` with ``Q = orthogonal`` a Householder sequence of ``num_householder`` reflections and ``R``
    upper triangular, ``diag R = exp(log_upper_diag) > 0``.

    Parameters: ``upper_entries`` (the strict upper triangle, row-major, ``D (D - 1) / 2`` values), ``log_upper_diag`` [D],
    ``bias`` [D]."""

    _HIP_AUTOGRAD = True

    def __init__(self, features, num_householder, using_cache=False):
        super().__init__(features, using_cache)
        self.upper_entries = nn.Parameter(torch.zeros(features * (features - 1) // 2))
        self.log_upper_diag = nn.Parameter(torch.zeros(features))
        self.orthogonal = HouseholderSequence(features=features, num_transforms=num_householder)
        self._triangles = {}      # device -> index tensors of the strict upper triangle (row-major, the storage order)
        bound = features ** -0.5
        with torch.no_grad():
            self.upper_entries.uniform_(-bound, bound)
            self.log_upper_diag.uniform_(-bound, bound)
            self.bias.zero_()

    def _create_upper(self):
        """Dense R from the stored triangle (differentiable: index_put of the parameters)."""
        d = self.features
        dev = self.upper_entries.device
        if dev not in self._triangles:
            self._triangles[dev] = tuple(torch.triu_indices(d, d, offset=1, device=dev))
        return torch.diag(torch.exp(self.log_upper_diag)).index_put(self._triangles[dev], self.upper_entries)

    def logabsdet(self):
        return torch.sum(self.log_upper_diag)

    # -- dense forms ------------------------------------------------------------------------------------------------
    def _fold(self, inverse):
        """float64 ``W = Q R`` (the columns of R through the reflections) or ``W^-1 = R^-1 Q^T`` (the columns of Q^T,
        i.e. the reversed reflections applied to the identity's rows and transposed, through one triangular solve)."""
        upper, q = self._create_upper().double(), self.orthogonal.q_vectors.double()
        if not inverse:
            return reflect(upper.t(), q).t()
        eye = torch.eye(self.features, dtype=torch.float64, device=upper.device)
        return torch.linalg.solve_triangular(upper, reflect(eye, q, reverse=True).t(), upper=True)

    def weight(self):
        """Formed in float64 and rounded once."""
        return self._fold(False).to(self.bias.dtype)

    def weight_inverse(self):
        """The identity is built on the parameters' device (the reference builds it on the CPU, qr.py:103, and fails for
        a module on a GPU)."""
        return self._fold(True).to(self.bias.dtype)

    # -- the map ----------------------------------------------------------------------------------------------------
    def _needs_grad(self, inputs):
        return torch.is_grad_enabled() and (inputs.requires_grad or any(p.requires_grad for p in self.parameters()))

    def _composition(self, inputs, inverse):
        """The reference's own composition (qr.py:45-82) on the device, differentiable as it stands: the widths above
        ``ops.MAX_ROW_FEATURES``, where no row kernel runs."""
        upper, q = self._create_upper(), self.orthogonal.q_vectors
        if not inverse:
            return reflect(inputs @ upper.t(), q) + self.bias
        outputs = reflect(inputs - self.bias, q, reverse=True)
        return torch.linalg.solve_triangular(upper, outputs.t(), upper=True).t()

    def _rows(self, inputs, inverse):
        """No-grad row kernels: the triangular product (or back substitution) in ``fc_linear``, the reflections in
        ``fc_householder``; the bias rides in the first kernel of the inverse."""
        upper, q = self._create_upper(), self.orthogonal.q_vectors
        if not inverse:
            outputs = ops.householder(ops.upper_linear(inputs, upper), q)
            return ops.pointwise_affine(outputs, torch.ones(1, device=inputs.device), self.bias)
        outputs = ops.pointwise_affine(inputs, torch.ones(1, device=inputs.device), self.bias, inverse=True)
        return ops.upper_linear(ops.householder(outputs, q, reverse=True), upper, inverse=True)

    def _map(self, inputs, inverse):
        if self.features > ops.MAX_ROW_FEATURES:
            outputs = self._composition(inputs, inverse)
        elif self._needs_grad(inputs):      # training: the kernels behind their autograd nodes
            upper, q = self._create_upper(), self.orthogonal.q_vectors
            if not inverse:
                outputs, _ = ops.householder_autograd(ops.upper_linear_autograd(inputs, upper), q)
                outputs = outputs + self.bias
            else:
                outputs, _ = ops.householder_autograd(inputs - self.bias, q, reverse=True)
                outputs = ops.upper_linear_autograd(outputs, upper, inverse=True)
        else:
            with torch.no_grad():
                if wide_rows(inputs, self.features):
                    outputs = folded_mm(self, inputs, inverse, self._fold, lambda x: self._rows(x, inverse))
                else:
                    outputs = self._rows(inputs, inverse)
        logabsdet = self.logabsdet()
        return outputs, (-logabsdet if inverse else logabsdet) * outputs.new_ones(outputs.shape[0])

    def forward_no_cache(self, inputs):
        """``orthogonal(R x) + bias``; logabsdet = sum log_upper_diag for every row."""
        return self._map(inputs, False)

    def inverse_no_cache(self, inputs):
        """``R^-1 orthogonal^-1(x - bias)``: the bias comes off first, then the reversed reflections, then the back
        substitution."""
        return self._map(inputs, True)
