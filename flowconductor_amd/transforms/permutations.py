"""Feature permutations (same classes, constructor arguments and ``_permutation`` buffer as
flowcon/transforms/permutations.py:10-64).  The gather itself is the ``fc_permute`` HIP kernel: bit-exact, zero
log-determinant."""
import numpy as np
import torch

from flowconductor_amd import ops
from flowconductor_amd.transforms.base import Transform
from flowconductor_amd.utils import typechecks as check


def _need_feature_count(features):
    if not check.is_positive_int(features):
        raise ValueError("Number of features must be a positive integer.")
    return features


class Permutation(Transform):
    """Reorders ``inputs`` along ``dim`` by a fixed index vector; the inverse applies the argsort of that vector."""

    def __init__(self, permutation, dim=1):
        index = torch.as_tensor(permutation)
        if index.dim() != 1:
            raise ValueError("Permutation must be a 1D tensor.")
        if not check.is_positive_int(dim):
            raise ValueError("dim must be a positive integer.")
        super().__init__()
        self._dim = dim
        self.register_buffer("_permutation", index)

    @property
    def _inverse_permutation(self):
        # recomputed per call like the reference (:23-25): the buffer may have been replaced by load_state_dict
        return torch.argsort(self._permutation)

    def _gather(self, inputs, index):
        dim = self._dim
        if inputs.dim() <= dim:
            raise ValueError("No dimension {} in inputs.".format(dim))
        if inputs.shape[dim] != index.numel():
            raise ValueError("Dimension {} in inputs must be of size {}.".format(dim, index.numel()))
        return ops.permute(inputs, index, dim), inputs.new_zeros(inputs.shape[0])

    def _index32(self, device):
        """The permutation as the int32 device vector the kernel takes, converted once per buffer version."""
        perm = self._permutation
        return ops.memo(self, "index32", ops.cache_key(perm, extra=(device,)),
                        lambda: perm.to(device=device, dtype=torch.int32).contiguous())

    def _apply_accumulate(self, inputs, context, inverse, total):
        """CompositeTransform fast path: logabsdet is identically zero -- nothing to allocate or add (two tiny launches per
        permutation layer of a small-batch flow)."""
        if inverse or self._dim != 1 or inputs.dim() != 2 or not inputs.is_cuda:
            outputs, _ = self.inverse(inputs, context) if inverse else self.forward(inputs, context)
            return outputs
        if inputs.shape[1] != self._permutation.numel():
            raise ValueError("Dimension {} in inputs must be of size {}.".format(1, self._permutation.numel()))
        return ops.permute(inputs, self._index32(inputs.device), 1)

    def forward(self, inputs, context=None):
        return self._gather(inputs, self._permutation)

    def inverse(self, inputs, context=None):
        return self._gather(inputs, self._inverse_permutation)


class RandomPermutation(Permutation):
    """A permutation drawn once at construction (from torch's global generator, as the reference does)."""

    def __init__(self, features, dim=1):
        super().__init__(torch.randperm(_need_feature_count(features)), dim)


class ReversePermutation(Permutation):
    """Feature order reversed."""

    def __init__(self, features, dim=1):
        count = _need_feature_count(features)
        super().__init__(torch.arange(count - 1, -1, -1), dim)


class FillTriangular(Transform):
    """``[B, d] -> [B, m, m]`` with d = m (m + 1) / 2: the entries fill the lower triangle in ``np.tril_indices(m)``
    order, zeros above (flowcon/transforms/permutations.py:67-113).  Zero logabsdet; the inverse gathers back.  Both
    directions are the bit-exact ``fc_tril_pack`` HIP kernel, each the other's backward."""

    _HIP_AUTOGRAD = True

    def __init__(self, features: int = None, matrix_dimension: int = None):
        super().__init__()
        if (features is not None) and (matrix_dimension is None):
            self.features = features
            self.matrix_dim = self.calc_matrix_dimension(features)
        elif (features is None) and (matrix_dimension is not None):
            self.features = self.calc_n_ltri(matrix_dimension)
            self.matrix_dim = matrix_dimension
        else:
            raise ValueError("Provide either 'features' or 'full_matrix_dimension', but not both.")
        self.lower_indices = np.tril_indices(self.matrix_dim, k=0)

    @staticmethod
    def calc_matrix_dimension(n_ltri_entries):
        assert n_ltri_entries > 0, f"Dimension must be positive, but is {n_ltri_entries}"
        temp = 1 + 8 * n_ltri_entries
        assert np.square(
            np.floor(np.sqrt(temp))) == temp, "invalid dimension: can't be mapped to lower triangular matrix"
        return int((-1 + np.floor(np.sqrt(temp))) // 2)

    @staticmethod
    def calc_n_ltri(matrix_dim):
        return int((matrix_dim * (matrix_dim + 1)) / 2)

    def forward(self, inputs, context=None):
        assert inputs.shape[-1] == self.features
        outputs = ops.fill_triangular(inputs, self.matrix_dim)
        return outputs, inputs.new_zeros(inputs.shape[0])

    def inverse(self, inputs, context=None):
        assert inputs.shape[-2:] == (self.matrix_dim, self.matrix_dim)
        outputs = ops.tril_gather(inputs)
        return outputs, inputs.new_zeros(inputs.shape[0])
