"""Element-wise transforms of a matrix diagonal (flowcon/transforms/matrix/diagonal.py).  The diagonal is read out
and put back by the bit-exact ``fc_matrix_diag`` HIP kernel (with its backward); the inner transform runs on the
``[B, m]`` diagonal as it is."""
import numpy as np
import torch
from torch import nn

from flowconductor_amd import ops
from flowconductor_amd.transforms.base import CompositeTransform, Transform
from flowconductor_amd.transforms.linear import ScalarScale, ScalarShift
from flowconductor_amd.transforms.nonlinearities import Exp, Sigmoid, Softplus

fancy_exp_transform = CompositeTransform([Sigmoid(),
                                          ScalarScale(scale=80., trainable=False),
                                          Exp(),
                                          ScalarShift(1e-5, trainable=False)])

fancy_softplus_transform = CompositeTransform([Sigmoid(),
                                               ScalarScale(scale=80., trainable=False),
                                               Softplus(),
                                               ScalarShift(1e-5, trainable=False)])


class TransformDiagonal(Transform):
    """Applies ``diag_transformation`` to the diagonal of ``[B, N, N]`` matrices and returns a copy with the new
    diagonal; logabsdet is the inner transform's.  The default ``Exp()`` is one instance shared by every layer built
    with the default, as in the reference.  Gradients flow through the diagonal read-out and put-back kernels; the
    inner transform's own backward decides whether its step trains (one without a backward kernel raises)."""

    _HIP_AUTOGRAD = True

    def __init__(self, N, diag_transformation: Transform = Exp()):
        super().__init__()
        self.N = N
        self.diag_indices = np.diag_indices(self.N)
        self.diag_mask = nn.Parameter(torch.diag_embed(torch.ones(1, self.N)), requires_grad=False)
        self.diag_transform = diag_transformation

    def _map(self, inputs, inverse):
        diagonal = ops.matrix_diagonal(inputs)
        inner = self.diag_transform.inverse if inverse else self.diag_transform
        transformed_diag, logabsdet_diag = inner(diagonal)
        outputs = ops.matrix_replace_diagonal(inputs, transformed_diag)
        return outputs, logabsdet_diag

    def forward(self, inputs, context=None):
        return self._map(inputs, False)

    def inverse(self, inputs, context=None):
        return self._map(inputs, True)


class TransformDiagonalExponential(TransformDiagonal):
    def __init__(self, N, eps=1e-5):
        super().__init__(N=N, diag_transformation=CompositeTransform([Exp(),
                                                                      ScalarShift(eps, trainable=False)]))


class TransformDiagonalSoftplus(TransformDiagonal):
    def __init__(self, N, eps=1e-5):
        super().__init__(N=N, diag_transformation=CompositeTransform([Softplus(),
                                                                      ScalarShift(eps, trainable=False)]))
