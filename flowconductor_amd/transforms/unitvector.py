"""``UnitVector``: the bijection between R^d and the unit sphere in R^(d+1) by the inverse stereographic projection (class
name, constructor argument and state-dict key of flowcon/transforms/unitvector.py:5-57); both directions are one
``fc_unit_vector`` launch."""
import torch

from flowconductor_amd import ops
from flowconductor_amd.transforms.base import Transform


class UnitVector(Transform):
    """forward: ``y = (2 x, |x|^2 - 1) / (|x|^2 + 1)`` on the sphere, ``logabsdet = d (log 2 - log1p(|x|^2))`` (half the
    log-determinant of J^T J); inverse: ``x = y[:d] / (1 - y[d])`` with the negated value at the recovered ``x``.

    ``dim_sphere`` is a float ``nn.Parameter`` as in the reference: it is the state-dict key, it takes no part in the
    arithmetic and its gradient stays ``None``.

    Deliberate differences from the reference: a wrong last dimension raises ``ValueError`` (there a bare ``assert``); the
    inverse's domain check ``| |y|^2 - 1 | <= 1e-4`` holds for EVERY row and raises ``InputOutsideDomain`` through the device
    error word -- the reference tests only the batch maximum of ``|y|^2``, so it lets a row far inside the sphere pass when
    another row sits on the sphere.  Every batch the reference rejects is rejected here too."""

    _HIP_AUTOGRAD = True

    def __init__(self, features):
        super().__init__()
        if features + 1 > ops.MAX_ROW_FEATURES:
            raise ValueError("UnitVector: %d + 1 features exceed the %d supported by the row kernels"
                             % (features, ops.MAX_ROW_FEATURES))
        self.dim_Rd = features
        self.dim_sphere = torch.nn.Parameter(torch.tensor(features + 1, dtype=torch.float32))

    def _map(self, inputs, inverse):
        width = self.dim_Rd + (1 if inverse else 0)
        if inputs.shape[-1] != width:
            raise ValueError("UnitVector: the last dimension of the inputs must be %d, got shape %s"
                             % (width, tuple(inputs.shape)))
        if inputs.dim() == 2:
            return ops.unit_vector_autograd(inputs, self.dim_Rd, inverse=inverse)
        # more than one leading dimension: flattened to rows, the logabsdet stays flat
        outputs, logabsdet = ops.unit_vector_autograd(inputs.reshape(-1, width), self.dim_Rd, inverse=inverse)
        return outputs.reshape(inputs.shape[:-1] + (outputs.shape[-1],)), logabsdet

    def forward(self, inputs, context=None):
        """R^d to the surface of the sphere."""
        return self._map(inputs, False)

    def inverse(self, inputs, context=None):
        """Surface of the sphere to R^d."""
        return self._map(inputs, True)
