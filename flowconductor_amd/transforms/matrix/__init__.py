"""Layers of flows on symmetric positive definite matrices (flowcon/transforms/matrix/)."""
from flowconductor_amd.transforms.matrix.diagonal import (  # noqa: F401
    TransformDiagonal,
    TransformDiagonalExponential,
    TransformDiagonalSoftplus,
)
from flowconductor_amd.transforms.matrix.cholesky import CholeskyOuterProduct  # noqa: F401
