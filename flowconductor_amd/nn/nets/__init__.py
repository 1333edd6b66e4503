from flowconductor_amd.nn.nets.mlp import MLP  # noqa: F401
from flowconductor_amd.nn.nets.resnet import (  # noqa: F401
    ConvResidualBlock,
    ConvResidualNet,
    ResidualBlock,
    ResidualNet,
)
