from flowconductor_amd.nn import nde, nets  # noqa: F401
from flowconductor_amd.nn.nets import ConvResidualBlock, ConvResidualNet  # noqa: F401
