from flowconductor_amd.nn.nets.mlp import MLP  # noqa: F401
from flowconductor_amd.nn.nets.resnet import (  # noqa: F401
    ConvResidualBlock,
    ConvResidualNet,
    ResidualBlock,
    ResidualNet,
)
from flowconductor_amd.nn.nets import activations  # noqa: F401
from flowconductor_amd.nn.nets.invertible_densenet import (  # noqa: F401
    DenseNet,
    InputConditionalDenseNet,
    LastLayerConditionalDenseNet,
    MixedConditionalDenseNet,
    MultiplicativeAndInputConditionalDenseNet,
    MultiplicativeConditionalDenseNet,
)
