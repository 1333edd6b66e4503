from torch import nn

from .wrappers import diffeq_wrapper

__all__ = ["SequentialDiffEq"]


class SequentialDiffEq(nn.Module):
    """A chain of layers, each either ``layer(x)`` or ``layer(t, x)``."""

    def __init__(self, *layers):
        super().__init__()
        self.layers = nn.ModuleList([diffeq_wrapper(layer) for layer in layers])

    def forward(self, t, x):
        for layer in self.layers:
            x = layer(t, x)
        return x
