from inspect import signature

from torch import nn

__all__ = ["diffeq_wrapper", "reshape_wrapper"]


class DiffEqWrapper(nn.Module):
    """Gives a module that takes ``(y)`` or ``(t, y)`` the signature ``(t, y)``."""

    def __init__(self, module):
        super().__init__()
        self.module = module
        arity = len(signature(self.module.forward).parameters)
        if arity not in (1, 2):
            raise ValueError("Differential equation needs to either take (t, y) or (y,) as input.")
        self._takes_time = arity == 2

    def forward(self, t, y):
        return self.module(t, y) if self._takes_time else self.module(y)

    def __repr__(self):
        return repr(self.module)


def diffeq_wrapper(layer):
    return DiffEqWrapper(layer)


class ReshapeDiffEq(nn.Module):
    """Runs a ``(t, x)`` net on rows viewed as ``input_shape`` and flattens the result again."""

    def __init__(self, input_shape, net):
        super().__init__()
        assert len(signature(net.forward).parameters) == 2, "use diffeq_wrapper before reshape_wrapper."
        self.input_shape = input_shape
        self.net = net

    def forward(self, t, x):
        batch = x.shape[0]
        return self.net(t, x.view(batch, *self.input_shape)).view(batch, -1)

    def __repr__(self):
        return repr(self.net)


def reshape_wrapper(input_shape, layer):
    return ReshapeDiffEq(input_shape, layer)
