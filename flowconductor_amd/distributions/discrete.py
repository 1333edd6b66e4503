"""Discrete distributions (API of flowcon/distributions/discrete.py:10-72).

``_log_prob`` is one HIP row kernel with a one-launch backward (``ops.bernoulli_log_prob``); ``_sample`` compares uniform
noise with ``sigmoid(logits)`` in one kernel that reads each context row's logits in place (``ops.bernoulli_sample``).
"""
import torch

from flowconductor_amd import ops
from flowconductor_amd.distributions.base import Distribution
from flowconductor_amd.utils import torchutils


class ConditionalIndependentBernoulli(Distribution):
    """An independent Bernoulli whose parameters are functions of a context.

    Unlike the reference, whose ``_sample`` draws its noise on the CPU whatever the device of the logits (and so fails
    with device tensors), ``_sample`` here draws ``torch.rand`` on the logits' device and returns float32
    ``[context_size, num_samples, *shape]`` there."""

    def __init__(self, shape, context_encoder=None):
        """``shape``: the event shape of one input (list, tuple or ``torch.Size``).  ``context_encoder``: a callable (an
        ``nn.Module`` is registered, so its parameters train and appear in the ``state_dict``) that maps a context batch to
        logits with ``prod(shape)`` values per row; ``None`` stands for the identity."""
        super().__init__()
        self._shape = torch.Size(shape)
        self._context_encoder = _identity if context_encoder is None else context_encoder

    def _compute_params(self, context):
        """Logits ``[N, *shape]`` of the context rows."""
        if context is None:
            raise ValueError("Context can't be None.")
        logits = self._context_encoder(context)
        if logits.shape[0] != context.shape[0]:
            raise RuntimeError("The batch dimension of the parameters is inconsistent with the input.")
        return logits.reshape(logits.shape[0], *self._shape)

    def _log_prob(self, inputs, context):
        if inputs.shape[1:] != self._shape:
            raise ValueError("Expected input of shape {}, got {}".format(self._shape, inputs.shape[1:]))
        logits = self._compute_params(context)
        assert logits.shape == inputs.shape
        return ops.bernoulli_log_prob(inputs, logits)

    def _sample(self, num_samples, context):
        logits = self._compute_params(context)
        context_size = context.shape[0]
        noise = torch.rand(context_size * num_samples, *self._shape, device=logits.device)
        samples = ops.bernoulli_sample(logits, noise, num_samples)
        return torchutils.split_leading_dim(samples, [context_size, num_samples])

    def _mean(self, context):
        logits = self._compute_params(context)
        return torch.sigmoid(logits)


def _identity(x):
    """The default context encoder (a module-level function, so that the distribution pickles)."""
    return x
