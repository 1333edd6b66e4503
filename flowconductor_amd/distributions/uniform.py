"""Uniform distributions and the priors built on them (API of flowcon/distributions/uniform.py:7-89).

``BoxUniform.log_prob`` is one HIP row kernel (``ops.box_log_prob``); everything else is torch's own ``Uniform`` /
``Independent`` / ``MultivariateNormal`` machinery, with every constant built on the device of the values it meets."""
from typing import Union

import torch
from torch import distributions

from flowconductor_amd import ops


class BoxUniform(distributions.Independent):
    def __init__(
        self,
        low: Union[torch.Tensor, float],
        high: Union[torch.Tensor, float],
        reinterpreted_batch_ndims: int = 1,
        validate_args=None,
    ):
        """Multidimensional uniform distribution defined on a box.

        A `Uniform` distribution initialized with e.g. a parameter vector low or high of length 3 has a /batch/ dimension
        of length 3: a log_prob evaluation returns three numbers, one per independent Uniform.  A `BoxUniform` initialized
        in the same way has three /event/ dimensions, and returns one log_prob per point: whether it is inside the box
        defined by low and high or outside.  Only `log_prob` is overridden; sampling, the support, the moments and the
        entropy are `torch.distributions.Independent`'s.

        Args:
            low (Tensor or float): lower range (inclusive).
            high (Tensor or float): upper range (exclusive).
            reinterpreted_batch_ndims (int): the number of batch dims to reinterpret as event dims.
            validate_args (bool or None): torch's argument validation, handed to `Uniform` and `Independent` (an addition:
                the reference follows the process-wide default only).  With validation on, current torch raises
                `ValueError` for a point outside the box instead of returning `-inf`.
        """
        super().__init__(distributions.Uniform(low=low, high=high, validate_args=validate_args),
                         reinterpreted_batch_ndims, validate_args=validate_args)

    def log_prob(self, value):
        base = self.base_dist
        if self.reinterpreted_batch_ndims != 1 or base.low.dim() != 1 or not torch.is_tensor(value) \
                or value.dim() < 1 or value.shape[-1] != base.low.shape[0]:
            return super().log_prob(value)
        if base._validate_args:       # what Uniform.log_prob does first
            base._validate_sample(value)
        return ops.box_log_prob(value, base.low.contiguous(), base.high.contiguous())


class MG1Uniform(distributions.Uniform):
    def log_prob(self, value):
        return super().log_prob(self._to_noise(value))

    def sample(self, sample_shape=torch.Size()):
        return self._to_parameters(super().sample(sample_shape))

    def _to_parameters(self, noise):
        A_inv = torch.tensor([[1.0, 1, 0], [0, 1, 0], [0, 0, 1]], dtype=noise.dtype, device=noise.device)
        return noise @ A_inv

    def _to_noise(self, parameters):
        A = torch.tensor([[1.0, -1, 0], [0, 1, 0], [0, 0, 1]], dtype=parameters.dtype, device=parameters.device)
        return parameters @ A


class LotkaVolterraOscillating:
    def __init__(self, device=None):
        """``device``: where the prior's constants live (and so where it samples and evaluates); the default is the CPU,
        as in the reference, which has no such argument."""
        mean = torch.log(torch.tensor([0.01, 0.5, 1, 0.01], device=device))
        sigma = 0.5
        covariance = sigma ** 2 * torch.eye(4, device=device)
        self._gaussian = distributions.MultivariateNormal(loc=mean, covariance_matrix=covariance)
        # validation off: the rejection loop below and log_prob need -inf outside the box, where torch's validation (on by
        # default since the reference was written) raises
        self._uniform = BoxUniform(low=-5 * torch.ones(4, device=device), high=2 * torch.ones(4, device=device),
                                   validate_args=False)
        self._log_normalizer = -torch.log(torch.erf((2 - mean) / sigma) - torch.erf((-5 - mean) / sigma)).sum()

    def log_prob(self, value):
        unnormalized_log_prob = self._gaussian.log_prob(value) + self._uniform.log_prob(value)
        return self._log_normalizer + unnormalized_log_prob

    def sample(self, sample_shape=torch.Size()):
        """Rejection sampling on the host, as the reference does it: draw as many Gaussian candidates as are still missing,
        keep those inside the box, repeat (one ``.item()`` per round)."""
        wanted = sample_shape[0]
        missing, kept = wanted, []
        while missing > 0:
            candidates = self._gaussian.sample((missing,))
            inside = ~torch.isinf(self._uniform.log_prob(candidates))
            kept.append(candidates[inside].detach())
            missing -= inside.sum().item()
        samples = torch.cat(kept)[:wanted]
        assert samples.shape[0] == wanted
        return samples
