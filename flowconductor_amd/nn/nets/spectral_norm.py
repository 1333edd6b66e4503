"""Soft normalisation of a weight by an induced operator norm, as a ``torch.nn.utils.parametrize`` parametrisation
(the entry point and ``state_dict`` layout of flowcon/nn/nets/spectral_norm.py: ``...parametrizations.weight.original``,
``...weight.0._u``, ``...weight.0._v``).

The induced norm ``|W|_(p->q) = max over |v|_p = 1 of |W v|_q`` is estimated by the generalised power method
(Boyd 1974): alternately ``u <- the dual vector of W v for the q-norm`` and ``v <- the unit p-norm vector that
maximises <v, W^T u>``; then ``sigma = <u, W v>``.  For p = q = 2 both steps are plain normalisations and this is the
usual spectral-norm power iteration.  The normalisation is soft, ``W / max(1, sigma / coeff)``: a weight whose norm is
already below ``coeff`` is left alone.  Power iterations run in training mode only; in eval mode ``sigma`` comes from
the stored vectors, so the normalised weight is a constant of the parameters (which is what the eval-mode kernels
pack).  Norm orders are plain numbers (1, 2, inf or any p > 1); learnable orders are not ported."""
import math
from typing import Optional

import torch
import torch.nn.functional as F
from torch.nn.utils.parametrizations import _SpectralNorm
from torch.nn.utils.parametrize import register_parametrization

_TRANSPOSED_CONVS = (torch.nn.ConvTranspose1d, torch.nn.ConvTranspose2d, torch.nn.ConvTranspose3d)


def scaled_spectral_norm(module, domain, codomain, coeff=0.97, name: str = "weight", n_power_iterations: int = 1,
                         eps: float = 1e-12, dim: Optional[int] = None):
    """Put the soft induced-norm normalisation on ``module.<name>``; returns the module."""
    if not isinstance(getattr(module, name, None), torch.Tensor):
        raise ValueError("Module '{}' has no parameter or buffer with name '{}'".format(module, name))
    if dim is None:
        dim = int(isinstance(module, _TRANSPOSED_CONVS))    # the output channels of a transposed convolution are dim 1
    norm = _InducedSpectralNorm(getattr(module, name), domain, codomain, n_power_iterations, dim, eps, coeff=coeff)
    register_parametrization(module, name, norm)
    return module


def _one_hot_of_largest(vec):
    """sign(vec_k) e_k at the entry of largest magnitude."""
    k = torch.argmax(vec.abs())
    out = torch.zeros_like(vec)
    out[k] = 1.0 if vec[k] >= 0 else -1.0
    return out


def _signed_power(vec, exponent):
    """sign(vec) (|vec| / max|vec|)^exponent: the scaling keeps large exponents in range."""
    magnitude = vec.abs()
    return torch.sign(vec) * (magnitude / magnitude.max().clamp_min(torch.finfo(vec.dtype).tiny)) ** exponent


def dual_vector(y, q):
    """``u`` with ``|u|_(q*) = 1`` and ``<u, y> = |y|_q`` (``1/q + 1/q* = 1``)."""
    if q == 2:
        return F.normalize(y, p=2, dim=0)
    if q == 1:
        return torch.sign(y)
    if q == math.inf:
        return _one_hot_of_largest(y)
    u = _signed_power(y, q - 1)
    return u / torch.linalg.vector_norm(u, ord=q / (q - 1))


def maximiser(z, p):
    """``v`` with ``|v|_p = 1`` that maximises ``<v, z>``."""
    if p == 2:
        return F.normalize(z, p=2, dim=0)
    if p == 1:
        return _one_hot_of_largest(z)
    if p == math.inf:
        return torch.sign(z)
    v = _signed_power(z, 1 / (p - 1))
    return v / torch.linalg.vector_norm(v, ord=p)


class _InducedSpectralNorm(_SpectralNorm):
    """torch's spectral-norm parametrisation (its ``_u`` / ``_v`` buffers and weight reshaping) with the power method
    and the normalisation replaced."""

    def __init__(self, weight, domain, codomain, n_power_iterations: int = 1, dim: int = 0, eps: float = 1e-12,
                 coeff=0.97):
        if torch.is_tensor(domain) or torch.is_tensor(codomain):
            raise NotImplementedError("learnable (tensor-valued) induced norms are not ported")
        # needed by the power iterations that the base class runs while it constructs u and v; an nn.Module takes plain
        # attributes before its __init__
        self.domain, self.codomain, self.coeff = domain, codomain, coeff
        super().__init__(weight, n_power_iterations, dim, eps)

    @torch.no_grad()
    def _power_method(self, weight_mat, n_power_iterations):
        for _ in range(n_power_iterations):
            self._u.copy_(dual_vector(weight_mat @ self._v, self.codomain))
            self._v.copy_(maximiser(weight_mat.t() @ self._u, self.domain))

    def estimate_max_singular_val(self, weight):
        weight_mat = self._reshape_weight_to_matrix(weight)
        if self.training:
            self._power_method(weight_mat, self.n_power_iterations)
        # copies: the next training-mode call overwrites the buffers, which autograd must not see
        u, v = self._u.clone(), self._v.clone()
        return torch.dot(u, weight_mat @ v)

    def forward(self, weight):
        if weight.ndim == 1:
            return F.normalize(weight, dim=0, eps=self.eps)
        sigma = self.estimate_max_singular_val(weight)
        # The reference holds this factor in float32 whatever the weight's dtype (its max() is taken against a float32
        # one), so a float64 copy of a module divides by a float32-rounded number; the recorded float64 oracles of
        # tests/golden contain that, and a port that is to compute what the reference computes keeps it.
        return weight / torch.clamp(sigma / self.coeff, min=1.0).to(torch.float32)
