"""Helpers of the invertible residual blocks (the names of flowcon/transforms/lipschitz/util.py): the generators of
power-series coefficients for the training-mode log-determinant estimators, and two general fixed-point solvers.

``log det(I + J) = sum_k (-1)^(k+1) tr(J^k) / k``.  The biased generator truncates the series.  The unbiased one
(Russian roulette) always keeps ``n_exact_terms`` terms, draws how many more to keep from a geometric law and divides
every kept extra term by the probability that it was kept, which makes the truncated sum unbiased.  The draw comes from
``np.random.geometric`` and the estimators' probe vectors from ``torch.randn_like``, the reference's two sources, so a
run seeded through ``np.random.seed`` and ``torch.manual_seed`` reproduces the reference's training-mode numbers."""
import math
from typing import Callable, Tuple

import numpy as np
import torch


class ParameterGenerator(torch.nn.Module):
    """``sample_parameters(training) -> (coeff_fn, n_power_series)``: the weight of term k and the number of terms."""

    def sample_parameters(self, training=True) -> Tuple[Callable, int]:
        raise NotImplementedError


class GeometricSampler:
    """N ~ Geometric(p) on 1, 2, ... with ``p = sigmoid(geom_p)``, drawn from numpy's global generator."""

    def __init__(self, geom_p):
        self.geom_p = 1.0 / (1.0 + math.exp(-geom_p))

    def sample_fn(self, m):
        return np.random.geometric(self.geom_p, m)

    def rcdf_fn(self, k, offset):
        """P(N >= k - offset); one for the terms up to ``offset``, which are always kept."""
        extra = k - offset
        return 1.0 if extra <= 1 else (1.0 - self.geom_p) ** (extra - 1)


class UnbiasedParameterGenerator(ParameterGenerator):
    geom_p = 0.0        # the logit of p = 1/2

    def __init__(self, n_exact_terms, n_samples):
        super().__init__()
        self.sampler = GeometricSampler(self.geom_p)
        self.n_exact_terms = n_exact_terms
        self.n_samples = n_samples

    def sample_parameters(self, training=True):
        draws = self.sampler.sample_fn(self.n_samples)
        n_power_series = int(draws.max()) + self.n_exact_terms + (0 if training else 20)
        exact = self.n_exact_terms

        def coeff_fn(k):
            kept = float(np.mean(draws >= k - exact))           # share of the draws that reach term k
            return kept / self.sampler.rcdf_fn(k, exact)

        return coeff_fn, n_power_series


class BiasedParameterGenerator(ParameterGenerator):
    def __init__(self, n_power_series):
        super().__init__()
        self.n_power_series = n_power_series

    def sample_parameters(self, training=True):
        return (lambda k: 1), self.n_power_series


# ---- fixed points -----------------------------------------------------------------------------------------------------

def _residual_ratio(fx, x, tol):
    """Per sample: the largest ``|f(x) - x| / tol`` over its elements."""
    return ((fx - x).abs() / tol).flatten(1).amax(dim=1)


def find_fixed_point_noaccel(f, x0, threshold=1000, eps=1e-5):
    """``x = f(x)`` by the relaxed iteration ``x <- x + a (f(x) - x)`` with a step ``a`` per sample: it starts at 1,
    halves (not below 1/16) when the sample's residual grew, and doubles back when it shrank.  Stops when every
    element has ``|f(x) - x| <= eps (1 + |x0|)`` or after ``threshold`` evaluations of ``f``; samples that are done are
    left where they are."""
    with torch.no_grad():
        tol = eps * (1.0 + x0.abs())
        shape = (x0.shape[0],) + (1,) * (x0.dim() - 1)
        step = torch.ones(shape, dtype=x0.dtype, device=x0.device)
        x = x0
        last = None
        for _ in range(threshold):
            fx = f(x)
            ratio = _residual_ratio(fx, x, tol)
            if bool((ratio <= 1).all()):
                break
            if last is not None:
                grew = (ratio > last).view(shape)
                step = torch.where(grew, step * 0.5, step * 2.0).clamp(1.0 / 16.0, 1.0)
            last = ratio
            move = torch.where((ratio > 1).view(shape), step, torch.zeros_like(step))
            x = x + move * (fx - x)
        return x


def find_fixed_point(f, x0, threshold=1000, eps=1e-5):
    """``x = f(x)`` by Anderson mixing of depth one: with residuals ``r_n = f(x_n) - x_n`` the next iterate is
    ``f(x_n) - c (f(x_n) - f(x_(n-1)))``, ``c = <r_n, r_n - r_(n-1)> / |r_n - r_(n-1)|^2`` per sample (the secant step
    of a linear map).  If the residual has not improved for 10 steps, the relaxed iteration above takes over from the
    best iterate.  Same stopping rule as ``find_fixed_point_noaccel``."""
    with torch.no_grad():
        tol = eps * (1.0 + x0.abs())
        shape = (x0.shape[0],) + (1,) * (x0.dim() - 1)
        x, fx = x0, f(x0)
        best, best_x, since_best = math.inf, x0, 0
        prev_fx = prev_r = None
        for used in range(1, threshold):
            r = fx - x
            worst = float(_residual_ratio(fx, x, tol).max())
            if worst <= 1:
                return x
            if worst < best:
                best, best_x, since_best = worst, x, 0
            else:
                since_best += 1
                if since_best >= 10:
                    break
            if prev_r is None:
                new_x = fx
            else:
                dr = (r - prev_r).flatten(1)
                c = (r.flatten(1) * dr).sum(1) / (dr.square().sum(1) + 1e-30)
                new_x = fx - c.view(shape) * (fx - prev_fx)
            prev_fx, prev_r = fx, r
            x, fx = new_x, f(new_x)
        return find_fixed_point_noaccel(f, best_x, threshold=max(threshold - used, 1), eps=eps)
