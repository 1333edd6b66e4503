"""Sum-of-sigmoids monotone transform and the deep sigmoidal flow (API of flowcon/transforms/adaptive_sigmoids.py)."""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from flowconductor_amd import ops
from flowconductor_amd.transforms.base import Transform
from flowconductor_amd.transforms.no_analytic_inv.base import MonotonicTransform
from flowconductor_amd.transforms.nonlinearities import ExtendedSoftplus


class SumOfSigmoids(MonotonicTransform):
    """Element-wise sum of S shifted/scaled sigmoids plus an extended softplus (linear far from the
    origin); inverse by bisection + Newton.  Both directions are one fused HIP kernel.

    Parameters keep the reference's names: ``shift_preact``, ``log_scale_preact``, ``raw_softmax``
    (``[1, F, S]``), ``extended_softplus.shift`` (``[1, F]``), ``log_scale_postact`` (``[1]``, frozen).
    With ``raw_params`` (``[N, F, 3S+1]``) the same tensors are per-sample views of it."""

    _HIP_AUTOGRAD = True    # forward kernel behind an autograd node (gradients from the same map in torch ops)

    PREACT_SCALE_MIN = .1
    PREACT_SCALE_MAX = 10.
    PREACT_SHIFT_MAX = 10

    def __init__(self, features, n_sigmoids=10, iterations_bisection_inverse=50, lim_bisection_inverse=120,
                 raw_params: torch.Tensor = None):
        self.n_sigmoids = n_sigmoids
        self.features = features
        super().__init__(num_iterations=iterations_bisection_inverse, lim=lim_bisection_inverse)
        self._raw = None
        if raw_params is None:
            self.shift_preact = nn.Parameter(torch.randn(1, features, self.n_sigmoids), requires_grad=True)
            self.log_scale_preact = nn.Parameter(torch.zeros(1, features, self.n_sigmoids), requires_grad=True)
            self.raw_softmax = nn.Parameter((torch.ones(1, features, self.n_sigmoids, requires_grad=False)))
            self.extended_softplus = ExtendedSoftplus(features=features)
        else:
            assert raw_params.shape[1:] == (features, 3 * self.n_sigmoids + 1)
            self.set_raw_params(features, raw_params)
        self.log_scale_postact = nn.Parameter(torch.log(torch.ones(1, device=self.shift_preact.device)),
                                              requires_grad=False)
        self.eps = 1e-6

    def get_raw_params(self):
        """All raw parameters concatenated: ``[-1, features, 3*n_sigmoids + 1]``."""
        return torch.cat((self.shift_preact.reshape(-1, self.features, self.n_sigmoids),
                          self.log_scale_preact.reshape(-1, self.features, self.n_sigmoids),
                          self.raw_softmax.reshape(-1, self.features, self.n_sigmoids),
                          self.extended_softplus.shift.reshape(-1, self.features, 1)), dim=-1)

    def set_raw_params(self, features, raw_params):
        vals = torch.split(raw_params, [self.n_sigmoids, self.n_sigmoids, self.n_sigmoids, 1], dim=-1)
        self.shift_preact, self.log_scale_preact, self.raw_softmax = vals[:3]
        self.extended_softplus = ExtendedSoftplus(features=features, shift=vals[3])
        self._raw = raw_params

    def _kernel(self, inputs, inverse, offset=0.0):
        raw = self._raw if self._raw is not None else self.get_raw_params()
        shared = raw.shape[0] == 1
        if not shared and raw.shape[0] != inputs.shape[0]:
            raise ValueError("raw_params batch %d != inputs batch %d" % (raw.shape[0], inputs.shape[0]))
        return ops.sum_of_sigmoids_autograd(inputs, raw, self.n_sigmoids, inverse=inverse, offset=offset,
                                            iterations=self.num_iterations, lim=self.lim, shared_params=shared)

    def forward(self, inputs, context=None):
        return self._kernel(inputs, inverse=False)

    def inverse(self, inputs, context=None, forward_function=None):
        if forward_function is not None:
            return super().inverse(inputs, context=context, forward_function=forward_function)
        return self._kernel(inputs, inverse=True)


class DeepSigmoidModule(Transform):
    """The deep sigmoidal flow of Neural Autoregressive Flows (adaptive_sigmoids.py:145-218): per element
    ``y = logit((1 - eps) sum_k w_k sigmoid(a_k x + b_k) + eps / 2)`` with ``3 * n_sigmoids`` raw values
    ``[raw_a | raw_b | raw_w]`` per element (``a = softplus``, mollified; ``w = softmax``).  2-D float32 device inputs run
    in one HIP kernel (``fc_deep_sigmoid``), with a HIP backward kernel behind autograd; anything else -- other ranks,
    other dtypes, the CPU, rows too long for the kernel's LDS plan -- takes the reference's composition of torch ops.

    This class deliberately extends the reference, whose ``inverse`` raises ``NotImplementedError("..")`` and whose
    constructor accepts ``num_inverse_iterations`` and ``lim`` only to drop them: here both are stored and
    ``inverse_given_params`` solves ``f(x) = y`` per element (bracket from ``[-lim, lim]``, safeguarded Newton capped at
    ``num_inverse_iterations``, two closing Newton steps; ``logabsdet = -logabsdet_forward(x)``).  Inputs at or beyond
    the range ``|y| < log((1 - eps / 2) / (eps / 2))`` raise ``InputOutsideDomain``."""

    _HIP_AUTOGRAD = True

    @staticmethod
    def softmax(x, dim=-1):
        e_x = torch.exp(x - x.max(dim=dim, keepdim=True)[0])
        return e_x / e_x.sum(dim=dim, keepdim=True)

    def __init__(self, n_sigmoids=4, mollify=0., eps=1e-4, num_inverse_iterations=100, lim=10):
        super().__init__()
        self.n_sigmoids = n_sigmoids
        self.act_a = nn.Softplus()
        self.act_b = nn.Identity()
        self.act_w = nn.Softmax(dim=-1)
        self._mollify = mollify
        self.eps = eps
        self.num_inverse_iterations = num_inverse_iterations
        self.lim = lim
        self.softplus_ = nn.Softplus()
        self.sigmoid_ = nn.Sigmoid()

    def forward(self, inputs, context=None):
        dsparams = self.get_params(inputs, context)
        return self.forward_given_params(inputs, dsparams=dsparams)

    def inverse(self, inputs, context=None):
        dsparams = self.get_params(inputs, context)
        return self.inverse_given_params(inputs, dsparams=dsparams)

    def get_params(self, inputs, context=None):
        raise NotImplementedError()

    def raw_scales(self, dsparams):
        return dsparams[..., 0 * self.n_sigmoids:1 * self.n_sigmoids]

    def raw_shifts(self, dsparams):
        return dsparams[..., 1 * self.n_sigmoids:2 * self.n_sigmoids]

    def raw_weights(self, dsparams):
        return dsparams[..., 2 * self.n_sigmoids:3 * self.n_sigmoids]

    def mollify(self, a_, b_):
        a = a_ * (1 - self._mollify) + 1.0 * self._mollify
        b = b_ * (1 - self._mollify) + 0.0 * self._mollify
        return a, b

    def forward_given_params(self, inputs, dsparams=None):
        """``dsparams``: ``[F, 3S]`` (shared over the batch) or ``[N, F, 3S]``."""
        return self._given_params(inputs, dsparams, inverse=False)

    def inverse_given_params(self, inputs, dsparams=None):
        """The numerical inverse (not in the reference); ``dsparams`` as for ``forward_given_params``."""
        return self._given_params(inputs, dsparams, inverse=True)

    # ---- dispatch -------------------------------------------------------------------------------------------------
    def _given_params(self, inputs, dsparams, inverse, divisor=1.0):
        """``divisor``: the MADE form hands over the conditioner's output and 5: the kernel multiplies by 1 / 5 itself."""
        features = inputs.shape[-1]
        if dsparams.dim() not in (2, 3) or dsparams.shape[-2:] != (features, 3 * self.n_sigmoids):
            raise ValueError("dsparams must be [%d, %d] or [N, %d, %d], got %s" % (
                features, 3 * self.n_sigmoids, features, 3 * self.n_sigmoids, tuple(dsparams.shape)))
        if dsparams.dim() == 3 and dsparams.shape[0] != inputs.shape[0]:
            raise ValueError("dsparams batch %d != inputs batch %d" % (dsparams.shape[0], inputs.shape[0]))
        if (inputs.dim() == 2 and inputs.is_cuda and inputs.dtype == torch.float32 and dsparams.dtype == torch.float32
                and dsparams.device == inputs.device and ops.deep_sigmoid_fits(features, features, self.n_sigmoids)):
            return ops.deep_sigmoid_autograd(inputs, dsparams, self.n_sigmoids, inverse=inverse, mollify=self._mollify,
                                             eps=self.eps, prescale=1.0 / divisor, iterations=self.num_inverse_iterations,
                                             lim=self.lim, shared_params=dsparams.dim() == 2)
        if divisor != 1.0:
            dsparams = dsparams / divisor
        if inverse:
            return self._composition_inverse(inputs, dsparams)
        return self._composition(inputs, dsparams)

    # ---- the reference's composition of torch ops (adaptive_sigmoids.py:177-210, same operation order) --------------
    def _log(self, x):
        return torch.log(x * 1e2) - np.log(1e2)

    def _logsigmoid(self, x):
        return -(self.softplus_(-x) + self.eps)

    def _composition(self, inputs, dsparams):
        scale_ = self.act_a(self.raw_scales(dsparams))
        shift_ = self.act_b(self.raw_shifts(dsparams))
        weight = self.act_w(self.raw_weights(dsparams))
        scale, shift = self.mollify(scale_, shift_)
        pre_sigm = scale * inputs.unsqueeze(-1) + shift
        x_pre = torch.sum(weight * torch.sigmoid(pre_sigm), dim=-1)
        x_pre_clipped = x_pre * (1 - self.eps) + self.eps * 0.5
        outputs = self._log(x_pre_clipped) - self._log(1 - x_pre_clipped)
        logj = F.log_softmax(self.raw_weights(dsparams), dim=-1) + self._logsigmoid(pre_sigm) \
            + self._logsigmoid(-pre_sigm) + self._log(scale)
        logj = torch.logsumexp(logj, -1)
        logabsdet = logj + np.log(1 - self.eps) - (self._log(x_pre_clipped) + self._log(-x_pre_clipped + 1))
        return outputs, logabsdet.sum(-1)

    def _composition_inverse(self, inputs, dsparams):
        """The kernel's search in torch ops, for the inputs the kernel does not take: domain check, a bracket doubled out
        from ``[-lim, lim]``, ``num_inverse_iterations`` bisection steps, two Newton steps."""
        bound = np.log((1 - 0.5 * self.eps) / (0.5 * self.eps))
        if not bool((inputs.abs() < bound).all()):
            raise ops.InputOutsideDomain()

        def value(x):
            return self._composition(x.unsqueeze(-1), dsparams.unsqueeze(-2))

        # (each element is a one-feature row of its own, so that _composition's row sum leaves the per-element log-slope)
        params = dsparams.detach()
        with torch.no_grad():
            def f(x):
                return self._composition(x.unsqueeze(-1), params.unsqueeze(-2))[0].squeeze(-1)

            hi = torch.full_like(inputs, float(self.lim))
            lo = -hi
            for _ in range(40):
                grow = f(hi) < inputs
                if not bool(grow.any()):
                    break
                hi = torch.where(grow, hi * 2, hi)
            for _ in range(40):
                grow = f(lo) > inputs
                if not bool(grow.any()):
                    break
                lo = torch.where(grow, lo * 2, lo)
            for _ in range(int(self.num_inverse_iterations)):
                mid = 0.5 * (lo + hi)
                above = f(mid) > inputs
                hi = torch.where(above, mid, hi)
                lo = torch.where(above, lo, mid)
            x = 0.5 * (lo + hi)
            for _ in range(2):
                val, logslope = value(x)
                x = x - (val.squeeze(-1) - inputs) / (torch.exp(logslope) + 1e-7)
        # one Newton-shaped step through the differentiable composition carries the implicit-function gradients
        val, logslope = value(x)
        # (the log-det carries the reference's -2 eps per element: the slope itself is exp(logslope + 2 eps))
        x = x - (val.squeeze(-1) - inputs) / torch.exp(logslope + 2 * self.eps).detach()
        _, logslope = value(x)
        return x, -logslope.sum(-1)


class DeepSigmoid(DeepSigmoidModule):
    """Deep sigmoidal flow with one batch-shared parameter ``dsparams`` ``[features, 3 * n_sigmoids]``
    (adaptive_sigmoids.py:221-235).  ``inverse`` is this project's extension (the reference raises
    ``NotImplementedError``): see ``DeepSigmoidModule``."""

    def __init__(self, features, *args, **kwargs):
        self.features = features
        super().__init__(*args, **kwargs)
        _a_preact = -2 * torch.ones(self.features, self.n_sigmoids)  # scale
        _b_preact = torch.zeros(self.features, self.n_sigmoids)  # shift
        _w_preact = torch.ones(self.features, self.n_sigmoids)  # softmax
        self.dsparams = nn.Parameter(torch.cat([_a_preact + 1e-5 * torch.randn_like(_a_preact),
                                                _b_preact + 1e-5 * torch.randn_like(_b_preact),
                                                _w_preact + 1e-3 * torch.randn_like(_w_preact)], -1),
                                     requires_grad=True)

    def get_params(self, inputs, context=None):
        return self.dsparams

    def forward(self, inputs, context=None):
        return self.forward_given_params(inputs=inputs, dsparams=self.dsparams)

    def inverse(self, inputs, context=None):
        return self.inverse_given_params(inputs=inputs, dsparams=self.dsparams)
