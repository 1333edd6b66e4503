"""``Linear``: base of the transforms that parameterise an invertible [D, D] weight (LU, ...).

Protocol (flowcon/transforms/linear.py:15-126, restated from SURVEY.md 8a row U2): a subclass supplies
``weight()``, ``weight_inverse()``, ``logabsdet()`` and the uncached ``forward_no_cache`` / ``inverse_no_cache``.
With ``using_cache`` and the module in eval mode the dense weight (or its inverse) and log|det W| are computed once
and reused -- any ``train(True)`` drops them -- and the map itself is one ``fc_linear`` launch:

    forward:  y = W x + b,            logabsdet =  log|det W|   (the same value for every row)
    inverse:  y = W^-1 (x - b),       logabsdet = -log|det W|

Above ``ops.MAX_ROW_FEATURES`` features the map is the reference's ``F.linear`` on the device.
"""
import numpy as np
import torch
from torch import nn
from torch.nn import functional as F
from torch.nn import init

from flowconductor_amd import ops, options
from flowconductor_amd.transforms.base import Transform
from flowconductor_amd.utils import torchutils
from flowconductor_amd.utils import typechecks as check


class LinearCache:
    """The three cached quantities (``None`` = not computed yet)."""

    weight = inverse = logabsdet = None

    def invalidate(self):
        self.weight = self.inverse = self.logabsdet = None


class Linear(Transform):
    """Abstract base class for linear transforms that parameterize a weight matrix."""

    def __init__(self, features, using_cache=False):
        check.need_positive_int(features, "Number of features")
        super().__init__()
        self.features, self.using_cache, self.cache = features, using_cache, LinearCache()
        self.bias = nn.Parameter(torch.zeros(features))     # state_dict key "bias", as in the reference

    # -- cache ----------------------------------------------------------------------------------------------------
    def use_cache(self, mode=True):
        self.using_cache = check.need_bool(mode, "Mode")

    def train(self, mode=True):
        if bool(mode):                    # parameters are about to change
            self.cache.invalidate()
        return super().train(mode)

    def _cache_active(self, inputs):
        wants_grad = torch.is_grad_enabled() and (inputs.requires_grad
                                                  or any(p.requires_grad for p in self.parameters()))
        return self.using_cache and not self.training and not wants_grad

    def _fill(self, slot, one, both):
        """Make ``cache.<slot>`` and ``cache.logabsdet`` present: the joint routine when both are missing (a
        subclass may share work between them), otherwise only the missing one."""
        cache = self.cache
        have_matrix, have_det = getattr(cache, slot) is not None, cache.logabsdet is not None
        if not have_matrix and not have_det:
            matrix, cache.logabsdet = both()
            setattr(cache, slot, matrix)
        elif not have_matrix:
            setattr(cache, slot, one())
        elif not have_det:
            cache.logabsdet = self.logabsdet()

    def _check_forward_cache(self):
        self._fill("weight", self.weight, self.weight_and_logabsdet)

    def _check_inverse_cache(self):
        self._fill("inverse", self.weight_inverse, self.weight_inverse_and_logabsdet)

    # -- the map --------------------------------------------------------------------------------------------------
    def forward(self, inputs, context=None):
        if not self._cache_active(inputs):
            return self.forward_no_cache(inputs)
        self._check_forward_cache()
        if self.features > ops.MAX_ROW_FEATURES:    # wider than the row kernels: the reference's F.linear
            outputs = F.linear(inputs, self.cache.weight, self.bias)
        else:
            outputs = ops.linear(inputs, self.cache.weight, bias=self.bias, mode=ops.LINEAR_DENSE)
        return outputs, self.cache.logabsdet.expand(outputs.shape[0]).clone()

    def inverse(self, inputs, context=None):
        if not self._cache_active(inputs):
            return self.inverse_no_cache(inputs)
        self._check_inverse_cache()
        # W^-1 (x - b) with the bias subtracted first, as the reference does: W^-1 x - W^-1 b cancels when |b| dominates
        if self.features > ops.MAX_ROW_FEATURES:
            outputs = F.linear(inputs - self.bias, self.cache.inverse)
        else:
            outputs = ops.linear(inputs, self.cache.inverse, bias=self.bias, mode=ops.LINEAR_DENSE_SHIFTED)
        return outputs, (-self.cache.logabsdet).expand(outputs.shape[0]).clone()

    # -- what a subclass provides -----------------------------------------------------------------------------------
    def weight_and_logabsdet(self):
        """Joint form; a subclass whose two quantities share work overrides it."""
        return (self.weight(), self.logabsdet())

    def weight_inverse_and_logabsdet(self):
        return (self.weight_inverse(), self.logabsdet())

    forward_no_cache = check.abstract("forward_no_cache", "(inputs) -> (outputs, logabsdet) from the parameters")
    inverse_no_cache = check.abstract("inverse_no_cache", "(inputs) -> (outputs, logabsdet) from the parameters")
    weight = check.abstract("weight", "() -> dense [D, D] weight")
    weight_inverse = check.abstract("weight_inverse", "() -> dense [D, D] inverse weight")
    logabsdet = check.abstract("logabsdet", "() -> scalar log|det W|")


class _FactorisedInverse(torch.autograd.Function):
    """``W^-1`` as a differentiable function of ``W`` from an inverse that was factorised without a graph:
    ``dW = -W^-T g W^-T`` (two GEMMs, no solver call under autograd)."""

    @staticmethod
    def forward(ctx, weight, weight_inverse):
        ctx.save_for_backward(weight_inverse)
        return weight_inverse.clone()

    @staticmethod
    def backward(ctx, grad):
        w_inv, = ctx.saved_tensors
        return -(w_inv.T @ grad @ w_inv.T), None


class NaiveLinear(Linear):
    """``y = W x + bias`` with an unconstrained weight (flowcon/transforms/linear.py:129-229; parameters ``_weight`` [D, D] and
    ``bias`` [D], reference checkpoints load).  The products run in ``fc_linear``, wide no-grad batches in ``fc_dense_mm``.

    ``W^-1`` and, without a graph, ``log|det W|`` come from ONE float64 ``lu_factor`` on the parameter's device, rounded
    once to float32 and kept until a parameter changes (a sampling loop factorises once); the inverse subtracts the bias
    before the product.  Under autograd both directions sit behind ``_DenseLinearFunction`` (kernel forward, library GEMMs
    backward; the inverse is handed the factorised ``W^-1``) and the log-determinant is a differentiable ``slogdet``.

    Deliberate difference: ``weight_inverse_and_logabsdet`` builds its identity on the parameter's device (the reference
    builds it on the CPU, linear.py:216, and fails for a module on a GPU)."""

    _HIP_AUTOGRAD = True

    def __init__(self, features, orthogonal_initialization=True, using_cache=False):
        super().__init__(features, using_cache)
        if orthogonal_initialization:
            self._weight = nn.Parameter(torchutils.random_orthogonal(features))
        else:
            self._weight = nn.Parameter(torch.empty(features, features))
            stdv = 1.0 / np.sqrt(features)
            init.uniform_(self._weight, -stdv, stdv)

    # -- dense forms ------------------------------------------------------------------------------------------------
    def _factorised(self):
        """``(W^-1, log|det W|)`` in float32 from one float64 LU factorisation, memoised per parameter version."""
        def factorise():
            w = self._weight.detach().double()
            lu, pivots = torch.linalg.lu_factor(w)
            eye = torch.eye(self.features, dtype=torch.float64, device=w.device)
            w_inv = torch.linalg.lu_solve(lu, pivots, eye)
            logabsdet = torch.sum(torch.log(torch.abs(torch.diagonal(lu))))
            return w_inv.to(self._weight.dtype).contiguous(), logabsdet.to(self._weight.dtype)

        return ops.memo(self, "factorised", ops.cache_key(self._weight, self.bias), factorise)

    def weight(self):
        return self._weight

    def weight_inverse(self):
        if self._needs_grad(self._weight):
            return _FactorisedInverse.apply(self._weight, self._factorised()[0])
        return self._factorised()[0]

    def weight_inverse_and_logabsdet(self):
        if self._needs_grad(self._weight):
            return self.weight_inverse(), self.logabsdet()
        return self._factorised()

    def logabsdet(self):
        if self._needs_grad(self._weight):
            return torchutils.logabsdet(self._weight)
        return self._factorised()[1]

    # -- the map ----------------------------------------------------------------------------------------------------
    def _needs_grad(self, inputs):
        return torch.is_grad_enabled() and (inputs.requires_grad or any(p.requires_grad for p in self.parameters()))

    def _composition(self, inputs, inverse):
        """The reference's own composition (linear.py:159-190), differentiable as it stands: the widths above
        ``ops.MAX_ROW_FEATURES``, where no row kernel runs."""
        if not inverse:
            return F.linear(inputs, self._weight, self.bias)
        lu, pivots = torch.linalg.lu_factor(self._weight)
        return torch.linalg.lu_solve(lu, pivots, (inputs - self.bias).t()).t()

    def _wide(self, inputs):
        """``LULinear``'s wide-batch rule: enough rows on the device, a shape ``fc_dense_mm`` takes."""
        rows = inputs.shape[0]
        return (inputs.dim() == 2 and inputs.is_cuda and rows >= 1024 and rows % ops.SYLVESTER_MM_ROWS == 0
                and ops.sylvester_mm_supported(rows, self.features) and options.get("sylvester_mm"))

    def _map(self, inputs, inverse):
        if self.features > ops.MAX_ROW_FEATURES:
            outputs = self._composition(inputs, inverse)
            logabsdet = torchutils.logabsdet(self._weight)
        elif self._needs_grad(inputs):
            # training / differentiable sampling: the kernel behind an autograd node
            outputs = ops.dense_linear_autograd(inputs, self._weight, self.bias, self._factorised()[0] if inverse else None)
            logabsdet = torchutils.logabsdet(self._weight)
        else:
            with torch.no_grad():
                if not inverse:
                    logabsdet = self._factorised()[1]
                    if self._wide(inputs):
                        outputs = ops.dense_mm(inputs, self._weight, self.bias)
                    else:
                        outputs = ops.linear(inputs, self._weight, bias=self.bias, mode=ops.LINEAR_DENSE)
                else:
                    w_inv, logabsdet = self._factorised()
                    # the bias comes off BEFORE the product: W^-1 x - W^-1 b cancels when |b| dominates the result
                    if self._wide(inputs):
                        outputs = ops.dense_mm(inputs, w_inv, pre=self.bias)
                    else:
                        outputs = ops.linear(inputs, w_inv, bias=self.bias, mode=ops.LINEAR_DENSE_SHIFTED)
        return outputs, (-logabsdet if inverse else logabsdet) * outputs.new_ones(outputs.shape[0])

    def forward_no_cache(self, inputs):
        """``W x + bias``; logabsdet = log|det W| for every row."""
        return self._map(inputs, False)

    def inverse_no_cache(self, inputs):
        """``W^-1 (x - bias)``: the bias comes off first."""
        return self._map(inputs, True)


class ScalarScale(Transform):
    """y = (exp(_scale) + eps) x with ONE scalar for the whole tensor (flowcon/transforms/linear.py:232-252; the
    reference's matrix/ helpers compose it).  The reference's log-determinant multiplies log(scale) by the SUM of the
    non-batch sizes (``np.sum(inputs.shape[1:])``), which equals the number of elements only for [N, D] inputs: kept."""

    _HIP_AUTOGRAD = True

    def __init__(self, scale=1.0, trainable=True, eps=1e-4):
        super().__init__()
        if not np.all(np.asarray(scale) > 1e-6):
            raise AssertionError("Scale too small..")
        self._scale = nn.Parameter(torch.log(torch.tensor(scale, dtype=torch.get_default_dtype())), requires_grad=trainable)
        self.eps = eps

    @property
    def scale(self):
        return torch.exp(self._scale) + self.eps

    def _map(self, inputs, inverse):
        scale = self.scale
        outputs = ops.pointwise_affine_autograd(inputs, scale.reshape(1), torch.zeros(1, device=inputs.device), inverse=inverse)
        logabsdet = inputs.new_ones(inputs.shape[0]) * torch.log(scale).sum() * float(np.sum(inputs.shape[1:]))
        return outputs, (-logabsdet if inverse else logabsdet)

    def forward(self, inputs, context=None):
        return self._map(inputs, False)

    def inverse(self, inputs, context=None):
        return self._map(inputs, True)


class ScalarShift(Transform):
    """y = x + shift with one scalar (flowcon/transforms/linear.py:255-266); logabsdet = 0."""

    _HIP_AUTOGRAD = True

    def __init__(self, shift=0.0, trainable=True):
        super().__init__()
        self.shift = nn.Parameter(torch.tensor(shift, dtype=torch.get_default_dtype()), requires_grad=trainable)

    def _map(self, inputs, inverse):
        # (x - b) / 1 is the kernel's inverse form: subtracting the shift
        outputs = ops.pointwise_affine_autograd(inputs, torch.ones(1, device=inputs.device), self.shift.reshape(1),
                                                inverse=inverse)
        return outputs, inputs.new_zeros(inputs.shape[0])

    def forward(self, inputs, context=None):
        return self._map(inputs, False)

    def inverse(self, inputs, context=None):
        return self._map(inputs, True)
