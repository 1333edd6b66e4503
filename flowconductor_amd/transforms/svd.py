"""SVD-parameterised linear transform: class name, constructor arguments, parameter names and shapes of
flowcon/transforms/svd.py:11-127 (reference checkpoints load); both directions run in the one-launch
``fc_hdh_linear`` HIP kernel, wide no-grad batches as one matrix-core product."""
import math

import torch
from torch import nn
from torch.nn import functional as F

from flowconductor_amd import ops, options
from flowconductor_amd.transforms.linear import Linear
from flowconductor_amd.transforms.orthogonal import HouseholderSequence


def reflect(inputs, q_vectors, reverse=False):
    """The reflections of orthogonal.py:144-171 as a torch expression (any device and dtype, differentiable): the dense
    weights, and the map itself above ``ops.MAX_ROW_FEATURES`` features."""
    outputs = inputs
    order = range(q_vectors.shape[0] - 1, -1, -1) if reverse else range(q_vectors.shape[0])
    for i in order:
        q = q_vectors[i]
        outputs = outputs - (outputs @ q).unsqueeze(-1) * ((2.0 / (q @ q)) * q)
    return outputs


def wide_rows(inputs, features):
    """The wide-batch condition of ``LULinear`` / ``HouseholderSequence._dense``: enough rows on the device to pay for
    folding the parameters into one [D, D] matrix, a shape ``fc_dense_mm`` takes, and the option on."""
    return (inputs.dim() == 2 and inputs.is_cuda and inputs.shape[0] >= 1024
            and ops.sylvester_mm_supported(inputs.shape[0], features) and options.get("sylvester_mm"))


def folded_mm(module, inputs, inverse, fold, tail):
    """``fc_dense_mm`` with the module's weight (or inverse weight) folded once in float64 -- ``fold(inverse)``, cached per
    parameter version -- over the rows that fill whole tiles; ``tail(rows)`` maps the remaining rows.  The inverse
    subtracts the bias inside the kernel, before the product."""
    mats = ops.memo(module, "dense", ops.cache_key(*module.parameters()), dict)
    if inverse not in mats:
        mats[inverse] = fold(inverse).float().contiguous()
    n = inputs.shape[0]
    body = n - n % ops.SYLVESTER_MM_ROWS
    if inverse:
        out = ops.dense_mm(inputs[:body], mats[inverse], pre=module.bias)
    else:
        out = ops.dense_mm(inputs[:body], mats[inverse], module.bias)
    return out if body == n else torch.cat((out, tail(inputs[body:])))


class SVDLinear(Linear):
    """``y = U (S (V^T x)) + bias`` with ``U = orthogonal_1``, ``V^T = orthogonal_2`` Householder sequences of
    ``num_householder`` reflections each and ``S = diag(softplus(unconstrained_diagonal) + eps) > 0``."""

    _HIP_AUTOGRAD = True

    def __init__(self, features, num_householder, using_cache=False, identity_init=True, eps=1e-3):
        super().__init__(features, using_cache)
        assert num_householder % 2 == 0
        self.eps = eps
        self.orthogonal_1 = HouseholderSequence(features=features, num_transforms=num_householder)
        self.unconstrained_diagonal = nn.Parameter(torch.zeros(features))
        self.orthogonal_2 = HouseholderSequence(features=features, num_transforms=num_householder)
        self.identity_init = identity_init
        with torch.no_grad():
            self.bias.zero_()
            if identity_init:
                # softplus(c) + eps = 1  <=>  c = log(exp(1 - eps) - 1): W = I at initialisation
                self.unconstrained_diagonal.fill_(math.log(math.expm1(1.0 - eps)))
            else:
                bound = features ** -0.5
                self.unconstrained_diagonal.uniform_(-bound, bound)

    @property
    def diagonal(self):
        return self.eps + F.softplus(self.unconstrained_diagonal)

    @property
    def log_diagonal(self):
        return torch.log(self.diagonal)

    def logabsdet(self):
        return torch.sum(self.log_diagonal)

    # -- dense forms ------------------------------------------------------------------------------------------------
    def _fold(self, inverse):
        """float64 ``W`` (or ``W^-1``) as svd.py:97-119 builds them: rows of diag(S) through ``orthogonal_2^-1``, the
        transpose through ``orthogonal_1``, transposed back (the inverse weight the other way round)."""
        q1, q2 = self.orthogonal_1.q_vectors.double(), self.orthogonal_2.q_vectors.double()
        diagonal = self.diagonal.double()
        if not inverse:
            return reflect(reflect(torch.diag(diagonal), q2, reverse=True).t(), q1).t()
        return reflect(reflect(torch.diag(torch.reciprocal(diagonal)), q1).t(), q2, reverse=True).t()

    def weight(self):
        """Formed in float64 and rounded once (the reference applies the 2 K reflections in the parameters' dtype)."""
        return self._fold(False).to(self.bias.dtype)

    def weight_inverse(self):
        return self._fold(True).to(self.bias.dtype)

    # -- the map ----------------------------------------------------------------------------------------------------
    def _needs_grad(self, inputs):
        return torch.is_grad_enabled() and (inputs.requires_grad or any(p.requires_grad for p in self.parameters()))

    def _operands(self, inverse):
        """``fc_hdh_linear``'s (q_a, q_b, scale, pre, post, reverse) for one direction."""
        q1, q2 = self.orthogonal_1.q_vectors, self.orthogonal_2.q_vectors
        if not inverse:
            return q2, q1, self.diagonal, None, self.bias, False
        return q1, q2, torch.reciprocal(self.diagonal), self.bias, None, True

    def _composition(self, inputs, inverse):
        """The reference's own composition (svd.py:56-95) on the device, differentiable as it stands: the widths above
        ``ops.MAX_ROW_FEATURES``, where no row kernel runs."""
        q_a, q_b, scale, pre, post, reverse = self._operands(inverse)
        outputs = inputs if pre is None else inputs - pre
        outputs = reflect(reflect(outputs, q_a, reverse) * scale, q_b, reverse)
        return outputs if post is None else outputs + post

    def _map(self, inputs, inverse):
        if self.features > ops.MAX_ROW_FEATURES:
            outputs = self._composition(inputs, inverse)
        elif self._needs_grad(inputs):      # training: one autograd node, one launch each way
            q_a, q_b, scale, pre, post, reverse = self._operands(inverse)
            outputs = ops.hdh_linear_autograd(inputs, q_a, q_b, scale, pre, post, reverse, reverse)
        else:
            with torch.no_grad():
                q_a, q_b, scale, pre, post, reverse = self._operands(inverse)

                def rows(x):
                    return ops.hdh_linear(x, q_a, q_b, scale, pre, post, reverse, reverse)

                outputs = folded_mm(self, inputs, inverse, self._fold, rows) if wide_rows(inputs, self.features) else rows(inputs)
        logabsdet = self.logabsdet()
        return outputs, (-logabsdet if inverse else logabsdet) * outputs.new_ones(outputs.shape[0])

    def forward_no_cache(self, inputs):
        """``orthogonal_1(diagonal * orthogonal_2(x)) + bias``; logabsdet = sum log diagonal for every row."""
        return self._map(inputs, False)

    def inverse_no_cache(self, inputs):
        """``orthogonal_2^-1(orthogonal_1^-1(x - bias) / diagonal)``: the bias comes off first."""
        return self._map(inputs, True)
