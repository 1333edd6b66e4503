"""Permutation, batch-shared point-wise affine, eval-mode batch norm and the element-wise non-linearities."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from flowconductor_amd import _hip
from ._core import _as_cols, _call, _err_word, _finish
from .colstats import batch_statistics_route, column_sums


class _PermuteFunction(torch.autograd.Function):
    """Gradient of a gather along ``dim`` = the gather by the inverse permutation (same HIP kernel)."""

    @staticmethod
    def forward(ctx, inputs, permutation, dim):
        with torch.no_grad():
            out = _permute_nograd(inputs, permutation, dim)
        ctx.permutation, ctx.dim = permutation, dim
        return out

    @staticmethod
    def backward(ctx, grad):
        inverse = torch.argsort(torch.as_tensor(ctx.permutation).to(grad.device).long())
        return _permute_nograd(grad.contiguous(), inverse, ctx.dim), None, None


def permute(inputs, permutation, dim=1):
    """``index_select(inputs, dim, permutation)`` bit-exactly (reference permutations.py:27-46); records an
    autograd node when gradients are required."""
    if torch.is_grad_enabled() and inputs.requires_grad:
        return _PermuteFunction.apply(inputs, permutation, dim)
    return _permute_nograd(inputs, permutation, dim)


def _permute_nograd(inputs, permutation, dim=1):
    lib = _hip.load()
    x = _hip.dev_f32(inputs, "inputs")
    _hip.require_no_grad(inputs)
    perm = _as_cols(permutation, x.device)
    d = x.shape[dim]
    outer = 1
    for s in x.shape[:dim]:
        outer *= s
    inner = 1
    for s in x.shape[dim + 1:]:
        inner *= s
    y = torch.empty_like(x)
    _call("fc_permute", lib.fc_permute, x.device, _hip.ptr(x), _hip.ptr(y), _hip.ptr(perm), outer, d,
          inner, _hip.stream_ptr(x.device))
    return y


def _item_vector(t, item_shape, device, name):
    """Broadcast a scalar / per-feature tensor to the flattened item shape (1 or m entries)."""
    t = torch.as_tensor(t, dtype=torch.float32, device=device)
    if t.numel() == 1:
        return t.reshape(1).contiguous()
    try:
        return t.expand(item_shape).reshape(-1).contiguous()
    except RuntimeError:
        raise RuntimeError("%s of shape %s is not broadcastable to inputs of shape %s"
                           % (name, tuple(t.shape), tuple(item_shape)))


def pointwise_affine(inputs, scale, shift, inverse=False):
    """``inputs * scale + shift`` or ``(inputs - shift) / scale`` with batch-shared scale/shift
    (reference standard.py:54-68, normalization.py:171-204)."""
    lib = _hip.load()
    x = _hip.dev_f32(inputs, "inputs")
    _hip.require_no_grad(inputs)
    n = x.shape[0]
    item_shape = x.shape[1:]
    m = 1
    for s in item_shape:
        m *= s
    sc = _item_vector(scale, item_shape, x.device, "scale")
    sh = _item_vector(shift, item_shape, x.device, "shift")
    y = torch.empty_like(x)
    _call("fc_pointwise_affine", lib.fc_pointwise_affine, x.device, _hip.ptr(x), _hip.ptr(y),
          _hip.ptr(sc), _hip.ptr(sh), None, None, n, m, sc.numel(), sh.numel(), 1 if inverse else 0,
          _hip.stream_ptr(x.device))
    return y


_zeros = {}


def _zero(device):
    """A one-element zero on ``device`` (the shift of a gradient's point-wise map), allocated once."""
    key = (device.type, device.index)
    if key not in _zeros:
        _zeros[key] = torch.zeros(1, dtype=torch.float32, device=device)
    return _zeros[key]


class _PointwiseAffineFunction(torch.autograd.Function):
    """``pointwise_affine`` with gradients: the HIP kernel forward, reductions over the batch backward
    (y = x s + b: dx = gy s, ds = sum gy x, db = sum gy; inverse y = (x - b) / s: dx = gy / s, ds = -sum gy y / s,
    db = -sum gy / s) -- ActNorm / point-wise affine layers of a flow that is being trained.  For [N, D] float32 device
    gradients with per-feature [D] scale and shift the two sums are one ``fc_column_sums`` and dx the point-wise kernel;
    every other case (4-D inputs, a scalar scale or shift, a double backward) is the torch expression."""

    @staticmethod
    def forward(ctx, inputs, scale, shift, inverse):
        with torch.no_grad():
            outputs = pointwise_affine(inputs, scale, shift, inverse=inverse)
        ctx.save_for_backward(outputs if inverse else inputs, scale, shift)
        ctx.inverse = inverse
        return outputs

    @staticmethod
    def backward(ctx, gy):
        saved, scale, shift = ctx.saved_tensors
        d = gy.shape[-1] if gy.dim() == 2 else -1
        if (not torch.is_grad_enabled() and batch_statistics_route(gy) and saved.shape == gy.shape
                and saved.dtype == torch.float32 and scale.shape == (d,) and shift.shape == (d,)
                and scale.dtype == torch.float32 and scale.device == gy.device):
            gx = None
            if ctx.needs_input_grad[0]:
                gx = pointwise_affine(gy, scale, _zero(gy.device), inverse=ctx.inverse)
            if not (ctx.needs_input_grad[1] or ctx.needs_input_grad[2]):
                return gx, None, None, None
            s1, s2 = column_sums(gy, saved)
            if ctx.inverse:
                return gx, -s2 / scale, -s1 / scale, None
            return gx, s2, s1, None
        s = scale.to(gy.dtype)
        if ctx.inverse:
            gx = gy / s
            gs = -(gx * saved).sum(0)
            gb = -gx.sum(0)
        else:
            gx = gy * s
            gs = (gy * saved).sum(0)
            gb = gy.sum(0)
        return gx, gs.sum_to_size(scale.shape), gb.sum_to_size(shift.shape), None


def pointwise_affine_autograd(inputs, scale, shift, inverse=False):
    """``pointwise_affine``; records an autograd node when gradients are required.  ``scale`` / ``shift`` broadcast
    against one batch item."""
    scale, shift = torch.as_tensor(scale, device=inputs.device), torch.as_tensor(shift, device=inputs.device)
    if torch.is_grad_enabled() and (inputs.requires_grad or scale.requires_grad or shift.requires_grad):
        return _PointwiseAffineFunction.apply(inputs, scale, shift, inverse)
    return pointwise_affine(inputs, scale, shift, inverse=inverse)


def batchnorm_eval(inputs, mean, std, weight, bias, inverse=False):
    """Eval-mode BatchNorm map and its inverse (reference normalization.py:98-141)."""
    lib = _hip.load()
    x = _hip.dev_f32(inputs, "inputs")
    _hip.require_no_grad(inputs)
    n, m = x.shape[0], int(np.prod(x.shape[1:]))
    vecs = [_hip.dev_f32(v.detach().reshape(-1), "batch-norm statistic") for v in (std, bias, mean, weight)]
    for v in vecs:
        if v.numel() != m:
            raise ValueError("Expected features = {}, got {}.".format(v.numel(), m))
    y = torch.empty_like(x)
    _call("fc_pointwise_affine", lib.fc_pointwise_affine, x.device, _hip.ptr(x), _hip.ptr(y),
          _hip.ptr(vecs[0]), _hip.ptr(vecs[1]), _hip.ptr(vecs[2]), _hip.ptr(vecs[3]), n, m, m, m,
          3 if inverse else 2, _hip.stream_ptr(x.device))
    return y


EW_EXP, EW_TANH, EW_LOGTANH, EW_LEAKY_RELU, EW_SIGMOID, EW_SOFTPLUS, EW_CAUCHY_CDF = range(7)
EW_EXTENDED_SOFTPLUS, EW_GLU = 7, 8


def elementwise(inputs, kind, inverse=False, aux=None, p=(0.0, 0.0, 0.0, 0.0), row_sum=True,
                elem_lad=False, may_raise=False):
    """Element-wise bijector ``kind`` (``FC_EW_*``) over ``[N, ...]`` inputs.

    Returns ``(outputs, logabsdet)`` with ``logabsdet`` summed over everything but the batch dim
    (``row_sum``) or left per element (``elem_lad``)."""
    lib = _hip.load()
    x = _hip.dev_f32(inputs, "inputs")
    _hip.require_no_grad(inputs)
    n = x.shape[0]
    m = 1
    for s in x.shape[1:]:
        m *= s
    if aux is not None:
        aux = _hip.dev_f32(torch.as_tensor(aux).detach().to(x.device), "parameter")
    y = torch.empty_like(x)
    lad_row = torch.empty(n, dtype=torch.float32, device=x.device) if row_sum else None
    lad_el = torch.empty_like(x) if elem_lad else None
    err = _err_word(x.device, may_raise)
    p = tuple(float(v) for v in p) + (0.0,) * (4 - len(p))
    _call("fc_elementwise", lib.fc_elementwise, x.device, _hip.ptr(x), _hip.ptr(y), _hip.ptr(lad_row),
          _hip.ptr(lad_el), _hip.ptr(aux), _hip.ptr(err), n, m, kind, 1 if inverse else 0, p[0], p[1], p[2],
          p[3], _hip.stream_ptr(x.device))
    _finish(may_raise)
    return y, (lad_el if elem_lad else lad_row)


_LN2 = 0.6931471805599453
_LOG_PI = 1.1447298858494002


def _tanh_log_derivative(x):
    """log(1 - tanh(x)^2) = 2 (ln 2 - |x| - softplus(-2|x|)): the kernel's form, no cancellation near saturation."""
    ax = x.abs()
    return 2.0 * (_LN2 - ax - F.softplus(-2.0 * ax))


def _atanh_pair(x):
    """atanh(x) and -log(1 - x^2) from log1p(x), log1p(-x)."""
    up, down = torch.log1p(x), torch.log1p(-x)
    return 0.5 * (up - down), -(up + down)


def elementwise_expression(inputs, kind, inverse=False, aux=None, p=(0.0, 0.0, 0.0, 0.0)):
    """Bijector ``kind`` as a differentiable torch expression in the dtype and on the device of ``inputs``: ``(outputs,
    per-element log-derivative)``.  What ``_ElementwiseFunction.backward`` differentiates; the values are those of
    ``fc_elementwise`` to rounding.  Branches are taken with ``where`` on inputs made harmless for the branch not taken,
    so that no 0 * inf reaches a gradient."""
    x = inputs
    p = tuple(float(v) for v in p) + (0.0,) * (4 - len(p))
    if kind == EW_EXP:
        if not inverse:
            return torch.exp(x), x
        y = torch.log(x)
        return y, -y
    if kind == EW_TANH:
        if not inverse:
            return torch.tanh(x), _tanh_log_derivative(x)
        return _atanh_pair(x)
    if kind == EW_LOGTANH:
        cut, alpha, beta, inv_cut = p
        if not inverse:
            mid = ~((x > cut) | (x < -cut))
            xm, xa = torch.where(mid, x, torch.zeros_like(x)), torch.where(mid, torch.ones_like(x), x.abs())
            y = torch.where(mid, torch.tanh(xm), torch.sign(x) * (alpha * torch.log(beta * xa)))
            return y, torch.where(mid, _tanh_log_derivative(xm), torch.log(alpha / xa))
        mid = ~((x > inv_cut) | (x < -inv_cut))
        xm, xa = torch.where(mid, x, torch.zeros_like(x)), torch.where(mid, torch.zeros_like(x), x.abs())
        y_mid, lad_mid = _atanh_pair(xm)
        y = torch.where(mid, y_mid, torch.sign(x) * (torch.exp(xa / alpha) / beta))
        return y, torch.where(mid, lad_mid, -math.log(alpha * beta) + xa / alpha)
    if kind == EW_LEAKY_RELU:
        log_slope = aux.to(x).reshape(())
        y = torch.where(x > 0, x, x * (p[1] if inverse else p[0]))
        lad = torch.where(x < 0, -log_slope if inverse else log_slope, torch.zeros_like(x))
        return y, lad
    if kind == EW_SIGMOID:
        temp = aux.to(x).reshape(())
        if not inverse:
            t = temp * x
            return torch.sigmoid(t), torch.log(temp) - F.softplus(-t) - F.softplus(t)
        xc = torch.clamp(x, p[0], 1 - p[0])
        y = (1 / temp) * (torch.log(xc) - torch.log1p(-xc))
        return y, -(torch.log(temp) - F.softplus(-temp * y) - F.softplus(temp * y))
    if kind == EW_SOFTPLUS:
        thr, eps = p[0], p[1]
        if not inverse:
            return F.softplus(x, beta=1, threshold=thr) + eps, F.logsigmoid(x)
        xi = x - eps
        linear = xi > thr
        y = torch.where(linear, xi, torch.log(torch.expm1(torch.where(linear, torch.ones_like(xi), xi))))
        return y, -torch.log(-torch.expm1(-xi))
    if kind == EW_CAUCHY_CDF:
        if not inverse:
            return (1 / math.pi) * torch.atan(x) + 0.5, -_LOG_PI - torch.log(1 + x ** 2)
        y = torch.tan(math.pi * (x - 0.5))
        return y, _LOG_PI + torch.log(1 + y ** 2)
    if kind == EW_EXTENDED_SOFTPLUS:
        shift = F.softplus(aux.to(x).reshape(x.shape[1:])) + 1e-1
        y = F.softplus(x - shift) - F.softplus(-(x + shift))
        return y, torch.logaddexp(x - torch.logaddexp(shift, x), -F.softplus(shift + x))
    if kind == EW_GLU:
        context = aux.to(x).reshape(x.shape)
        gate = torch.sigmoid(context)
        if not inverse:
            return x * gate, F.logsigmoid(context)
        return x / gate, -F.logsigmoid(context)
    raise ValueError("unknown element-wise bijector kind %r" % (kind,))


class _ElementwiseFunction(torch.autograd.Function):
    """``elementwise`` with gradients: the HIP kernel forward; backward recomputes the bijector from the saved inputs and
    ``aux`` as the float32 torch expression ``elementwise_expression`` on the device and lets ``torch.autograd.grad``
    walk it with ``(grad_outputs, grad_logabsdet)`` -- no HIP backward kernel."""

    @staticmethod
    def forward(ctx, inputs, aux, kind, inverse, p, row_sum, elem_lad, may_raise):
        with torch.no_grad():
            outputs, logabsdet = elementwise(inputs, kind, inverse=inverse, aux=aux, p=p, row_sum=row_sum,
                                             elem_lad=elem_lad, may_raise=may_raise)
        ctx.save_for_backward(inputs, aux)
        ctx.config = (kind, inverse, p, elem_lad)
        return outputs, logabsdet

    @staticmethod
    def backward(ctx, grad_outputs, grad_logabsdet):
        inputs, aux = ctx.saved_tensors
        kind, inverse, p, elem_lad = ctx.config
        with torch.enable_grad():
            x = inputs.detach().requires_grad_(ctx.needs_input_grad[0])
            a = None if aux is None else aux.detach().requires_grad_(ctx.needs_input_grad[1])
            y, lad = elementwise_expression(x, kind, inverse=inverse, aux=a, p=p)
            if not elem_lad and lad.dim() > 1:
                lad = lad.sum(dim=list(range(1, lad.dim())))
            wanted = [t for t, needed in ((x, ctx.needs_input_grad[0]), (a, ctx.needs_input_grad[1])) if needed]
            # (LeakyReLU's outputs do not depend on its log-slope: only what hangs on a wanted tensor is walked)
            walked = [(t, g) for t, g in ((y, grad_outputs), (lad, grad_logabsdet)) if t.requires_grad]
            grads = list(torch.autograd.grad([t for t, _ in walked], wanted, [g for _, g in walked], allow_unused=True))
        gx = grads.pop(0) if ctx.needs_input_grad[0] else None
        ga = grads.pop(0) if ctx.needs_input_grad[1] else None
        return gx, ga, None, None, None, None, None, None


def elementwise_autograd(inputs, kind, inverse=False, aux=None, p=(0.0, 0.0, 0.0, 0.0), row_sum=True,
                         elem_lad=False, may_raise=False):
    """``elementwise``; records an autograd node when ``inputs`` or ``aux`` (temperature, log-slope, context, shift)
    require gradients.  Without one it is ``elementwise`` itself: one launch, the same bits."""
    if aux is not None:
        aux = torch.as_tensor(aux)
    if torch.is_grad_enabled() and (inputs.requires_grad or (aux is not None and aux.requires_grad)):
        return _ElementwiseFunction.apply(inputs, aux, kind, inverse, tuple(p), row_sum, elem_lad, may_raise)
    return elementwise(inputs, kind, inverse=inverse, aux=aux, p=p, row_sum=row_sum, elem_lad=elem_lad,
                       may_raise=may_raise)
