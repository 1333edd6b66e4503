"""Permutation, batch-shared point-wise affine, eval-mode batch norm and the element-wise non-linearities."""
import numpy as np
import torch

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
