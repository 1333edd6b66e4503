"""Sum of sigmoids and the deep sigmoidal flow."""
import math

import numpy as np
import torch

from flowconductor_amd import _hip
from ._core import LAD_STORE, _as_cols, _call, _err_word, _finish, _logabsdet_target, _prep_2d
from .rq import _inverse_through_forward


class _SoSFunction(torch.autograd.Function):
    """``sum_of_sigmoids`` (forward direction, per-sample raw parameters) with its HIP backward kernel
    (``fc_sum_of_sigmoids_backward``: closed-form derivatives of adaptive_sigmoids.py:108-142)."""

    @staticmethod
    def forward(ctx, inputs, raw_params, n_sigmoids, offset, log_scale_postact):
        with torch.no_grad():
            outputs, logabsdet = sum_of_sigmoids(inputs, raw_params, n_sigmoids, offset=offset,
                                                 log_scale_postact=log_scale_postact)
        ctx.save_for_backward(inputs, raw_params)
        ctx.n_sigmoids, ctx.log_post = n_sigmoids, log_scale_postact
        return outputs, logabsdet

    @staticmethod
    def backward(ctx, grad_outputs, grad_logabsdet):
        inputs, raw_params = ctx.saved_tensors
        gx, gp = sum_of_sigmoids_backward(inputs, raw_params, grad_outputs, grad_logabsdet, ctx.n_sigmoids, ctx.log_post)
        return gx, gp, None, None, None


def sum_of_sigmoids_backward(inputs, raw_params, grad_outputs, grad_logabsdet, n_sigmoids, log_scale_postact=0.0):
    """Gradients of ``sum_of_sigmoids(inputs, raw_params, n_sigmoids)`` (forward direction, per-sample rows):
    ``(grad_inputs [N, D], grad_raw_params)``; ``grad_outputs`` / ``grad_logabsdet`` may be None (zeros)."""
    lib = _hip.load()
    x = _prep_2d(inputs.detach())
    p = _hip.dev_f32(raw_params.detach(), "raw_params")
    gy = _hip.dev_f32(grad_outputs if grad_outputs is not None else torch.zeros_like(x), "grad_outputs")
    gl = None if grad_logabsdet is None else _hip.dev_f32(grad_logabsdet, "grad_logabsdet")
    n, d = x.shape
    gx = torch.empty_like(x)
    gp = torch.empty_like(p)
    _call("fc_sum_of_sigmoids_backward", lib.fc_sum_of_sigmoids_backward, x.device, _hip.ptr(x), _hip.ptr(p),
          _hip.ptr(gy), _hip.ptr(gl), _hip.ptr(gx), _hip.ptr(gp), n, d, n_sigmoids, float(log_scale_postact),
          _hip.stream_ptr(x.device))
    return gx, gp.view_as(raw_params)


def sum_of_sigmoids_autograd(inputs, raw_params, n_sigmoids, inverse=False, offset=0.0, iterations=50, lim=120.0,
                             shared_params=False):
    """``sum_of_sigmoids``; with autograd on, the forward kernel sits behind ``_SoSFunction`` (HIP backward kernel; a
    batch-shared parameter row is expanded to per-sample rows, autograd sums its gradient), and the inverse goes through
    ``_inverse_through_forward``."""
    if not (torch.is_grad_enabled() and (inputs.requires_grad or raw_params.requires_grad)):
        return sum_of_sigmoids(inputs, raw_params, n_sigmoids, inverse=inverse, offset=offset, iterations=iterations,
                               lim=lim, shared_params=shared_params)
    x = _prep_2d(inputs)

    def forward_fn(v, raw):
        rows = raw.reshape(1, -1).expand(v.shape[0], -1) if shared_params else raw.reshape(v.shape[0], -1)
        return _SoSFunction.apply(v, rows.contiguous(), n_sigmoids, offset, 0.0)

    if not inverse:
        return forward_fn(x, raw_params)
    return _inverse_through_forward(
        forward_fn, lambda v, raw: sum_of_sigmoids(v, raw, n_sigmoids, inverse=True, offset=offset,
                                                   iterations=iterations, lim=lim, shared_params=shared_params),
        x, raw_params)


def sum_of_sigmoids(inputs, raw_params, n_sigmoids, inverse=False, offset=0.0, iterations=50, lim=120.0,
                    log_scale_postact=0.0, shared_params=False):
    """Sum-of-sigmoids bijector (reference adaptive_sigmoids.py:108-142; inverse base.py:23-83).

    ``raw_params``: ``[N, D, 3S+1]`` per-sample rows, or ``[D, 3S+1]`` with ``shared_params``."""
    lib = _hip.load()
    x = _prep_2d(inputs)
    p = _hip.dev_f32(raw_params, "raw_params")
    _hip.require_no_grad(inputs, raw_params)
    n, d = x.shape
    rowlen = d * (3 * n_sigmoids + 1)
    want = rowlen if shared_params else n * rowlen
    if p.numel() != want:
        raise ValueError("raw_params has %d elements, expected %d" % (p.numel(), want))
    y = torch.empty_like(x)
    lad = torch.empty(n, dtype=torch.float32, device=x.device)
    err = _err_word(x.device, inverse)
    _call("fc_sum_of_sigmoids", lib.fc_sum_of_sigmoids, x.device, _hip.ptr(x), _hip.ptr(y), _hip.ptr(p), None,
          _hip.ptr(lad), _hip.ptr(err), n, d, d, n_sigmoids, 1 if inverse else 0, int(iterations), float(lim),
          float(offset), float(log_scale_postact), 1 if shared_params else 0, LAD_STORE,
          _hip.stream_ptr(x.device))
    _finish(inverse)
    return y, lad


def deep_sigmoid_bound(eps):
    """The range of the deep sigmoidal flow is ``|y| < log((1 - eps / 2) / (eps / 2))``: the float32 bound the inverse kernel
    tests against (it sees ``eps`` as a float32)."""
    e = float(np.float32(eps))
    return float(np.float32(math.log((1.0 - 0.5 * e) / (0.5 * e))))


def deep_sigmoid_fits(d, d_t, n_sigmoids):
    """Whether one sample's rows fit the tile kernels' LDS plan (``plan_tile`` of csrc/fc_tile.h at one sample per tile,
    150 KiB); beyond it the modules take the torch composition."""
    def round4(v):
        return (v + 3) & ~3
    return 4 * (round4(d_t * 3 * n_sigmoids) + round4(d) + round4(d_t)) <= 150 * 1024


def deep_sigmoid(inputs, raw_params, n_sigmoids, inverse=False, mollify=0.0, eps=1e-4, prescale=1.0, iterations=100,
                 lim=10.0, shared_params=False, cols=None, lad_mode=LAD_STORE, logabsdet=None):
    """Deep sigmoidal flow (reference adaptive_sigmoids.py:177-210; the inverse is this project's, see
    csrc/fc_deep_sigmoid.hip) over ``inputs[:, cols]`` (all columns if ``cols`` is None).

    ``raw_params``: ``[N, d_t, 3S]`` per-sample rows ``[S raw_a | S raw_b | S raw_w]``, or ``[d_t, 3S]`` with
    ``shared_params``; every raw value is multiplied by ``prescale`` first.  ``lad_mode``: one of the ``LAD_*`` modes;
    the accumulating ones add onto ``logabsdet`` ([N], float32) in place.  Inverse inputs outside the range of the map
    raise ``InputOutsideDomain`` (deferred inside ``deferred_errors``)."""
    lib = _hip.load()
    x = _prep_2d(inputs)
    p = _hip.dev_f32(raw_params, "raw_params")
    _hip.require_no_grad(inputs, raw_params)
    n, d = x.shape
    cols = _as_cols(cols, x.device)
    d_t = d if cols is None else cols.numel()
    rowlen = d_t * 3 * n_sigmoids
    want = rowlen if shared_params else n * rowlen
    if p.numel() != want:
        raise ValueError("raw_params has %d elements, expected %d" % (p.numel(), want))
    y = torch.empty_like(x)
    if lad_mode & 1:
        if logabsdet is None:
            raise ValueError("an accumulating lad_mode needs the running logabsdet")
        lad, _ = _logabsdet_target(logabsdet, n, x.device)
    else:
        lad = torch.empty(n, dtype=torch.float32, device=x.device)
    err = _err_word(x.device, inverse)
    _call("fc_deep_sigmoid", lib.fc_deep_sigmoid, x.device, _hip.ptr(x), _hip.ptr(y), _hip.ptr(p), _hip.ptr(cols),
          _hip.ptr(lad), _hip.ptr(err), n, d, d_t, n_sigmoids, 1 if inverse else 0, int(iterations), float(lim),
          float(mollify), float(eps), float(prescale), 1 if shared_params else 0, int(lad_mode),
          _hip.stream_ptr(x.device))
    _finish(inverse)
    return y, lad


class _DeepSigmoidFunction(torch.autograd.Function):
    """``deep_sigmoid`` (forward direction, all columns) with its HIP backward kernel (``fc_deep_sigmoid_backward``).  A
    batch-shared row gets its gradient summed over the batch inside the kernel: no ``[N, D, 3S]`` tensor exists."""

    @staticmethod
    def forward(ctx, inputs, raw_params, n_sigmoids, mollify, eps, prescale, shared_params):
        with torch.no_grad():
            outputs, logabsdet = deep_sigmoid(inputs, raw_params, n_sigmoids, mollify=mollify, eps=eps,
                                              prescale=prescale, shared_params=shared_params)
        ctx.save_for_backward(inputs, raw_params)
        ctx.cfg = (n_sigmoids, mollify, eps, prescale, shared_params)
        return outputs, logabsdet

    @staticmethod
    def backward(ctx, grad_outputs, grad_logabsdet):
        inputs, raw_params = ctx.saved_tensors
        n_sigmoids, mollify, eps, prescale, shared = ctx.cfg
        lib = _hip.load()
        x = _prep_2d(inputs.detach())
        p = _hip.dev_f32(raw_params.detach(), "raw_params")
        gy = _hip.dev_f32(grad_outputs if grad_outputs is not None else torch.zeros_like(x), "grad_outputs")
        gl = None if grad_logabsdet is None else _hip.dev_f32(grad_logabsdet, "grad_logabsdet")
        n, d = x.shape
        gx = torch.empty_like(x)
        if shared:
            rows = lib.fc_deep_sigmoid_backward_rows(n, d, n_sigmoids)
            buf = torch.empty((1 + rows, p.numel()), dtype=torch.float32, device=x.device)   # gradient row + partial sums
            gp = buf[0]
        else:
            buf = gp = torch.empty_like(p)
        _call("fc_deep_sigmoid_backward", lib.fc_deep_sigmoid_backward, x.device, _hip.ptr(x), _hip.ptr(p), _hip.ptr(gy),
              _hip.ptr(gl), _hip.ptr(gx), _hip.ptr(buf), n, d, n_sigmoids, float(mollify), float(eps), float(prescale),
              1 if shared else 0, _hip.stream_ptr(x.device))
        return gx, gp.view_as(raw_params), None, None, None, None, None


def deep_sigmoid_autograd(inputs, raw_params, n_sigmoids, inverse=False, mollify=0.0, eps=1e-4, prescale=1.0,
                          iterations=100, lim=10.0, shared_params=False):
    """``deep_sigmoid``; with autograd on, the forward kernel sits behind ``_DeepSigmoidFunction`` (HIP backward kernel;
    a batch-shared row keeps its shape unless it is too long for the in-kernel reduction, then it is expanded to
    per-sample rows and autograd sums), and the inverse goes through ``_inverse_through_forward``."""
    kw = dict(mollify=mollify, eps=eps, prescale=prescale)
    if not (torch.is_grad_enabled() and (inputs.requires_grad or raw_params.requires_grad)):
        return deep_sigmoid(inputs, raw_params, n_sigmoids, inverse=inverse, iterations=iterations, lim=lim,
                            shared_params=shared_params, **kw)
    x = _prep_2d(inputs)
    n, d = x.shape
    reduce_in_kernel = shared_params and _hip.load().fc_deep_sigmoid_backward_rows(n, d, n_sigmoids) > 0

    def forward_fn(v, raw):
        if shared_params and not reduce_in_kernel:
            raw = raw.reshape(1, -1).expand(v.shape[0], -1)
        return _DeepSigmoidFunction.apply(v, raw.contiguous(), n_sigmoids, mollify, eps, prescale, reduce_in_kernel)

    if not inverse:
        return forward_fn(x, raw_params)
    return _inverse_through_forward(
        forward_fn, lambda v, raw: deep_sigmoid(v, raw, n_sigmoids, inverse=True, iterations=iterations, lim=lim,
                                                shared_params=shared_params, **kw),
        x, raw_params)
