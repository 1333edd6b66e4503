"""Rational-quadratic spline: the stand-alone kernel, its backward and the autograd wrappers."""
import math

import numpy as np
import torch

from flowconductor_amd import _hip, options
from ._core import LAD_STORE, _as_cols, _call, _err_word, _finish, _prep_2d, rq_param_count


DEFAULT_MIN_BIN_WIDTH = 1e-3
DEFAULT_MIN_BIN_HEIGHT = 1e-3
DEFAULT_MIN_DERIVATIVE = 1e-3
RQ_BACKWARD_MAX_BINS = 32      # kMaxBinsBwd of csrc/fc_rq_backward_op.h


def _rq_config(num_bins, tails, tail_bound, box, min_bin_width, min_bin_height, min_derivative,
               enable_identity_init, wh_divisor, inverse):
    cfg = _hip.RQConfig()
    cfg.num_bins = num_bins
    cfg.tails = 0 if tails is None else 1
    cfg.inverse = 1 if inverse else 0
    if tails == "linear":
        cfg.left, cfg.right, cfg.bottom, cfg.top = -tail_bound, tail_bound, -tail_bound, tail_bound
    else:
        cfg.left, cfg.right, cfg.bottom, cfg.top = box
    cfg.min_bin_width = min_bin_width
    cfg.min_bin_height = min_bin_height
    cfg.min_derivative = min_derivative
    cfg.wh_divisor = wh_divisor
    cfg.softplus_beta = (math.log(2) / (1 - min_derivative)) if enable_identity_init else 1.0
    cfg.tail_constant = float(np.log(np.exp(1 - min_derivative) - 1))
    return cfg


def rq_spline(inputs, params, cols=None, *, num_bins, tails=None, tail_bound=1.0,
              left=0.0, right=1.0, bottom=0.0, top=1.0,
              min_bin_width=DEFAULT_MIN_BIN_WIDTH, min_bin_height=DEFAULT_MIN_BIN_HEIGHT,
              min_derivative=DEFAULT_MIN_DERIVATIVE, enable_identity_init=False,
              wh_divisor=1.0, inverse=False, shared_params=False, out=None):
    """RQ spline over ``inputs[:, cols]`` (all columns if ``cols`` is None).

    ``params``: ``[N, d_t * (3K -/+ 1)]`` per-sample rows, or ``[d_t * (3K -/+ 1)]`` with
    ``shared_params``.  Returns ``(outputs [N, D], logabsdet [N])``; other columns are copied.
    Semantics: reference splines/rational_quadratic.py:13-181.
    """
    lib = _hip.load()
    x = _prep_2d(inputs)
    p = _hip.dev_f32(params, "params")
    _hip.require_no_grad(inputs, params)
    n, d = x.shape
    cols = _as_cols(cols, x.device)
    d_t = d if cols is None else cols.numel()
    if tails not in (None, "linear"):
        raise RuntimeError("{} tails are not implemented.".format(tails))
    mult = rq_param_count(num_bins, tails)
    if min_bin_width * num_bins > 1.0:
        raise ValueError("Minimal bin width too large for the number of bins")
    if min_bin_height * num_bins > 1.0:
        raise ValueError("Minimal bin height too large for the number of bins")
    rowlen = d_t * mult
    want = rowlen if shared_params else n * rowlen
    if p.numel() != want:
        raise ValueError("params has %d elements, expected %d" % (p.numel(), want))

    cfg = _rq_config(num_bins, tails, tail_bound, (left, right, bottom, top), min_bin_width, min_bin_height,
                     min_derivative, enable_identity_init, wh_divisor, inverse)

    if options.get("rq_force_tile"):
        cfg.flags |= 2  # FC_RQ_FORCE_TILE
    y = torch.empty_like(x) if out is None else out
    lad = torch.empty(n, dtype=torch.float32, device=x.device)
    err = _err_word(x.device, True)
    _call("fc_rq_spline", lib.fc_rq_spline, x.device, _hip.ptr(x), _hip.ptr(y), _hip.ptr(p),
          _hip.ptr(cols), _hip.ptr(lad), _hip.ptr(err), n, d, d_t, 1 if shared_params else 0,
          LAD_STORE, cfg, _hip.stream_ptr(x.device))
    _finish(True)
    return y, lad


def rq_spline_backward(inputs, params, cols, grad_outputs, grad_logabsdet, **kw):
    """Gradients of ``rq_spline(inputs, params, cols, **kw)`` (forward direction, per-sample params):
    returns ``(grad_inputs [N, D], grad_params [N, d_t * P])``; identity columns pass ``grad_outputs`` through."""
    lib = _hip.load()
    x = _prep_2d(inputs.detach())
    p = _hip.dev_f32(params.detach(), "params")
    gy = _hip.dev_f32(grad_outputs, "grad_outputs")
    n, d = x.shape
    cols = _as_cols(cols, x.device)
    d_t = d if cols is None else cols.numel()
    tails = kw.get("tails")
    cfg = _rq_config(kw["num_bins"], tails, kw.get("tail_bound", 1.0),
                     (kw.get("left", 0.0), kw.get("right", 1.0), kw.get("bottom", 0.0), kw.get("top", 1.0)),
                     kw.get("min_bin_width", DEFAULT_MIN_BIN_WIDTH), kw.get("min_bin_height", DEFAULT_MIN_BIN_HEIGHT),
                     kw.get("min_derivative", DEFAULT_MIN_DERIVATIVE), kw.get("enable_identity_init", False),
                     kw.get("wh_divisor", 1.0), False)
    gl = None if grad_logabsdet is None else _hip.dev_f32(grad_logabsdet, "grad_logabsdet")
    gx = torch.empty_like(gy)             # every column is written (identity columns: grad_outputs)
    gp = torch.empty_like(p)
    _call("fc_rq_spline_backward", lib.fc_rq_spline_backward, x.device, _hip.ptr(x), _hip.ptr(p), _hip.ptr(cols),
          _hip.ptr(gy), _hip.ptr(gl), _hip.ptr(gx), _hip.ptr(gp), n, d, d_t, cfg, _hip.stream_ptr(x.device))
    return gx, gp.view_as(params)


class _RQSplineFunction(torch.autograd.Function):
    """``rq_spline`` with gradients (forward direction): the HIP forward and backward kernels behind autograd, so
    that ``-flow.log_prob(x).mean().backward()`` trains through this path (reference: examples/toy_2d.py:57-68)."""

    @staticmethod
    def forward(ctx, inputs, params, cols, kw):
        with torch.no_grad():
            outputs, logabsdet = rq_spline(inputs, params, cols, **kw)
        ctx.save_for_backward(inputs, params)
        ctx.cols, ctx.kw = cols, kw
        return outputs, logabsdet

    @staticmethod
    def backward(ctx, grad_outputs, grad_logabsdet):
        inputs, params = ctx.saved_tensors
        if grad_outputs is None:
            grad_outputs = torch.zeros_like(inputs)
        gx, gp = rq_spline_backward(inputs, params, ctx.cols, grad_outputs.contiguous(), grad_logabsdet, **ctx.kw)
        return gx, gp, None, None


def _inverse_through_forward(forward_fn, inverse_nograd_fn, inputs, params):
    """Differentiable inverse of an element-wise bijector whose gradients exist for the forward direction only
    (sampling / reverse-KL training through ``Flow.sample``, ``sample_and_log_prob``): the inverse kernel finds
    ``y0 = f^-1(x; p)`` without a graph, then one Newton-shaped step ``y = y0 - (f(y0; p) - x) / f'(y0)`` through the
    differentiable forward op carries the implicit-function gradients ``dy/dx = 1 / f'``, ``dy/dp = -(df/dp) / f'``
    (its value only removes the inverse's rounding residual), and ``logabsdet = -logabsdet_f(y; p)`` is the forward op
    evaluated at that ``y``.  Three kernel passes instead of one; ``f'`` per element comes from the backward kernel."""
    with torch.no_grad():
        y0, _ = inverse_nograd_fn(inputs, params)
    y0 = y0.detach().requires_grad_(True)
    with torch.enable_grad():
        x_hat, _ = forward_fn(y0, params)
        fprime, = torch.autograd.grad(x_hat.sum(), y0, retain_graph=True)
        y = y0.detach() - (x_hat - inputs) / fprime.detach()
        _, logabsdet = forward_fn(y, params)
    return y, -logabsdet


def rq_spline_autograd(inputs, params, cols=None, **kw):
    """``rq_spline`` that records an autograd node when gradients are required (per-sample parameters; the inverse
    direction through ``_inverse_through_forward``); otherwise exactly ``rq_spline``."""
    needs = torch.is_grad_enabled() and (inputs.requires_grad or params.requires_grad)
    if not needs:
        return rq_spline(inputs, params, cols, **kw)
    if kw.get("shared_params"):
        raise RuntimeError("flowconductor_amd: gradients are implemented for the RQ spline with per-sample "
                           "parameters; wrap other calls in torch.no_grad().")
    if kw["num_bins"] > RQ_BACKWARD_MAX_BINS:
        raise NotImplementedError("autograd through the RQ spline needs num_bins <= %d (fc_rq_spline_backward); got "
                                  "num_bins = %d" % (RQ_BACKWARD_MAX_BINS, kw["num_bins"]))
    if kw.get("inverse"):
        fwd_kw = dict(kw, inverse=False)
        return _inverse_through_forward(lambda y, p: _RQSplineFunction.apply(y, p, cols, fwd_kw),
                                        lambda x, p: rq_spline(x, p, cols, **kw), inputs, params)
    return _RQSplineFunction.apply(inputs, params, cols, kw)
