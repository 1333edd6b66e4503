"""Affine / additive coupling on given shift and scale rows, and the base-distribution epilogue."""
import torch

from flowconductor_amd import _hip
from ._core import _as_cols, _call, _logabsdet_target, _prep_2d
from .rq import _inverse_through_forward


AFFINE_SIGMOID_PLUS2 = 0
AFFINE_SOFTPLUS_CLAMP3 = 1
AFFINE_SCALE_GIVEN = 2
AFFINE_ADDITIVE = 3
AFFINE_MAF_SOFTPLUS = 4
AFFINE_SHIFT_TANH2 = 5
AFFINE_SCALE_SOFTPLUS = 6


def affine_coupling(inputs, params, cols=None, *, activation=AFFINE_SIGMOID_PLUS2, inverse=False,
                    shared_params=False, logabsdet_accum=None):
    """Affine bijector on ``inputs[:, cols]`` with per-sample ``params`` rows; records an autograd node when
    gradients are required (forward direction, per-sample parameters).  See ``_affine_coupling_nograd``.
    ``logabsdet_accum``: running total the kernel adds onto (no-grad calls; otherwise added here)."""
    if torch.is_grad_enabled() and (inputs.requires_grad or params.requires_grad):
        if shared_params:
            raise RuntimeError("flowconductor_amd: gradients are implemented for the affine bijector with "
                               "per-sample parameters; wrap other calls in torch.no_grad().")
        if inverse:
            outputs, logabsdet = _inverse_through_forward(
                lambda y, p: _AffineFunction.apply(y, p, cols, activation),
                lambda x, p: _affine_coupling_nograd(x, p, cols, activation=activation, inverse=True), inputs, params)
        else:
            outputs, logabsdet = _AffineFunction.apply(inputs, params, cols, activation)
        if logabsdet_accum is not None:
            logabsdet_accum += logabsdet
            logabsdet = logabsdet_accum
        return outputs, logabsdet
    return _affine_coupling_nograd(inputs, params, cols, activation=activation, inverse=inverse,
                                   shared_params=shared_params, logabsdet_accum=logabsdet_accum)


class _AffineFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, inputs, params, cols, activation):
        with torch.no_grad():
            outputs, logabsdet = _affine_coupling_nograd(inputs, params, cols, activation=activation)
        ctx.save_for_backward(inputs, params)
        ctx.cols, ctx.activation = cols, activation
        return outputs, logabsdet

    @staticmethod
    def backward(ctx, grad_outputs, grad_logabsdet):
        inputs, params = ctx.saved_tensors
        lib = _hip.load()
        x = _prep_2d(inputs.detach())
        p = _hip.dev_f32(params.detach(), "params")
        gy = _hip.dev_f32(grad_outputs if grad_outputs is not None else torch.zeros_like(x), "grad_outputs")
        gl = None if grad_logabsdet is None else _hip.dev_f32(grad_logabsdet, "grad_logabsdet")
        n, d = x.shape
        cols = _as_cols(ctx.cols, x.device)
        d_t = d if cols is None else cols.numel()
        gx = gy.clone()                   # identity columns pass the upstream gradient through
        gp = torch.zeros_like(p)
        _call("fc_affine_backward", lib.fc_affine_backward, x.device, _hip.ptr(x), _hip.ptr(p), _hip.ptr(cols),
              _hip.ptr(gy), _hip.ptr(gl), _hip.ptr(gx), _hip.ptr(gp), n, d, d_t, ctx.activation,
              _hip.stream_ptr(x.device))
        return gx, gp.view_as(params), None, None


def _affine_coupling_nograd(inputs, params, cols=None, *, activation=AFFINE_SIGMOID_PLUS2, inverse=False,
                            shared_params=False, logabsdet_accum=None):
    """Affine bijector on ``inputs[:, cols]`` with per-sample ``params`` rows.

    Row layouts per ``activation``: see ``FC_AFFINE_*`` in include/flowcon_hip.h.
    Semantics: reference coupling.py:234-269, autoregressive/autoregressive.py:97-129.
    With ``logabsdet_accum`` (contiguous f32 [N]) the kernel adds the layer's logabsdet onto it and returns it.
    """
    lib = _hip.load()
    x = _prep_2d(inputs)
    p = _hip.dev_f32(params, "params")
    _hip.require_no_grad(inputs, params)
    n, d = x.shape
    cols = _as_cols(cols, x.device)
    d_t = d if cols is None else cols.numel()
    rowlen = d_t if activation in (AFFINE_ADDITIVE, AFFINE_SHIFT_TANH2, AFFINE_SCALE_SOFTPLUS) else 2 * d_t
    want = rowlen if shared_params else n * rowlen
    if p.numel() != want:
        raise ValueError("params has %d elements, expected %d" % (p.numel(), want))
    y = torch.empty_like(x)
    lad, accumulate = _logabsdet_target(logabsdet_accum, n, x.device)      # LAD_STORE / LAD_ACCUMULATE
    _call("fc_affine", lib.fc_affine, x.device, _hip.ptr(x), _hip.ptr(y), _hip.ptr(p), _hip.ptr(cols),
          _hip.ptr(lad), n, d, d_t, activation, 1 if inverse else 0, 1 if shared_params else 0,
          accumulate, _hip.stream_ptr(x.device))
    return y, lad


def _standard_normal_log_prob_nograd(noise, log_z, add=None):
    """``-0.5 * sum(noise**2, 1) - log_z (+ add)`` -> [N]  (reference distributions/normal.py:23-33)."""
    lib = _hip.load()
    z = _hip.dev_f32(noise, "inputs")
    _hip.require_no_grad(noise, add)
    n = z.shape[0]
    z2 = z.flatten(1) if z.dim() > 1 else z.reshape(n, 1)
    if add is not None:
        add = _hip.dev_f32(add, "logabsdet")
        if add.numel() != n:
            raise ValueError("logabsdet must have one entry per row")
    out = torch.empty(n, dtype=torch.float32, device=z.device)
    _call("fc_standard_normal_log_prob", lib.fc_standard_normal_log_prob, z.device, _hip.ptr(z2),
          _hip.ptr(add), _hip.ptr(out), n, z2.shape[1], float(log_z), _hip.stream_ptr(z.device))
    return out


class _StdNormalLogProbFunction(torch.autograd.Function):
    """Gradient of ``-0.5 * sum(z**2) - log_z + add``: ``-z`` per element, 1 for ``add`` (plain torch ops)."""

    @staticmethod
    def forward(ctx, noise, add, log_z):
        with torch.no_grad():
            out = _standard_normal_log_prob_nograd(noise, log_z, add)
        ctx.save_for_backward(noise)
        ctx.has_add = add is not None
        return out

    @staticmethod
    def backward(ctx, grad):
        (noise,) = ctx.saved_tensors
        gz = -noise * grad.reshape((-1,) + (1,) * (noise.dim() - 1))
        return gz, (grad if ctx.has_add else None), None


def standard_normal_log_prob(noise, log_z, add=None):
    """``-0.5 * sum(noise**2, 1) - log_z (+ add)`` -> [N]  (reference distributions/normal.py:23-33); records
    an autograd node when gradients are required."""
    if torch.is_grad_enabled() and (noise.requires_grad or (add is not None and add.requires_grad)):
        return _StdNormalLogProbFunction.apply(noise, add, log_z)
    return _standard_normal_log_prob_nograd(noise, log_z, add)
