"""RQ-spline coupling bijector with the conditioner's final Linear fused in: the K = 8 linear-tails kernel, the general
one (any K = 4..16, tails or box, hidden <= 256) and the fused backward.
"""
import torch

from flowconductor_amd import _hip
from ._core import _aligned16, _as_cols, _call, _err_word, _finish, _logabsdet_target, _prep_2d, rq_param_count
from .rq import DEFAULT_MIN_BIN_HEIGHT, DEFAULT_MIN_BIN_WIDTH, DEFAULT_MIN_DERIVATIVE, _rq_config
from .packing import FUSED_BINS, FUSED_DT, FUSED_HIDDEN, FUSED_ROWS


def fused_linear_supported(n, d, d_t, hidden, num_bins, tails):
    """Shapes the fused final-layer + RQ-spline kernel is specialised for (the north-star layer)."""
    return (1 <= hidden <= FUSED_HIDDEN and 1 <= d_t <= FUSED_DT and num_bins == FUSED_BINS and tails == "linear"
            and d <= 128 and n >= FUSED_ROWS)


def rq_spline_fused_linear(inputs, hidden, w_pad, bias_pad, cols, *, num_bins, tail_bound,
                           min_bin_width=DEFAULT_MIN_BIN_WIDTH, min_bin_height=DEFAULT_MIN_BIN_HEIGHT,
                           min_derivative=DEFAULT_MIN_DERIVATIVE, wh_divisor=1.0, inverse=False,
                           logabsdet_accum=None, enable_identity_init=False):
    """RQ-spline coupling bijector with the conditioner's final Linear fused in (rows must be a multiple
    of 32).  ``hidden``: [N, 64] input of that Linear.  Returns ``(outputs [N, D], logabsdet [N])``; with
    ``logabsdet_accum`` (f32 [N], contiguous) the kernel adds the layer's logabsdet onto it in place and that
    tensor is returned.  ``enable_identity_init``: the autoregressive form's softplus beta
    (autoregressive.py:612)."""
    lib = _hip.load()
    x = _prep_2d(inputs, align16=True)
    h = _aligned16(_hip.dev_f32(hidden, "hidden"))
    _hip.require_no_grad(inputs, hidden)
    n, d = x.shape
    cols = _as_cols(cols, x.device)
    d_t = cols.numel()
    raw = w_pad.shape[0] == d_t * 23          # the nn.Linear tensors as they are (FC_RQ_RAW_WEIGHTS)
    if (n % FUSED_ROWS != 0 or h.shape != (n, FUSED_HIDDEN) or not 1 <= d_t <= FUSED_DT
            or (not raw and w_pad.shape[0] != -(-d_t // 4) * 4 * 24) or w_pad.shape[1] != FUSED_HIDDEN
            or bias_pad.numel() != w_pad.shape[0]):
        raise ValueError("fused RQ layer: unsupported shapes %s / %s" % (tuple(x.shape), tuple(h.shape)))
    w_pad = _aligned16(_hip.dev_f32(w_pad.detach(), "weight"))
    bias_pad = _hip.dev_f32(bias_pad.detach(), "bias")
    cfg = _rq_config(num_bins, "linear", tail_bound, None, min_bin_width, min_bin_height, min_derivative,
                     enable_identity_init, wh_divisor, inverse)
    y = torch.empty_like(x)
    lad, cfg.flags = _logabsdet_target(logabsdet_accum, n, x.device)      # FC_RQ_ACCUMULATE_LOGABSDET
    if raw:
        cfg.flags |= 4  # FC_RQ_RAW_WEIGHTS
    err = _err_word(x.device, True)
    _call("fc_rq_spline_fused_linear", lib.fc_rq_spline_fused_linear, x.device, _hip.ptr(x), _hip.ptr(y),
          _hip.ptr(h), _hip.ptr(w_pad), _hip.ptr(bias_pad), _hip.ptr(cols), _hip.ptr(lad), _hip.ptr(err), n, d,
          d_t, FUSED_HIDDEN, cfg, _hip.stream_ptr(x.device))
    _finish(True)
    return y, lad


GENERAL_BINS = range(4, 17)
GENERAL_HIDDEN = (64, 128, 256)


def general_hidden_width(hidden):
    """Width (64 / 128 / 256) a hidden activation is zero-padded to for ``fc_rq_spline_fused_general``; None if wider."""
    for w in GENERAL_HIDDEN:
        if hidden <= w:
            return w
    return None


def fused_general_supported(n, d, d_t, hidden, num_bins, tails):
    """Shapes of the general fused final-layer + RQ-spline kernel: K = 4..16, linear tails or none, hidden <= 256,
    <= 32 transformed dims per launch, D <= 128, >= 32 rows."""
    return (general_hidden_width(hidden) is not None and 1 <= d_t <= FUSED_DT and num_bins in GENERAL_BINS
            and tails in (None, "linear") and d <= 128 and n >= FUSED_ROWS)


def rq_fused_linear_backward(inputs, hidden, grad_outputs, grad_logabsdet, packed, packed_t, cols, *, num_bins, tails,
                             tail_bound=1.0, left=0.0, right=1.0, bottom=0.0, top=1.0,
                             min_bin_width=DEFAULT_MIN_BIN_WIDTH, min_bin_height=DEFAULT_MIN_BIN_HEIGHT,
                             min_derivative=DEFAULT_MIN_DERIVATIVE, wh_divisor=1.0, enable_identity_init=False):
    """Gradients of ``rq_spline_fused_general(inputs, hidden, *packed, cols, ...)`` (forward direction, hidden width
    64, rows a multiple of 32): returns ``(grad_inputs [N, D], grad_hidden [N, 64], grad_weight [d_t * P, 64],
    grad_bias [d_t * P])`` for the <= 32 dims of ``cols``.  One launch of ``fc_rq_fused_linear_backward`` (one wave per
    SIMD, ``csrc/fc_rq_fused_backward512.h``): gx / gh deterministic, grad_weight / grad_bias summed with float atomics."""
    lib = _hip.load()
    x = _prep_2d(inputs.detach(), align16=True)
    h = _aligned16(_hip.dev_f32(hidden.detach(), "hidden"))
    gy = _aligned16(_hip.dev_f32(grad_outputs, "grad_outputs"))
    gl = None if grad_logabsdet is None else _hip.dev_f32(grad_logabsdet, "grad_logabsdet")
    n, d = x.shape
    cols = _as_cols(cols, x.device)
    d_t = cols.numel()
    w_frag, w_un, bias_pad = packed
    if n % FUSED_ROWS != 0 or h.shape != (n, 64) or not 1 <= d_t <= FUSED_DT:
        raise ValueError("fused RQ layer backward: unsupported shapes %s / %s" % (tuple(x.shape), tuple(h.shape)))
    cfg = _rq_config(num_bins, tails, tail_bound, (left, right, bottom, top), min_bin_width, min_bin_height,
                     min_derivative, enable_identity_init, wh_divisor, False)
    p = rq_param_count(num_bins, tails)
    pp = bias_pad.shape[-1]
    groups = bias_pad.shape[0]
    gx = torch.empty_like(x)
    gh = torch.empty(n, 64, dtype=torch.float32, device=x.device)
    acc = torch.zeros(groups * 4 * pp * 65, dtype=torch.float32, device=x.device)      # one memset for both accumulators
    gb = acc[:groups * 4 * pp].view(groups, 4, pp)
    gw = acc[groups * 4 * pp:].view(groups, 4, pp, 64)
    args = (_hip.ptr(x), _hip.ptr(h), _hip.ptr(gy), _hip.ptr(gl), _hip.ptr(w_frag), _hip.ptr(w_un),
            _hip.ptr(bias_pad), _hip.ptr(packed_t), _hip.ptr(cols), _hip.ptr(gx), _hip.ptr(gh), _hip.ptr(gb),
            _hip.ptr(gw), n, d, d_t, cfg, _hip.stream_ptr(x.device))
    _call("fc_rq_fused_linear_backward", lib.fc_rq_fused_linear_backward, x.device, 3, *args)      # FC_RQ_BACKWARD_ONE_LAUNCH
    grad_w = gw.reshape(groups * 4, pp, 64)[:d_t, :p].reshape(d_t * p, 64)
    grad_b = gb.reshape(groups * 4, pp)[:d_t, :p].reshape(d_t * p)
    return gx, gh, grad_w, grad_b


def fused_backward_supported(n, d, d_t, hidden, num_bins, tails):
    """Shapes of the fused training path: hidden <= 64, 3K -/+ 1 <= 32 parameters per dim (K <= 10 / 11), <= 32 dims per
    launch, D <= 128."""
    if tails not in (None, "linear") or num_bins not in GENERAL_BINS or hidden > 64:
        return False
    p = rq_param_count(num_bins, tails)
    return p <= 32 and 1 <= d_t <= FUSED_DT and d <= 128 and n >= FUSED_ROWS


def rq_spline_fused_general(inputs, hidden, w_frag, w_unscale, bias_pad, cols, *, num_bins, tails, tail_bound=1.0,
                            left=0.0, right=1.0, bottom=0.0, top=1.0, min_bin_width=DEFAULT_MIN_BIN_WIDTH,
                            min_bin_height=DEFAULT_MIN_BIN_HEIGHT, min_derivative=DEFAULT_MIN_DERIVATIVE,
                            wh_divisor=1.0, inverse=False, logabsdet_accum=None, enable_identity_init=False,
                            streamed_weights=False):
    """RQ-spline coupling bijector with the conditioner's final Linear fused in, general shapes (rows a multiple of
    32; ``hidden`` [N, 64 / 128 / 256] zero-padded; packed weights from ``pack_final_layer_general``).  Semantics and
    return values as ``rq_spline_fused_linear``; without tails inputs outside the box raise InputOutsideDomain.
    ``streamed_weights``: never the resident-weight instances (A/B measurements and tests)."""
    lib = _hip.load()
    x = _prep_2d(inputs, align16=True)
    h = _aligned16(_hip.dev_f32(hidden, "hidden"))
    _hip.require_no_grad(inputs, hidden)
    n, d = x.shape
    cols = _as_cols(cols, x.device)
    d_t = cols.numel()
    hw = h.shape[1]
    if (n % FUSED_ROWS != 0 or h.shape[0] != n or hw not in GENERAL_HIDDEN or not 1 <= d_t <= FUSED_DT
            or w_frag.shape[0] != -(-d_t // 4) or w_frag.shape[1] != hw // 32):
        raise ValueError("general fused RQ layer: unsupported shapes %s / %s" % (tuple(x.shape), tuple(h.shape)))
    cfg = _rq_config(num_bins, tails, tail_bound, (left, right, bottom, top), min_bin_width, min_bin_height,
                     min_derivative, enable_identity_init, wh_divisor, inverse)
    y = torch.empty_like(x)
    lad, cfg.flags = _logabsdet_target(logabsdet_accum, n, x.device)      # FC_RQ_ACCUMULATE_LOGABSDET
    if streamed_weights:
        cfg.flags |= 8  # FC_RQ_STREAMED_WEIGHTS
    err = _err_word(x.device, True)
    _call("fc_rq_spline_fused_general", lib.fc_rq_spline_fused_general, x.device, _hip.ptr(x), _hip.ptr(y),
          _hip.ptr(h), _hip.ptr(w_frag), _hip.ptr(w_unscale), _hip.ptr(bias_pad), _hip.ptr(cols), _hip.ptr(lad),
          _hip.ptr(err), n, d, d_t, hw, cfg, _hip.stream_ptr(x.device))
    _finish(True)
    return y, lad
