"""Conditioner drivers: the hidden stack of a ResidualNet / MADE (64-wide, wide, backward), the one-kernel affine coupling
layer and the one-kernel autoregressive inverse.
"""
import torch

from flowconductor_amd import _hip
from ._core import _aligned16, _as_cols, _call, _err_word, _finish, _logabsdet_target, _prep_2d
from .rq import DEFAULT_MIN_BIN_HEIGHT, DEFAULT_MIN_BIN_WIDTH, DEFAULT_MIN_DERIVATIVE, _rq_config
from .splines import SPLINE_LINEAR, _spline_config, spline_multiplier
from .affine import AFFINE_ADDITIVE, AFFINE_MAF_SOFTPLUS, AFFINE_SIGMOID_PLUS2, AFFINE_SOFTPLUS_CLAMP3


HIDDEN_ROWS = 16

ACT_RELU, ACT_TANH, ACT_SILU, ACT_ELU, ACT_LEAKY_RELU, ACT_SIGMOID = range(6)


def activation_code(fn):
    """``(FC_ACT_* code, parameter)`` of an activation callable / module the hidden-layer kernel knows, else None."""
    import torch.nn as nn
    from torch.nn import functional as F

    if isinstance(fn, nn.ReLU) or fn in (F.relu, torch.relu):
        return ACT_RELU, 0.0
    if isinstance(fn, nn.Tanh) or fn in (torch.tanh, F.tanh):
        return ACT_TANH, 0.0
    if isinstance(fn, nn.SiLU) or fn is F.silu:
        return ACT_SILU, 0.0
    if isinstance(fn, nn.ELU):
        return ACT_ELU, float(fn.alpha)
    if fn is F.elu:
        return ACT_ELU, 1.0
    if isinstance(fn, nn.LeakyReLU):
        return ACT_LEAKY_RELU, float(fn.negative_slope)
    if fn is F.leaky_relu:
        return ACT_LEAKY_RELU, 0.01
    if isinstance(fn, nn.Sigmoid) or fn in (torch.sigmoid, F.sigmoid):
        return ACT_SIGMOID, 0.0
    return None


CONTEXT_GLU, CONTEXT_ADDITIVE = 1, 2

WIDE_ROWS = 64

HIDDEN_BWD_ROWS = 128

MADE_AFFINE, MADE_RQ = 0, 1
# forms with entries of their own: the mixture sampler is 2 (FC_MADE_MOG, ops/mog.py)
MADE_SOS, MADE_SPLINE = 3, 4


def made_inverse_param_limit(kind):
    """Parameters per dim the device loop holds for ``kind``: six 16-row tiles for the sum of sigmoids (S <= 31; the
    reference's default S = 30 has 91), three for every other form."""
    return 96 if kind == MADE_SOS else 48


# Rows x sigmoids up to which ``fc_made_inverse_sos`` beats the host loop (MI355X, DESIGN.md "Device loop: sum-of-sigmoids
# and sibling splines"): one lane per sample runs the root search, so beyond one full round of the chip (2^15 rows) the kernel
# grows with rows x S, while the host loop's stand-alone kernel spreads the elements over all lanes.  Measured at S = 6, 15,
# 30 and D = 8, 32, 64: ahead at every shape up to 2^16 rows x 30 sigmoids, level or behind at twice that.
MADE_SOS_ROW_SIGMOIDS = 30 << 16


def made_inverse_row_limit(kind, per_dim):
    """Most rows for which the device loop of ``kind`` is the default route, or None for no limit (the affine,
    rational-quadratic and sibling-spline forms win at every measured size)."""
    if kind != MADE_SOS:
        return None
    return MADE_SOS_ROW_SIGMOIDS // max(1, (per_dim - 1) // 3)


def _made_lds_bytes(features, num_blocks, per_dim, with_context):
    """LDS of the device loop at one 16-row block per wave: fc_made_inverse.h ``mi_lds_bytes`` (the hidden stack's image and
    the waves' parameter strips) and, with a context, ``mi_ctx_lds_bytes`` (the context layers' images behind them)."""
    k0s = 1 if features <= 32 else 2
    pt = -(-per_dim // 16)
    image = (k0s * 8 + 2 * num_blocks * 16) * 1024 + (1 + 2 * num_blocks) * 256 + 64 + 8 * 16 * (16 * pt + 4) * 4
    return image + ((1 + num_blocks) * (8 * 1024 + 256) + 64 if with_context else 0)


def made_inverse_form_fits(features, num_blocks, per_dim):
    """``fc_made_inverse_sos`` / ``fc_made_inverse_spline`` in 160 KB: all but D > 32, three blocks, six parameter tiles."""
    return (0 <= num_blocks <= 3 and features <= 64 and 1 <= per_dim <= 96
            and _made_lds_bytes(features, num_blocks, per_dim, False) <= 160 * 1024)


def made_inverse_context_fits(features, num_blocks, per_dim):
    """``fc_made_inverse_context`` / ``fc_made_mog_sample_context`` in 160 KB."""
    return (num_blocks <= 3 and features <= 64 and per_dim <= 48
            and _made_lds_bytes(features, num_blocks, per_dim, True) <= 160 * 1024)


def _made_pack_matches(packed, d):
    """``units_needed`` of a ``pack_made_inverse`` pack holds one int32 per dim."""
    return packed[6].dtype == torch.int32 and packed[6].numel() == d


def _made_context_pack(caller, rows_name, device, n, d, context, context_pack, num_blocks, per_dim, count, unit):
    """``context_pack`` once it, the ``context`` of the [n, d] rows and the shape are what ``fc_<caller>_context`` takes."""
    if (not torch.is_tensor(context) or context.dtype != torch.float32 or context.dim() != 2 or context.shape[0] != n
            or not 1 <= context.shape[1] <= 32 or not context.is_contiguous() or context.device != device):
        raise ValueError("%s: context must be a contiguous float32 [N, C <= 32] tensor on the %s device" % (caller, rows_name))
    if not made_inverse_context_fits(d, num_blocks, per_dim):
        raise ValueError("fc_%s_context has no instantiation for D = %d, %d blocks, %d %s" % (caller, d, num_blocks, count, unit))
    cf, cu, cb = context_pack
    if cf.numel() != (1 + num_blocks) * 4096 or cu.numel() != 1 + num_blocks or cb.numel() != (1 + num_blocks) * 64:
        raise ValueError("%s: context_pack does not match num_blocks = %d" % (caller, num_blocks))
    return cf, cu, cb


def _made_arguments(rows, outputs, packed, context_pack, n, d, num_blocks, tail):
    """The arguments all six device-loop entries take: the input rows (the context last of them), the two outputs, the hidden
    stack's image (, the context layers': ``context_pack``), the final layer's with ``units_needed`` (, the error word, last
    in ``outputs``); n, d (, C), num_blocks, the form's ``tail``, the stream.  The tensors go as plain addresses."""
    tensors = (*rows, *outputs[:2], *packed[:3], *context_pack, *packed[3:], *outputs[2:])
    sizes = (n, d, rows[-1].shape[1], num_blocks) if context_pack else (n, d, num_blocks)
    return (*[t.data_ptr() for t in tensors], *sizes, *tail, _hip.stream_ptr(rows[0].device))


def _made_inverse_entry(kind, d, num_blocks, per_dim, form, with_context=False, flags=0):
    """``(entry, its arguments from num_blocks to the stream)`` for ``kind`` and its keyword arguments ``form``; raises what
    the entries do not hold.  Touches neither the library nor a device.  ``flags``: 1 to add onto the logabsdet."""
    if kind in (MADE_AFFINE, MADE_RQ):
        cfg = None
        if kind == MADE_RQ:
            rq = dict(form)
            cfg = _rq_config(rq.pop("num_bins"), rq.pop("tails"), rq.pop("tail_bound", 1.0),
                             (rq.pop("left", 0.0), rq.pop("right", 1.0), rq.pop("bottom", 0.0), rq.pop("top", 1.0)),
                             rq.pop("min_bin_width", DEFAULT_MIN_BIN_WIDTH), rq.pop("min_bin_height", DEFAULT_MIN_BIN_HEIGHT),
                             rq.pop("min_derivative", DEFAULT_MIN_DERIVATIVE), rq.pop("enable_identity_init", False),
                             rq.pop("wh_divisor", 1.0), True)
            if rq:
                raise TypeError("made_inverse: unknown spline arguments %s" % sorted(rq))
        if flags:
            cfg = cfg or _hip.RQConfig()          # affine form: only the flags are read
            cfg.flags = flags
        return "fc_made_inverse_context" if with_context else "fc_made_inverse", (per_dim, kind, cfg)
    if with_context:
        raise ValueError("made_inverse: the sum-of-sigmoids and sibling-spline forms take no context")
    form = dict(form)
    if kind == MADE_SOS:
        sigmoids = form.pop("n_sigmoids")
        want = 3 * sigmoids + 1
        name, tail = "fc_made_inverse_sos", (sigmoids, int(form.pop("iterations", 50)), float(form.pop("lim", 120.0)),
                                             float(form.pop("offset", 0.0)), float(form.pop("log_scale_postact", 0.0)))
    else:
        spline, bins, tails = form.pop("kind"), form.pop("num_bins"), form.pop("tails", None)
        if tails not in (None, "linear"):
            raise RuntimeError("{} tails are not implemented.".format(tails))
        want = spline_multiplier(spline, bins, tails)
        min_w = form.pop("min_bin_width", DEFAULT_MIN_BIN_WIDTH)
        min_h = form.pop("min_bin_height", DEFAULT_MIN_BIN_HEIGHT)
        if spline != SPLINE_LINEAR and (min_w * bins > 1.0 or min_h * bins > 1.0):
            raise ValueError("Minimal bin width / height too large for the number of bins")
        cfg = _spline_config(spline, bins, tails, form.pop("tail_bound", 1.0),
                             (form.pop("left", 0.0), form.pop("right", 1.0), form.pop("bottom", 0.0), form.pop("top", 1.0)),
                             min_w, min_h, form.pop("width_divisor", 1.0), form.pop("height_divisor", 1.0), True)
        name, tail = "fc_made_inverse_spline", (cfg,)
    if form:
        raise TypeError("made_inverse: unknown arguments %s" % sorted(form))
    if per_dim != want or per_dim > made_inverse_param_limit(kind) or not made_inverse_form_fits(d, num_blocks, per_dim):
        raise ValueError("made_inverse: no instantiation for D = %d, %d blocks, %d parameters per dim (the form has %d)"
                         % (d, num_blocks, per_dim, want))
    return name, tail + (flags,)


def made_inverse(inputs, packed, num_blocks, per_dim, kind, rq=None, logabsdet_accum=None, context=None, context_pack=None):
    """The D passes of an autoregressive inverse in ONE kernel (``fc_made_inverse``): ``inputs`` [N, D <= 64] (rows a
    multiple of 16), ``packed`` from ``pack_made_inverse``; ``kind`` ``MADE_AFFINE`` or ``MADE_RQ`` (``rq``: keyword
    arguments of the spline as for ``rq_spline``).  With ``context`` [N, C <= 32] and ``context_pack`` from
    ``pack_made_inverse_context`` the conditional form (``fc_made_inverse_context``).  ``MADE_SOS`` (``rq``: ``n_sigmoids``,
    ``offset``, ``iterations``, ``lim``, ``log_scale_postact`` as for ``sum_of_sigmoids``) and ``MADE_SPLINE`` (``rq``: the
    keyword arguments of ``piecewise_spline``) run ``fc_made_inverse_sos`` / ``fc_made_inverse_spline``, which take no
    context.  Returns ``(outputs, logabsdet)``."""
    lib = _hip.load()
    z = _prep_2d(inputs)
    _hip.require_no_grad(inputs, context)
    n, d = z.shape
    if n % HIDDEN_ROWS != 0 or d > 64:
        raise ValueError("fc_made_inverse: rows must be a multiple of %d, D <= 64" % HIDDEN_ROWS)
    if (context is None) != (context_pack is None):
        raise ValueError("made_inverse: context and context_pack go together")
    rows = (z,) if context is None else (z, context)
    if context is not None:
        context_pack = _made_context_pack("made_inverse", "inputs'", z.device, n, d, context, context_pack, num_blocks, per_dim,
                                          per_dim, "parameters per dim")
    name, tail = _made_inverse_entry(kind, d, num_blocks, per_dim, rq, context is not None, int(logabsdet_accum is not None))
    lad, _ = _logabsdet_target(logabsdet_accum, n, z.device)
    if not _made_pack_matches(packed, d):
        raise ValueError("made_inverse: units_needed must hold one int32 per dim")
    y = torch.empty_like(z)
    _call(name, getattr(lib, name), z.device,
          *_made_arguments(rows, (y, lad, _err_word(z.device, True)), packed, context_pack or (), n, d, num_blocks, tail))
    _finish(True)
    return y, lad


def affine_tail_fits(in_features, num_blocks, d):
    """LDS budget of ``fc_affine_coupling_resnet``: the weight image (initial layer, 2 per block, the final Linear) + one
    [16, D | 1] float tile per wave next to it, 160 KB per CU; D <= 128, <= 3 blocks."""
    k0s = 1 if in_features <= 32 else 2
    layers = 2 + 2 * num_blocks
    image = (k0s * 8 + (2 * num_blocks + 1) * 16) * 1024 + layers * 64 * 4 + 64 + 32 * k0s * 4 + 512
    return d <= 128 and num_blocks <= 3 and image + 16 + 8 * 16 * (d | 1) * 4 <= 160 * 1024


def affine_tail_activation(code):
    """Scale activations ``fc_affine_coupling_resnet`` evaluates itself."""
    return code in (AFFINE_SIGMOID_PLUS2, AFFINE_SOFTPLUS_CLAMP3, AFFINE_ADDITIVE, AFFINE_MAF_SOFTPLUS)


def affine_coupling_resnet(inputs, id_cols, tr_cols, packed, in_features, num_blocks, activation, inverse=False,
                           logabsdet_accum=None):
    """One affine / additive coupling layer with a ResidualNet(hidden <= 64, <= 3 ReLU blocks) conditioner in ONE kernel
    (``fc_affine_coupling_resnet``); rows a multiple of 16.  Returns ``(outputs, logabsdet)``; with ``logabsdet_accum`` the
    layer's logabsdet is added onto that tensor, which is returned."""
    lib = _hip.load()
    x = _prep_2d(inputs, align16=True)        # the kernel moves whole 16-row chunks with 16-byte loads
    _hip.require_no_grad(inputs)
    n, d = x.shape
    if n % HIDDEN_ROWS != 0 or not affine_tail_activation(activation):
        raise ValueError("fc_affine_coupling_resnet: unsupported rows / activation")
    w_frag, w_un, bias_acc = packed
    ids, cols = _as_cols(id_cols, x.device), _as_cols(tr_cols, x.device)
    y = torch.empty_like(x)
    lad, accumulate = _logabsdet_target(logabsdet_accum, n, x.device)
    _call("fc_affine_coupling_resnet", lib.fc_affine_coupling_resnet, x.device, _hip.ptr(x), _hip.ptr(y), _hip.ptr(ids),
          _hip.ptr(cols), _hip.ptr(w_frag), _hip.ptr(w_un), _hip.ptr(bias_acc), _hip.ptr(lad), n, d, in_features,
          cols.numel(), 64, num_blocks, int(activation), 1 if inverse else 0, accumulate, _hip.stream_ptr(x.device))
    return y, lad


def resnet_hidden_packed(inputs, id_cols, packed, in_features, num_blocks, activation=(ACT_RELU, 0.0)):
    """``resnet_hidden`` (no context) from a ready-made weight image (``device_pack_resnet_hidden_forward``)."""
    lib = _hip.load()
    x = _prep_2d(inputs)
    _hip.require_no_grad(inputs)
    n, d = x.shape
    if n % HIDDEN_ROWS != 0:
        raise ValueError("fc_resnet_hidden needs a multiple of %d rows" % HIDDEN_ROWS)
    w_frag, w_un, bias_acc = packed
    k0s = 1 if in_features <= 32 else 2
    if w_frag.numel() != (k0s + 4 * num_blocks) * 4096 or w_un.numel() != 1 + 2 * num_blocks:
        raise ValueError("weight image does not match in_features = %d, num_blocks = %d" % (in_features, num_blocks))
    ids = _as_cols(id_cols, x.device)
    h = torch.empty(n, 64, dtype=torch.float32, device=x.device)
    # (timed and reported under the name of the kernel it launches: fc_resnet_hidden with a ready-made image)
    _call("fc_resnet_hidden", lib.fc_resnet_hidden_packed, x.device, _hip.ptr(x), _hip.ptr(h), _hip.ptr(ids),
          _hip.ptr(w_frag), _hip.ptr(w_un), _hip.ptr(bias_acc), n, d, in_features, 64, num_blocks, int(activation[0]),
          float(activation[1]), _hip.stream_ptr(x.device))
    return h


def resnet_hidden_backward(inputs, grad_hidden, id_cols, packed, in_features, num_blocks, grad_inputs_accum=None):
    """Backward of ``resnet_hidden`` (hidden 64, <= 2 ReLU blocks, no context; rows a multiple of 128): returns
    ``(grad_x_id [N, in_features], grad_w0 [64, in_features], grad_wb [2 blocks, 64, 64], grad_b [L, 64])`` with the
    activations recomputed from ``inputs``.  With ``grad_inputs_accum`` [N, D] the gradient wrt the identity columns is
    added into it in place (``fc_resnet_hidden_backward_accum``) and the first result is None."""
    lib = _hip.load()
    x = _prep_2d(inputs.detach())
    gh = _aligned16(_hip.dev_f32(grad_hidden, "grad_hidden"))
    n, d = x.shape
    if n % HIDDEN_BWD_ROWS != 0 or gh.shape != (n, 64) or not 0 <= num_blocks <= 2:
        raise ValueError("fc_resnet_hidden_backward: unsupported shapes")
    w_frag, wt_frag, w_un, bias_acc, k0s = packed
    ids = _as_cols(id_cols, x.device)
    layers = 1 + 2 * num_blocks
    if grad_inputs_accum is not None and (grad_inputs_accum.shape != x.shape or not grad_inputs_accum.is_contiguous()
                                          or grad_inputs_accum.dtype != torch.float32):
        raise ValueError("grad_inputs_accum must be a contiguous float32 [N, D] tensor")
    gxid = None if grad_inputs_accum is not None else torch.empty(n, 32 * k0s, dtype=torch.float32, device=x.device)
    nb2 = max(1, 2 * num_blocks)
    acc = torch.zeros(64 * 32 * k0s + nb2 * 4096 + layers * 64, dtype=torch.float32, device=x.device)   # one memset
    gw0 = acc[:64 * 32 * k0s].view(64, 32 * k0s)
    gwb = acc[64 * 32 * k0s:64 * 32 * k0s + nb2 * 4096].view(nb2, 64, 64)
    gb = acc[64 * 32 * k0s + nb2 * 4096:].view(layers, 64)
    fn = lib.fc_resnet_hidden_backward if gxid is not None else lib.fc_resnet_hidden_backward_accum
    _call("fc_resnet_hidden_backward", fn, x.device, _hip.ptr(x), _hip.ptr(gh), _hip.ptr(ids),
          _hip.ptr(w_frag), _hip.ptr(wt_frag), _hip.ptr(w_un), _hip.ptr(bias_acc),
          _hip.ptr(gxid if gxid is not None else grad_inputs_accum), _hip.ptr(gw0),
          _hip.ptr(gwb), _hip.ptr(gb), n, d, in_features, 64, num_blocks, ACT_RELU, _hip.stream_ptr(x.device))
    return (None if gxid is None else gxid[:, :in_features]), gw0[:, :in_features], gwb, gb


def resnet_hidden_wide(inputs, id_cols, packed, in_features, num_blocks, width, activation=(ACT_RELU, 0.0)):
    """Hidden layers of a wide conditioner on the rows of ``inputs`` (multiple of 64 rows) -> h [N, width]."""
    lib = _hip.load()
    x = _prep_2d(inputs)
    _hip.require_no_grad(inputs)
    n, d = x.shape
    if n % WIDE_ROWS != 0 or width not in (128, 256):
        raise ValueError("fc_resnet_hidden_wide needs a multiple of %d rows and a width of 128 or 256" % WIDE_ROWS)
    w_frag, w_un, bias = packed
    ids = _as_cols(id_cols, x.device)
    h = torch.empty(n, width, dtype=torch.float32, device=x.device)
    _call("fc_resnet_hidden_wide", lib.fc_resnet_hidden_wide, x.device, _hip.ptr(x), _hip.ptr(h), _hip.ptr(ids),
          _hip.ptr(w_frag), _hip.ptr(w_un), _hip.ptr(bias), n, d, in_features, width, num_blocks, int(activation[0]),
          float(activation[1]), _hip.stream_ptr(x.device))
    return h


def resnet_hidden(inputs, id_cols, packed, in_features, num_blocks, context=None, activation=(ACT_RELU, 0.0),
                  context_mode=CONTEXT_GLU):
    """Hidden layers of the conditioner on the rows of ``inputs`` (multiple of 16 rows) -> h [N, 64].
    ``activation``: ``activation_code`` of the blocks' activation.  ``context_mode``: ``CONTEXT_GLU`` (ResidualNet:
    concatenated into the initial layer, GLU gate per block) or ``CONTEXT_ADDITIVE`` (MADE: added after the initial
    layer through the activation and inside every block; ``packed`` then carries ``blocks + 1`` context layers).
    ``in_features`` = number of identity columns read from ``inputs``; ``context`` [N, C] (C <= 32,
    in_features + C <= 64) enters the initial layer after them and gates every block (``packed`` then carries
    the context layers)."""
    lib = _hip.load()
    x = _prep_2d(inputs)
    _hip.require_no_grad(inputs)
    n, d = x.shape
    if n % HIDDEN_ROWS != 0:
        raise ValueError("fc_resnet_hidden needs a multiple of %d rows" % HIDDEN_ROWS)
    w0, b0, wb, bb = packed[:4]
    ids = _as_cols(id_cols, x.device)
    h = torch.empty(n, 64, dtype=torch.float32, device=x.device)
    if context is None:
        _call("fc_resnet_hidden", lib.fc_resnet_hidden, x.device, _hip.ptr(x), _hip.ptr(h), _hip.ptr(ids),
              _hip.ptr(w0), _hip.ptr(b0), _hip.ptr(wb), _hip.ptr(bb), n, d, in_features, 64, num_blocks,
              int(activation[0]), float(activation[1]), _hip.stream_ptr(x.device))
        return h
    wc, bc = packed[4:6]
    c = _prep_2d(context)
    _hip.require_no_grad(context)
    if c.shape[0] != n or w0.shape[1] != in_features + (c.shape[1] if context_mode == CONTEXT_GLU else 0):
        raise ValueError("context rows / width do not match the inputs / the initial layer")
    _call("fc_resnet_hidden_context", lib.fc_resnet_hidden_context, x.device, _hip.ptr(x), _hip.ptr(c), _hip.ptr(h),
          _hip.ptr(ids), _hip.ptr(w0), _hip.ptr(b0), _hip.ptr(wb), _hip.ptr(bb), _hip.ptr(wc), _hip.ptr(bc), n, d,
          in_features, c.shape[1], 64, num_blocks, int(context_mode), int(activation[0]), float(activation[1]),
          _hip.stream_ptr(x.device))
    return h
