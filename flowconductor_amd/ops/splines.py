"""Linear / quadratic / cubic splines."""
import torch

from flowconductor_amd import _hip
from ._core import LAD_STORE, _as_cols, _call, _err_word, _finish, _prep_2d
from .rq import DEFAULT_MIN_BIN_HEIGHT, DEFAULT_MIN_BIN_WIDTH, _inverse_through_forward


SPLINE_LINEAR, SPLINE_QUADRATIC, SPLINE_CUBIC = 0, 1, 2


def spline_multiplier(kind, num_bins, tails):
    if kind == SPLINE_LINEAR:
        return num_bins
    if kind == SPLINE_QUADRATIC:
        return num_bins * 2 - 1 if tails == "linear" else num_bins * 2 + 1
    return num_bins * 2 + 2


def _spline_config(kind, num_bins, tails, tail_bound, box, min_bin_width, min_bin_height, width_divisor,
                   height_divisor, inverse):
    cfg = _hip.SplineConfig()
    cfg.kind, cfg.num_bins = kind, num_bins
    cfg.tails = 0 if tails is None else 1
    cfg.inverse = 1 if inverse else 0
    if tails == "linear":
        cfg.left, cfg.right, cfg.bottom, cfg.top = -tail_bound, tail_bound, -tail_bound, tail_bound
    else:
        cfg.left, cfg.right, cfg.bottom, cfg.top = box
    cfg.min_bin_width, cfg.min_bin_height = min_bin_width, min_bin_height
    cfg.width_divisor, cfg.height_divisor = width_divisor, height_divisor
    cfg.cubic_eps, cfg.cubic_quadratic_threshold = 1e-5, 1e-3
    return cfg


class _PiecewiseSplineFunction(torch.autograd.Function):
    """``piecewise_spline`` (forward direction, per-sample rows) with its HIP backward kernel
    (``fc_piecewise_spline_backward``: forward-mode derivative of the kernel's own evaluation, one thread per
    (element, parameter))."""

    @staticmethod
    def forward(ctx, inputs, params, cols, kw):
        with torch.no_grad():
            outputs, logabsdet = piecewise_spline(inputs, params, cols, **kw)
        ctx.save_for_backward(inputs, params)
        ctx.cols, ctx.kw = cols, kw
        return outputs, logabsdet

    @staticmethod
    def backward(ctx, grad_outputs, grad_logabsdet):
        inputs, params = ctx.saved_tensors
        kw = dict(ctx.kw)
        lib = _hip.load()
        x = _prep_2d(inputs.detach())
        p = _hip.dev_f32(params.detach(), "params")
        n, d = x.shape
        cols = _as_cols(ctx.cols, x.device)
        d_t = d if cols is None else cols.numel()
        gy = _hip.dev_f32(grad_outputs if grad_outputs is not None else torch.zeros_like(x), "grad_outputs")
        gl = None if grad_logabsdet is None else _hip.dev_f32(grad_logabsdet, "grad_logabsdet")
        cfg = _spline_config(kw["kind"], kw["num_bins"], kw.get("tails"), kw.get("tail_bound", 1.0),
                             (kw.get("left", 0.0), kw.get("right", 1.0), kw.get("bottom", 0.0), kw.get("top", 1.0)),
                             kw.get("min_bin_width", DEFAULT_MIN_BIN_WIDTH), kw.get("min_bin_height", DEFAULT_MIN_BIN_HEIGHT),
                             kw.get("width_divisor", 1.0), kw.get("height_divisor", 1.0), False)
        gx = gy.clone() if d_t < d else torch.empty_like(x)       # identity columns pass the gradient through
        gp = torch.empty_like(p)
        _call("fc_piecewise_spline_backward", lib.fc_piecewise_spline_backward, x.device, _hip.ptr(x), _hip.ptr(p),
              _hip.ptr(cols), _hip.ptr(gy), _hip.ptr(gl), _hip.ptr(gx), _hip.ptr(gp), n, d, d_t, cfg,
              _hip.stream_ptr(x.device))
        return gx, gp.view_as(params), None, None


def piecewise_spline_backward_supported(kind, num_bins, tails):
    """``fc_piecewise_spline_backward`` keeps an element's parameters as dual numbers in LDS: <= 32 per element."""
    return spline_multiplier(kind, num_bins, tails) <= 32


def piecewise_spline_autograd(inputs, params, cols=None, *, inverse=False, shared_params=False, **kw):
    """``piecewise_spline``; under autograd (per-sample parameters) the kernel's forward sits behind a node whose
    gradients come from the same spline in torch ops, the inverse goes through ``_inverse_through_forward``."""
    if not (torch.is_grad_enabled() and (inputs.requires_grad or params.requires_grad)) or shared_params:
        return piecewise_spline(inputs, params, cols, inverse=inverse, shared_params=shared_params, **kw)
    x = _prep_2d(inputs)
    if not piecewise_spline_backward_supported(kw["kind"], kw["num_bins"], kw.get("tails")):
        raise NotImplementedError("autograd through piecewise splines needs <= 32 parameters per element "
                                  "(fc_piecewise_spline_backward); got num_bins = %d" % kw["num_bins"])

    def forward_fn(v, p):
        return _PiecewiseSplineFunction.apply(v, p, cols, kw)

    if not inverse:
        return forward_fn(x, params)
    return _inverse_through_forward(forward_fn, lambda a, b: piecewise_spline(a, b, cols, inverse=True, **kw), x, params)


def piecewise_spline(inputs, params, cols=None, *, kind, num_bins, tails=None, tail_bound=1.0,
                     left=0.0, right=1.0, bottom=0.0, top=1.0, min_bin_width=DEFAULT_MIN_BIN_WIDTH,
                     min_bin_height=DEFAULT_MIN_BIN_HEIGHT, width_divisor=1.0, height_divisor=1.0,
                     inverse=False, shared_params=False):
    """Linear / quadratic / cubic spline over ``inputs[:, cols]`` (reference splines/{linear,
    quadratic,cubic}.py).  Row layouts: ``FC_SPLINE_*`` in include/flowcon_hip.h."""
    lib = _hip.load()
    x = _prep_2d(inputs)
    p = _hip.dev_f32(params, "params")
    _hip.require_no_grad(inputs, params)
    n, d = x.shape
    cols = _as_cols(cols, x.device)
    d_t = d if cols is None else cols.numel()
    if tails not in (None, "linear"):
        raise RuntimeError("{} tails are not implemented.".format(tails))
    if kind != SPLINE_LINEAR:
        if min_bin_width * num_bins > 1.0:
            raise ValueError("Minimal bin width too large for the number of bins")
        if min_bin_height * num_bins > 1.0:
            raise ValueError("Minimal bin height too large for the number of bins")
    rowlen = d_t * spline_multiplier(kind, num_bins, tails)
    want = rowlen if shared_params else n * rowlen
    if p.numel() != want:
        raise ValueError("params has %d elements, expected %d" % (p.numel(), want))
    cfg = _spline_config(kind, num_bins, tails, tail_bound, (left, right, bottom, top), min_bin_width, min_bin_height,
                         width_divisor, height_divisor, inverse)
    y = torch.empty_like(x)
    lad = torch.empty(n, dtype=torch.float32, device=x.device)
    err = _err_word(x.device, True)
    _call("fc_piecewise_spline", lib.fc_piecewise_spline, x.device, _hip.ptr(x), _hip.ptr(y), _hip.ptr(p),
          _hip.ptr(cols), _hip.ptr(lad), _hip.ptr(err), n, d, d_t, 1 if shared_params else 0, LAD_STORE, cfg,
          _hip.stream_ptr(x.device))
    _finish(True)
    return y, lad
