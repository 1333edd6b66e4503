"""Invertible residual blocks over Lipschitz DenseNets (eval mode)."""
import torch

from flowconductor_amd import _hip
from ._core import _call, _prep_2d


IRES_MAX_DIM = 16
IRES_MAX_DEPTH = 4
IRES_MAX_WIDTH = 128
IRES_ACT_RELU, IRES_ACT_TANH, IRES_ACT_ELU, IRES_ACT_SWISH, IRES_ACT_LIPSWISH = 0, 1, 2, 3, 4
IRES_ACT_CLIPSWISH, IRES_ACT_SIN, IRES_ACT_CSIN, IRES_ACT_LEAKY_LSWISH = 5, 6, 7, 8
IRES_CONCAT_ACTS = (IRES_ACT_CLIPSWISH, IRES_ACT_CSIN)


def _pad4(v):
    return (v + 3) & ~3


def iresnet_supported(d, e, depth, growth, activation):
    """Whether ``fc_iresnet_forward`` / ``fc_iresnet_inverse`` take a net of this shape."""
    if not (1 <= d <= IRES_MAX_DIM and e >= 0 and 1 <= depth <= IRES_MAX_DEPTH and growth >= 1):
        return False
    if activation in IRES_CONCAT_ACTS and growth % 2 != 0:
        return False
    return d + e + depth * growth <= IRES_MAX_WIDTH


def iresnet_image_floats(d, e, depth, growth, activation):
    """Length of the packed net image (the layout is described in include/flowcon_hip.h)."""
    out_pad = _pad4(growth // 2 if activation in IRES_CONCAT_ACTS else growth)
    total, w_in = 4, d + e
    for _ in range(depth):
        total += 4 + out_pad + w_in * out_pad
        w_in += growth
    return total + _pad4(d) + w_in * _pad4(d)


def _ires_operands(rows, image, d, e, depth, growth, activation, extra, scale):
    x = _prep_2d(rows)
    n = x.shape[0]
    if x.shape[1] != d:
        raise ValueError("flowconductor_amd: rows of %d features for a net of dimension %d" % (x.shape[1], d))
    if not iresnet_supported(d, e, depth, growth, activation):
        raise ValueError("flowconductor_amd: the invertible-residual-block kernels take d <= %d, depth <= %d and a total "
                         "width <= %d" % (IRES_MAX_DIM, IRES_MAX_DEPTH, IRES_MAX_WIDTH))
    image = _hip.dev_f32(image, "image")
    if image.numel() != iresnet_image_floats(d, e, depth, growth, activation):
        raise ValueError("flowconductor_amd: net image of %d floats, expected %d"
                         % (image.numel(), iresnet_image_floats(d, e, depth, growth, activation)))
    if (e > 0) != (extra is not None):
        raise ValueError("flowconductor_amd: extra channels must be given exactly when e > 0")
    if extra is not None:
        extra = _hip.dev_f32(extra, "extra")
        if tuple(extra.shape) != (n, e):
            raise ValueError("flowconductor_amd: extra of shape %s, expected %s" % (tuple(extra.shape), (n, e)))
    if scale is not None:
        scale = _hip.dev_f32(scale, "scale")
        if scale.numel() != n:
            raise ValueError("flowconductor_amd: scale of %d entries for %d rows" % (scale.numel(), n))
    for t in (image, extra, scale):
        if t is not None and t.device != x.device:
            raise RuntimeError("flowconductor_amd: operand on %s, rows on %s" % (t.device, x.device))
    return x, image, extra, scale


def iresnet_forward(inputs, image, d, e, depth, growth, activation, extra=None, scale=None):
    """``y = x + scale g(x)`` and ``log|det(I + scale dg/dx)|`` of an eval-mode Lipschitz DenseNet ``g`` given as a packed
    image, one launch.  No autograd."""
    _hip.require_no_grad(inputs, extra, scale)
    lib = _hip.load()
    x, image, extra, scale = _ires_operands(inputs, image, d, e, depth, growth, activation, extra, scale)
    n = x.shape[0]
    y = torch.empty_like(x)
    logabsdet = torch.empty(n, dtype=torch.float32, device=x.device)
    _call("fc_iresnet_forward", lib.fc_iresnet_forward, x.device, _hip.ptr(x), _hip.ptr(extra), _hip.ptr(scale),
          _hip.ptr(image), _hip.ptr(y), _hip.ptr(logabsdet), n, d, e, depth, growth, activation, image.numel(),
          _hip.stream_ptr(x.device))
    return y, logabsdet


def iresnet_inverse(inputs, image, d, e, depth, growth, activation, extra=None, scale=None, max_iterations=1000,
                    atol=1e-5, rtol=1e-5, iterations_out=None):
    """``x`` with ``x + scale g(x) = y``: every row iterates ``x <- y - scale g(x)`` until ``|x - x_prev| <= atol +
    rtol |y|`` holds for all its elements (or ``max_iterations``), one launch, no host sync.  ``iterations_out``: an
    int32 device word that receives the largest iteration count of the launch."""
    _hip.require_no_grad(inputs, extra, scale)
    lib = _hip.load()
    y, image, extra, scale = _ires_operands(inputs, image, d, e, depth, growth, activation, extra, scale)
    if iterations_out is not None:
        if (iterations_out.dtype != torch.int32 or iterations_out.device != y.device or iterations_out.numel() != 1):
            raise ValueError("flowconductor_amd: iterations_out must be one int32 word on the device of the rows")
        iterations_out.zero_()
    x = torch.empty_like(y)
    _call("fc_iresnet_inverse", lib.fc_iresnet_inverse, y.device, _hip.ptr(y), _hip.ptr(extra), _hip.ptr(scale),
          _hip.ptr(image), _hip.ptr(x), _hip.ptr(iterations_out), y.shape[0], d, e, depth, growth, activation,
          image.numel(), int(max_iterations), float(atol), float(rtol), _hip.stream_ptr(y.device))
    return x
