"""Invertible residual blocks over Lipschitz DenseNets: the eval-mode kernels and the training node around them."""
import torch

from flowconductor_amd import _hip
from ._core import _call, _prep_2d, once_differentiable


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


# ---- training: fc_iresnet_backward ---------------------------------------------------------------------------------------
IRES_DOUBLE_BACKWARD_MSG = (
    "flowconductor_amd: the iResBlock kernel route (options 'iresblock_training') is once differentiable; for a gradient "
    "of a gradient (create_graph=True) run the block with options.override(iresblock_training=False), the torch "
    "composition")


def iresnet_backward(inputs, image, d, e, depth, growth, activation, grad_outputs, grad_logabsdet, extra=None, scale=None,
                     _max_blocks=0):
    """The raw ``fc_iresnet_backward``: ``(grad_inputs [N, D], grad_image [image floats], grad_extra [N, E] or None,
    grad_scale [N] or None)`` of ``iresnet_forward`` at ``inputs`` for the cotangents of its two outputs.  The streams
    are recomputed in the kernel; the parameter gradient is summed without atomics (the same bits on every run).
    ``_max_blocks`` caps the grid below the kernel's own 256 blocks (tests: several partials at a small N)."""
    lib = _hip.load()
    x, image, extra, scale = _ires_operands(inputs, image, d, e, depth, growth, activation, extra, scale)
    n = x.shape[0]
    gy = _hip.dev_f32(grad_outputs, "grad_outputs")
    gl = _hip.dev_f32(grad_logabsdet, "grad_logabsdet")
    if tuple(gy.shape) != tuple(x.shape) or gl.numel() != n:
        raise ValueError("flowconductor_amd: iresnet_backward: cotangents of shapes %s / %s for %d rows of %d"
                         % (tuple(gy.shape), tuple(gl.shape), n, d))
    if gy.device != x.device or gl.device != x.device:
        raise RuntimeError("flowconductor_amd: cotangents on %s / %s, rows on %s" % (gy.device, gl.device, x.device))
    floats = lib.fc_iresnet_backward_workspace(n, d, e, depth, growth, activation, int(_max_blocks))
    if floats < 0:
        raise ValueError("flowconductor_amd: iresnet_backward: outside the kernel's limits")
    dx = torch.empty_like(x)
    dimage = torch.empty_like(image)
    dextra = None if extra is None else torch.empty_like(extra)
    dscale = None if scale is None else torch.empty(n, dtype=torch.float32, device=x.device)
    ws = torch.empty(max(floats, 1), dtype=torch.float64, device=x.device)
    _call("fc_iresnet_backward", lib.fc_iresnet_backward, x.device, _hip.ptr(x), _hip.ptr(extra), _hip.ptr(scale),
          _hip.ptr(image), _hip.ptr(gy), _hip.ptr(gl), _hip.ptr(dx), _hip.ptr(dextra), _hip.ptr(dscale),
          _hip.ptr(dimage), _hip.ptr(ws), n, d, e, depth, growth, activation, image.numel(), int(_max_blocks),
          _hip.stream_ptr(x.device))
    return dx, dimage, dextra, dscale


class _IResNetFunction(torch.autograd.Function):
    """``fc_iresnet_forward`` with ``fc_iresnet_backward``: saves the rows, the image and the per-row extras -- no
    activation and no Jacobian outlives the forward launch."""

    @staticmethod
    def forward(ctx, inputs, image, extra, scale, shape, max_blocks):
        y, logabsdet = iresnet_forward(inputs.detach(), image.detach(), *shape,
                                       extra=None if extra is None else extra.detach(),
                                       scale=None if scale is None else scale.detach())
        ctx.shape, ctx.max_blocks = shape, max_blocks
        ctx.scale_shape = None if scale is None else tuple(scale.shape)
        ctx.save_for_backward(inputs, image, extra, scale)
        return y, logabsdet

    @staticmethod
    @once_differentiable(IRES_DOUBLE_BACKWARD_MSG)
    def backward(ctx, grad_y, grad_logabsdet):
        x, image, extra, scale = ctx.saved_tensors
        dx, dimage, dextra, dscale = iresnet_backward(x, image, *ctx.shape, grad_y.contiguous(),
                                                      grad_logabsdet.contiguous(), extra=extra, scale=scale,
                                                      _max_blocks=ctx.max_blocks)
        need = ctx.needs_input_grad
        return (dx.view(x.shape) if need[0] else None, dimage if need[1] else None,
                dextra if need[2] and dextra is not None else None,
                dscale.view(ctx.scale_shape) if need[3] and dscale is not None else None, None, None)


def iresnet_autograd(inputs, image, d, e, depth, growth, activation, extra=None, scale=None, _max_blocks=0):
    """``iresnet_forward`` as one autograd node: gradients reach ``inputs``, ``image`` (every entry of the packed net),
    ``extra`` and ``scale`` through one ``fc_iresnet_backward`` launch.  Once differentiable."""
    return _IResNetFunction.apply(inputs, image, extra, scale, (d, e, depth, growth, activation), _max_blocks)
