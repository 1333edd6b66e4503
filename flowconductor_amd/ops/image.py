"""Flows on images (transforms/reshape.py, transforms/conv.py)."""
import torch

from flowconductor_amd import _hip
from ._core import _call


CONV1X1_MAX_CHANNELS = 128   # FC_CONV1X1_MAX_CHANNELS: wider channel counts take the torch composition (conv.py)


def _squeeze_nograd(x, factor, mode):
    """mode 0: [B, C, H, W] -> [B, C f^2, H/f, W/f]; mode 1: the inverse.  ``x`` is contiguous float32 on the device."""
    lib = _hip.load()
    b, c, h, w = x.shape
    if mode == 0:
        planes, ph, pw = b * c, h, w
        y = torch.empty(b, c * factor * factor, h // factor, w // factor, dtype=torch.float32, device=x.device)
    else:
        planes, ph, pw = b * (c // (factor * factor)), h * factor, w * factor
        y = torch.empty(b, c // (factor * factor), ph, pw, dtype=torch.float32, device=x.device)
    _call("fc_squeeze", lib.fc_squeeze, x.device, _hip.ptr(x), _hip.ptr(y), planes, ph, pw, factor, mode,
          _hip.stream_ptr(x.device))
    return y


class _SqueezeFunction(torch.autograd.Function):
    """Squeeze (mode 0) or its inverse (mode 1); the backward is the other mode of the same kernel."""

    @staticmethod
    def forward(ctx, x, factor, mode):
        ctx.factor, ctx.mode = factor, mode
        return _squeeze_nograd(x, factor, mode)

    @staticmethod
    def backward(ctx, grad):
        return _squeeze_nograd(_hip.dev_f32(grad, "grad"), ctx.factor, 1 - ctx.mode), None, None


def squeeze(inputs, factor, inverse=False):
    """``SqueezeTransform`` (reshape.py:28-66) without its checks: forward ``[B, C, H, W] -> [B, C f^2, H/f, W/f]``,
    inverse ``[B, C, h, w] -> [B, C / f^2, h f, w f]`` (C divisible by f^2).  Bit-exact; records an autograd node when
    gradients are required."""
    x = _hip.dev_f32(inputs, "inputs")
    if x.dim() != 4:
        raise ValueError("flowconductor_amd: squeeze expects [B, C, H, W], got %s" % (tuple(x.shape),))
    mode = 1 if inverse else 0
    if torch.is_grad_enabled() and inputs.requires_grad:
        return _SqueezeFunction.apply(x, factor, mode)
    return _squeeze_nograd(x, factor, mode)


def _conv1x1_operand(t, device, name):
    """A weight / bias operand of ``conv1x1``: float32 required (a float64 module is refused, not reinterpreted), moved to
    the device of the inputs (differentiably, as ``Tensor.to`` is) and made contiguous."""
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s must be a tensor" % name)
    if t.dtype != torch.float32:
        raise TypeError("flowconductor_amd: %s must be float32, got %s" % (name, t.dtype))
    return t.to(device).contiguous()


def _conv1x1_nograd(x, weight, pre, post):
    lib = _hip.load()
    for t in (x, weight, pre, post):     # the launch reads raw device pointers: nothing else may reach it
        if t is not None and (t.device != x.device or t.dtype != torch.float32 or not t.is_contiguous()):
            raise RuntimeError("flowconductor_amd: conv1x1 operand on %s / %s / contiguous=%s, inputs on %s"
                               % (t.device, t.dtype, t.is_contiguous(), x.device))
    b, c = x.shape[0], x.shape[1]
    hw = x.shape[2] * x.shape[3]
    y = torch.empty_like(x)
    _call("fc_conv1x1", lib.fc_conv1x1, x.device, _hip.ptr(x), _hip.ptr(weight), _hip.ptr(pre), _hip.ptr(post),
          _hip.ptr(y), b, c, hw, _hip.stream_ptr(x.device))
    return y


class _Conv1x1Function(torch.autograd.Function):
    """``y = M (x - pre) + post`` at every pixel of an NCHW tensor.  Backward: ``gx = M^T gy`` by the same kernel,
    ``gM = sum_pixels gy (x - pre)^T`` and the two bias sums by torch contractions."""

    @staticmethod
    def forward(ctx, x, weight, pre, post):
        w = weight.detach().contiguous()
        p = pre.detach().contiguous() if pre is not None else None
        q = post.detach().contiguous() if post is not None else None
        y = _conv1x1_nograd(x, w, p, q)
        ctx.save_for_backward(x, w, p)
        ctx.has_pre, ctx.has_post = pre is not None, post is not None
        return y

    @staticmethod
    def backward(ctx, gy):
        x, w, p = ctx.saved_tensors
        gy = _hip.dev_f32(gy, "grad")
        b, c = x.shape[0], x.shape[1]
        gx = gw = gpre = gpost = None
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[2]:
            gx = _conv1x1_nograd(gy, w.t().contiguous(), None, None)
        if ctx.needs_input_grad[1]:
            xs = x if p is None else x - p.view(1, c, 1, 1)
            gw = torch.einsum("bip,bkp->ik", gy.reshape(b, c, -1), xs.reshape(b, c, -1))
        if ctx.has_pre and ctx.needs_input_grad[2]:
            gpre = -gx.sum(dim=(0, 2, 3))
        if ctx.has_post and ctx.needs_input_grad[3]:
            gpost = gy.sum(dim=(0, 2, 3))
        return (gx if ctx.needs_input_grad[0] else None), gw, gpre, gpost


def conv1x1(inputs, weight, pre=None, post=None):
    """``y[b, :, p] = weight (x[b, :, p] - pre) + post`` for ``[B, C, H, W]`` inputs, C <= CONV1X1_MAX_CHANNELS, in one
    pass over the tensor; records an autograd node when gradients are required."""
    x = _hip.dev_f32(inputs, "inputs")
    if x.dim() != 4:
        raise ValueError("flowconductor_amd: conv1x1 expects [B, C, H, W], got %s" % (tuple(x.shape),))
    c = x.shape[1]
    if c > CONV1X1_MAX_CHANNELS:
        raise ValueError("flowconductor_amd: conv1x1 takes C <= %d" % CONV1X1_MAX_CHANNELS)
    if weight.shape != (c, c):
        raise ValueError("flowconductor_amd: weight of shape %s for %d channels" % (tuple(weight.shape), c))
    for v in (pre, post):
        if v is not None and v.numel() != c:
            raise ValueError("flowconductor_amd: bias of %d entries for %d channels" % (v.numel(), c))
    weight = _conv1x1_operand(weight, x.device, "weight")
    pre = None if pre is None else _conv1x1_operand(pre, x.device, "pre")
    post = None if post is None else _conv1x1_operand(post, x.device, "post")
    tensors = [t for t in (inputs, weight, pre, post) if t is not None]
    if torch.is_grad_enabled() and any(t.requires_grad for t in tensors):
        return _Conv1x1Function.apply(x, weight, pre, post)
    return _conv1x1_nograd(x, weight, pre, post)
