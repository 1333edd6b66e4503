"""Row-norm bijectors: the radial flow and the stereographic unit-vector map (``fc_rownorm.hip`` and its backward)."""
import torch

from flowconductor_amd import _hip
from ._core import _call, _err_word, _finish, _prep_2d
from .rowwave import MAX_ROW_FEATURES, _param, _rows


def _radial_operands(x, z_0, a, b):
    d = x.shape[1]
    zv = _param(z_0, x.device, "z_0").reshape(-1)
    av = _param(a, x.device, "a").reshape(-1)
    bv = _param(b, x.device, "b").reshape(-1)
    if zv.numel() != d or av.numel() != 1 or bv.numel() != 1:
        raise ValueError("radial parameters do not match %d features" % d)
    return zv, av, bv


def radial(inputs, z_0, a, b, inverse=False):
    """Radial flow (reference no_analytic_inv/planar.py:199-211) with ``a = |alpha|`` and
    ``b = softplus(beta) - |alpha|`` given as one-element tensors: ``y = x + b / (a + r) (x - z_0)``, ``r = |x - z_0|``,
    and its logabsdet; ``inverse=True`` is the closed-form inverse (the reference has none)."""
    lib = _hip.load()
    x = _rows(inputs)
    _hip.require_no_grad(inputs)
    n, d = x.shape
    zv, av, bv = _radial_operands(x, z_0, a, b)
    y = torch.empty_like(x)
    lad = torch.empty(n, dtype=torch.float32, device=x.device)
    _call("fc_radial", lib.fc_radial, x.device, _hip.ptr(x), _hip.ptr(y), _hip.ptr(lad), _hip.ptr(zv), _hip.ptr(av),
          _hip.ptr(bv), n, d, 1 if inverse else 0, _hip.stream_ptr(x.device))
    return y, lad


class _RadialFunction(torch.autograd.Function):
    """Forward direction of ``radial`` with its HIP backward kernel (``fc_radial_backward``)."""

    @staticmethod
    def forward(ctx, inputs, z_0, a, b):
        with torch.no_grad():
            outputs, logabsdet = radial(inputs, z_0, a, b)
        ctx.save_for_backward(inputs, z_0, a, b)
        return outputs, logabsdet

    @staticmethod
    def backward(ctx, grad_outputs, grad_logabsdet):
        inputs, z_0, a, b = ctx.saved_tensors
        lib = _hip.load()
        x = _hip.dev_f32(inputs.detach(), "inputs")
        n, d = x.shape
        zv = _hip.dev_f32(z_0.detach().reshape(-1), "z_0")
        av = _hip.dev_f32(a.detach().reshape(-1), "a")
        bv = _hip.dev_f32(b.detach().reshape(-1), "b")
        gy = _hip.dev_f32(grad_outputs if grad_outputs is not None else torch.zeros_like(x), "grad_outputs")
        gl = None if grad_logabsdet is None else _hip.dev_f32(grad_logabsdet, "grad_logabsdet")
        gx = torch.empty_like(x)
        gpar = torch.zeros(d + 2, dtype=torch.float32, device=x.device)      # gz0 | ga | gb, one zero fill
        _call("fc_radial_backward", lib.fc_radial_backward, x.device, _hip.ptr(x), _hip.ptr(gy), _hip.ptr(gl), _hip.ptr(zv),
              _hip.ptr(av), _hip.ptr(bv), _hip.ptr(gx), _hip.ptr(gpar[:d]), _hip.ptr(gpar[d:d + 1]), _hip.ptr(gpar[d + 1:]),
              n, d, _hip.stream_ptr(x.device))
        return gx, gpar[:d].view_as(z_0), gpar[d:d + 1].view_as(a), gpar[d + 1:].view_as(b)


def _radial_inverse_through_forward(inputs, z_0, a, b):
    """Differentiable inverse of the radial flow, whose gradients exist for the forward direction only: the inverse kernel
    finds ``x0 = f^-1(y)`` without a graph, then one Newton-shaped step ``x = x0 - J(x0)^-1 (f(x0; p) - y)`` through the
    differentiable forward carries the implicit-function gradients (its value only removes the inverse's rounding
    residual).  The Jacobian ``J = (1 + h) I + (k / r^2) dz dz^T`` is inverted in closed form (Sherman-Morrison);
    ``logabsdet = -logabsdet_f(x; p)`` is the forward evaluated at that ``x``."""
    with torch.no_grad():
        x0, _ = radial(inputs, z_0, a, b, inverse=True)
        dz = x0 - z_0.reshape(1, -1)
        r = torch.linalg.vector_norm(dz, dim=1, keepdim=True)
        ar = a.reshape(1, 1) + r
        h = b.reshape(1, 1) / ar
        k = -b.reshape(1, 1) * r / ar ** 2
        along = torch.where(r > 0, k / (r * r), torch.zeros_like(r)) / ((1 + h) * (1 + h + k))
    with torch.enable_grad():
        x_hat, _ = _RadialFunction.apply(x0, z_0, a, b)
        residual = x_hat - inputs
        x = x0 - (residual / (1 + h) - along * (dz * residual).sum(1, keepdim=True) * dz)
        _, logabsdet = _RadialFunction.apply(x, z_0, a, b)
    return x, -logabsdet


def radial_autograd(inputs, z_0, a, b, inverse=False):
    """``radial`` with an autograd node when needed (the inverse through ``_radial_inverse_through_forward``)."""
    if torch.is_grad_enabled() and any(t.requires_grad for t in (inputs, z_0, a, b)):
        x = _rows(inputs)
        if inverse:
            return _radial_inverse_through_forward(x, z_0, a, b)
        return _RadialFunction.apply(x, z_0, a, b)
    return radial(inputs, z_0, a, b, inverse=inverse)


def _unit_rows(inputs, features, inverse):
    """``inputs`` as [N, d] (forward) or [N, d + 1] (inverse) rows for ``features`` = d; the wider side is the limit."""
    if features + 1 > MAX_ROW_FEATURES:
        raise ValueError("flowconductor_amd: %d + 1 features exceed the %d supported by the row kernels"
                         % (features, MAX_ROW_FEATURES))
    x = _prep_2d(inputs)
    if x.shape[1] != features + (1 if inverse else 0):
        raise ValueError("unit_vector: inputs of shape %s do not match %d features" % (tuple(x.shape), features))
    return x


def unit_vector(inputs, features, inverse=False):
    """Stereographic map R^d -> S^d (reference unitvector.py:18-53) and its inverse, with logabsdet.  The inverse checks
    EVERY row for ``| |y|^2 - 1 | <= 1e-4`` and raises ``InputOutsideDomain`` (the reference tests the batch maximum)."""
    lib = _hip.load()
    x = _unit_rows(inputs, features, inverse)
    _hip.require_no_grad(inputs)
    n = x.shape[0]
    y = torch.empty(n, features + (0 if inverse else 1), dtype=torch.float32, device=x.device)
    lad = torch.empty(n, dtype=torch.float32, device=x.device)
    err = _err_word(x.device, inverse)
    _call("fc_unit_vector", lib.fc_unit_vector, x.device, _hip.ptr(x), _hip.ptr(y), _hip.ptr(lad), _hip.ptr(err), n,
          features, 1 if inverse else 0, _hip.stream_ptr(x.device))
    _finish(inverse)
    return y, lad


class _UnitVectorFunction(torch.autograd.Function):
    """``unit_vector`` in either direction with its HIP backward kernel (``fc_unit_vector_backward``)."""

    @staticmethod
    def forward(ctx, inputs, features, inverse):
        with torch.no_grad():
            outputs, logabsdet = unit_vector(inputs, features, inverse)
        ctx.save_for_backward(inputs)
        ctx.features, ctx.inverse = features, inverse
        return outputs, logabsdet

    @staticmethod
    def backward(ctx, grad_outputs, grad_logabsdet):
        inputs, = ctx.saved_tensors
        lib = _hip.load()
        x = _hip.dev_f32(inputs.detach(), "inputs")
        n, d = x.shape[0], ctx.features
        if grad_outputs is None:
            grad_outputs = x.new_zeros(n, d + (0 if ctx.inverse else 1))
        gy = _hip.dev_f32(grad_outputs, "grad_outputs")
        gl = None if grad_logabsdet is None else _hip.dev_f32(grad_logabsdet, "grad_logabsdet")
        gx = torch.empty_like(x)
        _call("fc_unit_vector_backward", lib.fc_unit_vector_backward, x.device, _hip.ptr(x), _hip.ptr(gy), _hip.ptr(gl),
              _hip.ptr(gx), n, d, 1 if ctx.inverse else 0, _hip.stream_ptr(x.device))
        return gx, None, None


def unit_vector_autograd(inputs, features, inverse=False):
    """``unit_vector`` with an autograd node when the inputs require gradients."""
    if torch.is_grad_enabled() and inputs.requires_grad:
        return _UnitVectorFunction.apply(_unit_rows(inputs, features, inverse), int(features), bool(inverse))
    return unit_vector(inputs, features, inverse=inverse)
