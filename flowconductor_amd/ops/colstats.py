"""Batch statistics (``fc_colstats.hip``): reductions over the batch axis of [N, D] rows -- BatchNorm in training mode with
its backward, and the column sums behind the scale / shift gradients of ActNorm and PointwiseAffineTransform.

The kernels take contiguous float32 device rows with ``2 <= N`` and ``1 <= D <= MAX_ROW_FEATURES``
(``batch_statistics_supported``); callers keep the reference's torch expression for everything else.  Two stages, no
atomics: at most ``COLSTATS_MAX_PARTIALS`` workgroups reduce a slice of rows each, one workgroup merges their partial rows
in a fixed order, so a result's bits are a function of the shape alone.  Nothing here reads a device value on the host."""
import torch

from flowconductor_amd import _hip, options
from ._core import _call
from .rowwave import MAX_ROW_FEATURES

COLSTATS_MAX_PARTIALS = 512             # G: rows of the partial buffer (FC_COLSTATS_MAX_PARTIALS)
COLSTATS_ROWS_PER_ITERATION = 2048      # R: rows a stage-1 workgroup takes per loop iteration at D <= 4 (fewer when wider)


def batch_statistics_supported(x):
    """Whether the column kernels take ``x``: a float32 [N, D] tensor on a HIP device, 2 <= N, 1 <= D <= 512."""
    return (torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.shape[0] >= 2
            and 1 <= x.shape[1] <= MAX_ROW_FEATURES)


def batch_statistics_route(x):
    """``batch_statistics_supported`` and the ``batch_statistics_kernels`` option."""
    return options.get("batch_statistics_kernels") and batch_statistics_supported(x)


def _workspace(d, device):
    return torch.empty(COLSTATS_MAX_PARTIALS * (2 * d + 1), dtype=torch.float32, device=device)


def _rows(t, name):
    t = _hip.dev_f32(t, name)
    if not batch_statistics_supported(t):
        raise ValueError("%s must be [N, D] with 2 <= N and 1 <= D <= %d, got shape %s"
                         % (name, MAX_ROW_FEATURES, tuple(t.shape)))
    return t


def _vector(t, d, device, name):
    t = _hip.dev_f32(t.detach(), name)
    if t.shape != (d,) or t.device != device:
        raise ValueError("%s must hold one value per feature (%d) on %s, got shape %s on %s"
                         % (name, d, device, tuple(t.shape), t.device))
    return t


def column_sums(g, v, mean=None, invstd=None):
    """``(s1, s2)`` [D] each: ``s1 = g.sum(0)`` and ``s2 = (g * vh).sum(0)`` in one pass over ``g`` and ``v`` [N, D], with
    ``vh = (v - mean) * invstd`` when the two [D] vectors are given and ``vh = v`` otherwise."""
    return _column_sums(g, v, mean, invstd, None)[:2]


def _column_sums(g, v, mean, invstd, gl):
    lib = _hip.load()
    g, v = _rows(g, "g"), _rows(v, "v")
    _hip.require_no_grad(g, v)
    if g.shape != v.shape or g.device != v.device:
        raise ValueError("column_sums: g %s and v %s must have one shape and one device" % (tuple(g.shape), tuple(v.shape)))
    if (mean is None) != (invstd is None):
        raise ValueError("column_sums: mean and invstd come together")
    n, d = g.shape
    if mean is not None:
        mean, invstd = _vector(mean, d, g.device, "mean"), _vector(invstd, d, g.device, "invstd")
    if gl is not None:
        gl = _hip.dev_f32(gl, "gl")
        if gl.shape != (n,):
            raise ValueError("column_sums: gl must have one entry per row")
    d4 = (d + 3) // 4 * 4
    out = torch.empty(2 * d4 + 1, dtype=torch.float32, device=g.device)     # s1 | s2 | sum gl, each 16-byte aligned
    s1, s2, gl_sum = out[:d], out[d4:d4 + d], out[2 * d4:]
    _call("fc_column_sums", lib.fc_column_sums, g.device, _hip.ptr(g), _hip.ptr(v), _hip.ptr(mean), _hip.ptr(invstd),
          _hip.ptr(gl), _hip.ptr(s1), _hip.ptr(s2), _hip.ptr(gl_sum), _hip.ptr(_workspace(d, g.device)), n, d,
          _hip.stream_ptr(g.device))
    return s1, s2, (gl_sum if gl is not None else None)


def batchnorm_train(x, weight, bias, eps, running_mean=None, running_var=None, momentum=None):
    """Training-mode BatchNorm of ``x`` [N, D] (reference normalization.py:98-141) in one entry: returns
    ``(y, mean, var, invstd, half_log_sum)`` with the batch mean and unbiased variance [D], ``invstd = 1 / sqrt(var + eps)``,
    ``y = weight * ((x - mean) * invstd) + bias`` and ``half_log_sum = sum(-0.5 * log(var + eps))`` (a 0-dim tensor).  The
    running buffers, when given, move by ``momentum`` towards the batch statistics in place (``lerp_``), written by the
    kernel: their version counters stay where they are."""
    lib = _hip.load()
    x = _rows(x, "inputs")
    _hip.require_no_grad(x, weight, bias)
    n, d = x.shape
    weight, bias = _vector(weight, d, x.device, "weight"), _vector(bias, d, x.device, "bias")
    if (running_mean is None) != (running_var is None):
        raise ValueError("batchnorm_train: running_mean and running_var come together")
    if running_mean is not None:
        if momentum is None:
            raise ValueError("batchnorm_train: running statistics need a momentum")
        for name, r in (("running_mean", running_mean), ("running_var", running_var)):
            if not r.is_contiguous():
                raise ValueError("batchnorm_train: %s must be contiguous (it is updated in place)" % name)
            _vector(r, d, x.device, name)
    y = torch.empty_like(x)
    d4 = (d + 3) // 4 * 4
    stats = torch.empty(3 * d4 + 1, dtype=torch.float32, device=x.device)   # mean | var | invstd | half_log_sum
    mean, var, invstd, half_log_sum = stats[:d], stats[d4:d4 + d], stats[2 * d4:2 * d4 + d], stats[3 * d4:]
    _call("fc_batchnorm_train", lib.fc_batchnorm_train, x.device, _hip.ptr(x), _hip.ptr(weight), _hip.ptr(bias), _hip.ptr(y),
          _hip.ptr(mean), _hip.ptr(var), _hip.ptr(invstd), _hip.ptr(half_log_sum), _hip.ptr(running_mean),
          _hip.ptr(running_var), _hip.ptr(_workspace(d, x.device)), n, d, float(eps),
          float(momentum) if running_mean is not None else 0.0, _hip.stream_ptr(x.device))
    return y, mean, var, invstd, half_log_sum.reshape(())


def _batchnorm_reference(x, weight, bias, eps):
    """The reference's expression (normalization.py:98-141) in torch ops: ``(y, logabsdet)``."""
    var, mean = torch.var_mean(x, dim=0)
    y = weight * ((x - mean) / torch.sqrt(var + eps)) + bias
    return y, torch.sum(torch.log(weight) - 0.5 * torch.log(var + eps)) * x.new_ones(x.shape[0])


class _BatchNormTrainFunction(torch.autograd.Function):
    """``fc_batchnorm_train`` with ``fc_batchnorm_train_backward`` as its gradient over ``(x, weight, bias)``; the outputs
    are ``(y, logabsdet)``.  Saved: ``x``, ``weight`` and the [D] vectors ``mean`` / ``invstd`` -- no [N, D] tensor beside
    ``x``.  With ``s1, s2 = column_sums(gy, x, mean, invstd)``, ``GL = sum(g_logabsdet)`` and ``xh = (x - mean) invstd``:

        gx = w invstd (gy - s1 / N - xh s2 / (N - 1)) - GL invstd xh / (N - 1),    g_w = s2 + GL / w,    g_b = s1

    (the GL terms: logabsdet depends on ``x`` through the variance, and on ``w``).  Under ``create_graph`` the backward
    differentiates the reference's expression in torch ops instead, so that a second derivative exists."""

    @staticmethod
    def forward(ctx, x, weight, bias, eps, running_mean, running_var, momentum):
        y, mean, _, invstd, half_log_sum = batchnorm_train(x, weight, bias, eps, running_mean, running_var, momentum)
        logabsdet = (torch.log(weight).sum() + half_log_sum) * x.new_ones(x.shape[0])
        ctx.save_for_backward(x, weight, mean, invstd)
        ctx.eps = eps
        return y, logabsdet

    @staticmethod
    def backward(ctx, gy, gl):
        x, weight, mean, invstd = ctx.saved_tensors
        want = ctx.needs_input_grad[:3]
        if torch.is_grad_enabled():
            with torch.enable_grad():
                # (the gradient of the bias does not depend on its value: a fresh zero stands in for it)
                operands = (x, weight, torch.zeros_like(weight, requires_grad=True))
                outputs = _batchnorm_reference(*operands, ctx.eps)
                grads = iter(torch.autograd.grad(outputs, [t for t, w in zip(operands, want) if w], (gy, gl),
                                                 create_graph=True, allow_unused=True))
            return tuple(next(grads) if w else None for w in want) + (None,) * 4
        lib = _hip.load()
        n, d = x.shape
        gy = _hip.dev_f32(gy, "grad_outputs")
        gl = _hip.dev_f32(gl, "grad_logabsdet")          # (the gradient of a plain .sum() arrives as an expanded scalar)
        xc = _hip.dev_f32(x, "inputs")
        w = _hip.dev_f32(weight.detach(), "weight")
        gx = torch.empty_like(xc) if want[0] else None
        d4 = (d + 3) // 4 * 4
        sums = torch.empty(2 * d4 + 1, dtype=torch.float32, device=x.device)
        s1, s2, gl_sum = sums[:d], sums[d4:d4 + d], sums[2 * d4:]
        _call("fc_batchnorm_train_backward", lib.fc_batchnorm_train_backward, x.device, _hip.ptr(xc), _hip.ptr(gy),
              _hip.ptr(gl), _hip.ptr(mean), _hip.ptr(invstd), _hip.ptr(w), _hip.ptr(gx), _hip.ptr(s1), _hip.ptr(s2),
              _hip.ptr(gl_sum), _hip.ptr(_workspace(d, x.device)), n, d, _hip.stream_ptr(x.device))
        return gx, (s2 + gl_sum / w if want[1] else None), (s1 if want[2] else None), None, None, None, None


def batchnorm_train_autograd(x, weight, bias, eps, running_mean=None, running_var=None, momentum=None):
    """``(y, logabsdet)`` of a training-mode BatchNorm with an autograd node over ``(x, weight, bias)``: the kernels
    forward and backward (``_BatchNormTrainFunction``)."""
    return _BatchNormTrainFunction.apply(x, weight, bias, eps, running_mean, running_var, momentum)
