"""Discrete and uniform base densities (``fc_bernoulli.hip``): the independent-Bernoulli likelihood with its backward, its
sampler and the box-uniform density.

The kernels take contiguous float32 device tensors, flattened to [N, D]; every other call (CPU tensors, other dtypes,
strided views, a double backward) takes the reference's torch expression, which autograd differentiates as usual."""
import torch
from torch.nn import functional as F

from flowconductor_amd import _hip
from ._core import _call


def _fast(*tensors):
    """Whether every tensor is one the kernels read in place: float32, contiguous, all on one HIP device."""
    first = tensors[0]
    return all(torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()
               and t.device == first.device for t in tensors)


def _rows2d(t):
    return t.reshape(t.shape[0], -1)


# ---- Bernoulli likelihood --------------------------------------------------------------------------------------------
def _bernoulli_log_prob_torch(inputs, logits, add):
    """distributions/discrete.py:54-55 of the reference."""
    log_prob = -inputs * F.softplus(-logits) - (1.0 - inputs) * F.softplus(logits)
    log_prob = log_prob.reshape(log_prob.shape[0], -1).sum(dim=1)
    return log_prob if add is None else log_prob + add


def _bernoulli_log_prob_nograd(inputs, logits, add):
    lib = _hip.load()
    x, l = _rows2d(inputs), _rows2d(logits)
    n, d = x.shape
    out = torch.empty(n, dtype=torch.float32, device=x.device)
    _call("fc_bernoulli_log_prob", lib.fc_bernoulli_log_prob, x.device, _hip.ptr(x), _hip.ptr(l), _hip.ptr(add),
          _hip.ptr(out), n, d, _hip.stream_ptr(x.device))
    return out


class _BernoulliLogProbFunction(torch.autograd.Function):
    """``fc_bernoulli_log_prob`` with ``fc_bernoulli_log_prob_backward`` as its gradient: one launch writes the gradients
    that are asked for, from the saved ``inputs`` and ``logits`` alone.  Under ``create_graph`` the backward is the same
    expression in torch ops, so that a second derivative exists."""

    @staticmethod
    def forward(ctx, inputs, logits, add):
        out = _bernoulli_log_prob_nograd(inputs, logits, add)
        ctx.save_for_backward(inputs, logits)
        return out

    @staticmethod
    def backward(ctx, grad):
        inputs, logits = ctx.saved_tensors
        want_inputs, want_logits, want_add = ctx.needs_input_grad
        grad_add = grad if want_add else None
        if not (want_inputs or want_logits):
            return None, None, grad_add
        if torch.is_grad_enabled():
            rows = grad.reshape((-1,) + (1,) * (logits.dim() - 1))
            return (rows * logits if want_inputs else None,
                    rows * (inputs - torch.sigmoid(logits)) if want_logits else None, grad_add)
        lib = _hip.load()
        grad = _hip.dev_f32(grad, "grad_log_prob")      # (the gradient of a plain .sum() arrives as an expanded scalar)
        x, l = _rows2d(inputs), _rows2d(logits)
        n, d = l.shape
        gx = torch.empty_like(inputs) if want_inputs else None
        gl = torch.empty_like(logits) if want_logits else None
        _call("fc_bernoulli_log_prob_backward", lib.fc_bernoulli_log_prob_backward, l.device, _hip.ptr(x), _hip.ptr(l),
              _hip.ptr(grad), _hip.ptr(gl), _hip.ptr(gx), n, d, _hip.stream_ptr(l.device))
        return gx, gl, grad_add


def bernoulli_log_prob(inputs, logits, add=None):
    """``sum_d ( x l - softplus(l) ) (+ add)`` -> [N]: the log-probability of ``inputs`` [N, ...] under independent
    Bernoullis with ``logits`` of the same shape (reference distributions/discrete.py:54-55; equal to it for every real
    ``inputs``, not only 0 / 1).  ``add`` [N] is folded into the same pass.  Records an autograd node when gradients are
    required."""
    if inputs.shape != logits.shape or inputs.dim() < 1:
        raise ValueError("bernoulli_log_prob: inputs %s and logits %s must have one shape"
                         % (tuple(inputs.shape), tuple(logits.shape)))
    if add is not None and add.shape != inputs.shape[:1]:
        raise ValueError("bernoulli_log_prob: add must have one entry per row")
    operands = (inputs, logits) if add is None else (inputs, logits, add)
    if not _fast(*operands) or inputs.numel() == 0:
        return _bernoulli_log_prob_torch(inputs, logits, add)
    if torch.is_grad_enabled() and any(t.requires_grad for t in operands):
        return _BernoulliLogProbFunction.apply(inputs, logits, add)
    return _bernoulli_log_prob_nograd(inputs, logits, add)


# ---- Bernoulli sampler -----------------------------------------------------------------------------------------------
def bernoulli_sample(logits, noise, num_samples):
    """``(noise < sigmoid(logits repeated num_samples times per row)).float()``: ``logits`` [C, ...], ``noise``
    [C * num_samples, ...] uniform on [0, 1) -> draws of ``noise``'s shape (reference distributions/discrete.py:58-67).  The
    kernel reads each context row's logits in place; no gradient flows through a draw."""
    num_samples = int(num_samples)
    if (num_samples < 1 or noise.dim() != logits.dim() or noise.shape[1:] != logits.shape[1:]
            or noise.shape[0] != logits.shape[0] * num_samples):
        raise ValueError("bernoulli_sample: noise %s does not match %d draws of logits %s"
                         % (tuple(noise.shape), num_samples, tuple(logits.shape)))
    logits, noise = logits.detach(), noise.detach()
    if not _fast(logits, noise) or noise.numel() == 0:
        probs = torch.sigmoid(logits).repeat_interleave(num_samples, dim=0)
        return (noise < probs).float()
    lib = _hip.load()
    l = _rows2d(logits)
    out = torch.empty_like(noise)
    _call("fc_bernoulli_sample", lib.fc_bernoulli_sample, l.device, _hip.ptr(l), _hip.ptr(noise), _hip.ptr(out), l.shape[0],
          num_samples, l.shape[1], _hip.stream_ptr(l.device))
    return out


# ---- box uniform -----------------------------------------------------------------------------------------------------
def _box_log_prob_torch(inputs, low, high):
    """``torch.distributions.Uniform.log_prob`` summed over the event dimension."""
    lb = low.le(inputs).type_as(low)
    ub = high.gt(inputs).type_as(low)
    return (torch.log(lb.mul(ub)) - torch.log(high - low)).sum(-1)


def box_log_prob(inputs, low, high):
    """Log-density of ``inputs`` [..., D] under the uniform distribution on the box ``low <= x < high`` (both [D]):
    ``-sum_d log(high_d - low_d)`` inside, ``-inf`` outside or at a NaN.  The density is piecewise constant: the kernel
    runs where nothing requires a gradient, the torch expression otherwise."""
    if low.dim() != 1 or low.shape != high.shape or inputs.dim() < 1 or inputs.shape[-1] != low.shape[0]:
        raise ValueError("box_log_prob: inputs %s do not match low %s / high %s"
                         % (tuple(inputs.shape), tuple(low.shape), tuple(high.shape)))
    wants_grad = torch.is_grad_enabled() and any(t.requires_grad for t in (inputs, low, high))
    if wants_grad or not _fast(inputs, low, high) or inputs.numel() == 0:
        return _box_log_prob_torch(inputs, low, high)
    lib = _hip.load()
    d = low.shape[0]
    out = torch.empty(inputs.shape[:-1], dtype=torch.float32, device=inputs.device)
    _call("fc_box_log_prob", lib.fc_box_log_prob, inputs.device, _hip.ptr(inputs), _hip.ptr(low), _hip.ptr(high),
          _hip.ptr(out), inputs.numel() // d, d, _hip.stream_ptr(inputs.device))
    return out
