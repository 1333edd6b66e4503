"""Mixture-of-Gaussians MADE: the density and the one-kernel sampler."""
import torch

from flowconductor_amd import _hip
from ._core import _call, _logabsdet_target, _prep_2d
from .conditioner import HIDDEN_ROWS, _made_arguments, _made_context_pack, _made_pack_matches


MOG_MAX_COMPONENTS = 16


def _mog_operands(inputs, params, components):
    x = _prep_2d(inputs)
    p = _prep_2d(params, "params")
    n, d = x.shape
    if not 1 <= components <= MOG_MAX_COMPONENTS:
        raise ValueError("fc_mog_log_prob: 1 <= num_mixture_components <= %d" % MOG_MAX_COMPONENTS)
    if d < 1 or p.shape != (n, d * 3 * components) or p.device != x.device:
        raise ValueError("fc_mog_log_prob: params must be [N, D * 3 * components] on the inputs' device, got %s for inputs %s"
                         % (tuple(p.shape), tuple(x.shape)))
    return x, p, n, d


def _mog_log_prob_nograd(inputs, params, components, epsilon, logp_accum=None):
    lib = _hip.load()
    _hip.require_no_grad(inputs, params)
    x, p, n, d = _mog_operands(inputs, params, components)
    logp, flags = _logabsdet_target(logp_accum, n, x.device)
    _call("fc_mog_log_prob", lib.fc_mog_log_prob, x.device, _hip.ptr(x), _hip.ptr(p), _hip.ptr(logp), n, d, int(components),
          float(epsilon), flags, _hip.stream_ptr(x.device))
    return logp


def mog_log_prob_backward(grad_logp, inputs, params, components, epsilon):
    """``(grad_inputs [N, D], grad_params [N, D * 3C])`` of ``sum(grad_logp * mog_log_prob(inputs, params))``
    (``fc_mog_log_prob_backward``: the responsibilities are recomputed, nothing of the forward is kept)."""
    lib = _hip.load()
    x, p, n, d = _mog_operands(inputs, params, components)
    g = _hip.dev_f32(grad_logp, "grad_logp")
    if g.shape != (n,):
        raise ValueError("grad_logp must be [N]")
    gx, gp = torch.empty_like(x), torch.empty_like(p)
    _call("fc_mog_log_prob_backward", lib.fc_mog_log_prob_backward, x.device, _hip.ptr(g), _hip.ptr(x), _hip.ptr(p), _hip.ptr(gx),
          _hip.ptr(gp), n, d, int(components), float(epsilon), _hip.stream_ptr(x.device))
    return gx, gp


class _MoGLogProbFunction(torch.autograd.Function):
    """``fc_mog_log_prob`` with ``fc_mog_log_prob_backward`` as its gradient."""

    @staticmethod
    def forward(ctx, inputs, params, components, epsilon):
        with torch.no_grad():
            out = _mog_log_prob_nograd(inputs, params, components, epsilon)
        ctx.save_for_backward(inputs, params)
        ctx.form = (components, epsilon)
        return out

    @staticmethod
    def backward(ctx, grad):
        inputs, params = ctx.saved_tensors
        with torch.no_grad():
            gx, gp = mog_log_prob_backward(grad.contiguous(), inputs, params, *ctx.form)
        return (gx if ctx.needs_input_grad[0] else None), (gp if ctx.needs_input_grad[1] else None), None, None


def mog_log_prob(inputs, params, components, epsilon, logp_accum=None):
    """Log-density [N] of ``inputs`` [N, D] under the mixtures a ``MixtureOfGaussiansMADE`` emits: ``params``
    [N, D * 3 * components], per element ``components`` x (logit, mean, unconstrained std) (nn/nde/made.py:328-353),
    ``std = softplus(ustd) + epsilon``.  ``logp_accum`` [N]: added onto (inference only).  Records an autograd node when
    gradients are required."""
    if torch.is_grad_enabled() and (inputs.requires_grad or params.requires_grad):
        if logp_accum is not None:
            raise ValueError("mog_log_prob: logp_accum is for inference")
        return _MoGLogProbFunction.apply(inputs, params, int(components), float(epsilon))
    return _mog_log_prob_nograd(inputs, params, components, epsilon, logp_accum)


def made_mog_sample(normal, uniform, packed, num_blocks, components, epsilon, context=None, context_pack=None):
    """The D passes of a ``MixtureOfGaussiansMADE``'s ancestral sampler in ONE kernel (``fc_made_mog_sample``): ``normal``,
    ``uniform`` [N, 1 < D <= 64] noise (rows a multiple of 16), ``packed`` from ``pack_made_inverse`` with ``per_dim =
    3 * components``.  With ``context`` [N, C <= 32] and ``context_pack`` from ``pack_made_inverse_context`` the conditional
    form (``fc_made_mog_sample_context``).  Returns ``(draws [N, D], their log-density [N])``."""
    lib = _hip.load()
    z = _prep_2d(normal, "normal")
    u = _prep_2d(uniform, "uniform")
    _hip.require_no_grad(normal, uniform, context)
    n, d = z.shape
    per_dim = 3 * int(components)
    if n % HIDDEN_ROWS != 0 or d > 64 or u.shape != z.shape or u.device != z.device:
        raise ValueError("fc_made_mog_sample: normal and uniform must both be [N, D <= 64], N a multiple of %d" % HIDDEN_ROWS)
    if not 1 <= components <= MOG_MAX_COMPONENTS:
        raise ValueError("fc_made_mog_sample: 1 <= num_mixture_components <= %d" % MOG_MAX_COMPONENTS)
    if (context is None) != (context_pack is None):
        raise ValueError("made_mog_sample: context and context_pack go together")
    if not _made_pack_matches(packed, d) or packed[5].numel() != d * 16 * -(-per_dim // 16):
        raise ValueError("made_mog_sample: the pack does not match D = %d, %d components" % (d, components))
    rows = (z, u) if context is None else (z, u, context)
    if context is not None:
        context_pack = _made_context_pack("made_mog_sample", "noise's", z.device, n, d, context, context_pack, num_blocks, per_dim,
                                          components, "components")
    x = torch.empty_like(z)
    logp = torch.empty(n, dtype=torch.float32, device=z.device)
    name = "fc_made_mog_sample" if context is None else "fc_made_mog_sample_context"
    _call(name, getattr(lib, name), z.device,
          *_made_arguments(rows, (x, logp), packed, context_pack or (), n, d, num_blocks, (int(components), float(epsilon))))
    return x, logp
