"""Unconstrained monotonic neural networks: the Clenshaw-Curtis integral of a small MLP on the matrix cores."""
import numpy as np
import torch

from flowconductor_amd import _hip
from ._core import LAD_STORE, _call, _logabsdet_target, _pad_to, _prep_2d, cache_key, memo, once_differentiable
from .packing import _bias_accumulator_order, _hb_perm, _hidden_layer_fragments, _pow2_scale

UMNN_MAX_HIDDEN_LAYERS = 3
UMNN_MAX_WIDTH = 64
UMNN_MAX_COND = 31
UMNN_MAX_STEPS = 63
UMNN_POINTS = 68          # entries of the node / weight tables of the image


def umnn_fits(cond_size, hidden_widths, nb_steps):
    """Whether ``fc_umnn`` takes an integrand of this shape: 1 to 3 hidden layers of width <= 64 (zero-padded), an
    embedding of <= 31 values (one k-step together with t) and <= 63 quadrature steps.  Everything else takes the torch
    composition."""
    hidden_widths = list(hidden_widths)
    return (1 <= len(hidden_widths) <= UMNN_MAX_HIDDEN_LAYERS and all(1 <= w <= UMNN_MAX_WIDTH for w in hidden_widths)
            and 0 <= cond_size <= UMNN_MAX_COND and 1 <= nb_steps <= UMNN_MAX_STEPS)


def umnn_image_floats(hidden_layers):
    """float32 entries of the image's second part (layout: include/flowcon_hip.h)."""
    return hidden_layers * 64 + 64 + 64 + 4 + 2 * UMNN_POINTS


def pack_umnn(linears, nb_steps, device):
    """The integrand ``linears`` (first, hidden.., last) and the quadrature rule as ``fc_umnn`` keeps them in LDS:
    ``(frag, aux)`` -- f16 A fragments of the first layer (one k-step: column 0 multiplies t, columns 1.. the embedding)
    and of the hidden 64 x 64 layers, each scaled by a power of two and split in two pieces, rows in accumulator order;
    float32 biases in accumulator order, the t column of the first layer, the last layer's row, the layers' unscale
    factors, the last bias, and the tables ``(s_i + 1) / 2`` and ``w_i`` rounded from ``cc_weights``' float64."""
    from flowconductor_amd.transforms.UMNN import cc_weights

    with torch.no_grad():
        perm = _hb_perm().to(device)
        mfma = linears[:-1]
        frags, biases, uns = [], [], []
        for i, lin in enumerate(mfma):
            w = _pad_to(lin.weight.detach().to(device=device, dtype=torch.float32), (64, 32 if i == 0 else 64))
            if i == 0:
                w1t = w[:, 0].clone()
                w = w.clone()
                w[:, 0] = 0          # t's column stays in float32 (one fma per unit and point)
            sc, un = _pow2_scale(w.abs().amax().reshape(1))
            frags.append(_hidden_layer_fragments(w * sc, perm))
            uns.append(un.reshape(1))
            biases.append(_bias_accumulator_order(
                _pad_to(lin.bias.detach().to(device=device, dtype=torch.float32), (64,)), perm))
        last = linears[-1]
        wlast = _pad_to(last.weight.detach().to(device=device, dtype=torch.float32).reshape(-1), (64,))
        misc = torch.zeros(4, dtype=torch.float32, device=device)
        misc[:len(uns)] = torch.cat(uns)
        misc[3] = last.bias.detach().to(device=device, dtype=torch.float32).reshape(())
        nodes, weights = cc_weights(nb_steps)
        tt = np.ones(UMNN_POINTS)               # beyond the rule: t = x (the Jacobian point), weight 0
        ww = np.zeros(UMNN_POINTS)
        tt[:nb_steps + 1] = 0.5 * (nodes + 1.0)
        ww[:nb_steps + 1] = weights
        aux = torch.cat(biases + [_bias_accumulator_order(w1t, perm), _bias_accumulator_order(wlast, perm), misc,
                                  torch.as_tensor(tt, dtype=torch.float32).to(device),
                                  torch.as_tensor(ww, dtype=torch.float32).to(device)]).contiguous()
        frag = torch.cat(frags).contiguous()
    assert aux.numel() == umnn_image_floats(len(mfma)) and frag.numel() == (8 + 16 * (len(mfma) - 1)) * 512
    return frag, aux


def umnn_image(owner, linears, nb_steps, device):
    """``pack_umnn`` of ``owner``'s integrand, kept in the owner's run-time store under the parameters' versions (a copy
    or a pickle of the owner carries none of it)."""
    params = [t for lin in linears for t in (lin.weight, lin.bias)]
    key = cache_key(*params, extra=(nb_steps, device))
    return memo(owner, "umnn_image", key, lambda: pack_umnn(linears, nb_steps, device))


def umnn(inputs, h, image, cond_size, nb_steps, inverse=False, lad_mode=LAD_STORE, logabsdet=None):
    """``(outputs [N, D], logabsdet [N], jac [N, D])`` of z = h_0 + int_0^x f(t, h) dt (or of its inverse) for
    ``h`` [N, D, cond_size] and a ``pack_umnn`` image; ``jac`` = f at the x of each element, logabsdet = +-sum log jac
    (``lad_mode``: one of ``LAD_*``; the accumulating ones add onto ``logabsdet`` in place)."""
    lib = _hip.load()
    x = _prep_2d(inputs)
    emb = _hip.dev_f32(h, "h")
    _hip.require_no_grad(inputs, h)
    frag, aux = image
    n, d = x.shape
    if emb.numel() != n * d * cond_size:
        raise ValueError("h has %d elements, expected %d" % (emb.numel(), n * d * cond_size))
    hidden_layers = (frag.numel() // 512 - 8) // 16 + 1
    if frag.device != x.device or aux.device != x.device or aux.numel() != umnn_image_floats(hidden_layers):
        raise ValueError("flowconductor_amd: the integrand image does not belong to these inputs")
    y = torch.empty_like(x)
    jac = torch.empty_like(x)
    if lad_mode & 1:
        if logabsdet is None:
            raise ValueError("an accumulating lad_mode needs the running logabsdet")
        lad, _ = _logabsdet_target(logabsdet, n, x.device)
    else:
        lad = torch.empty(n, dtype=torch.float32, device=x.device)
    _call("fc_umnn", lib.fc_umnn, x.device, _hip.ptr(x), _hip.ptr(emb), _hip.ptr(frag), _hip.ptr(aux), _hip.ptr(y),
          _hip.ptr(jac), _hip.ptr(lad), n, d, cond_size, hidden_layers, nb_steps, 1 if inverse else 0, int(lad_mode),
          _hip.stream_ptr(x.device))
    return y, lad, jac


# ---- training: fc_umnn_backward ------------------------------------------------------------------------------------------
UMNN_DOUBLE_BACKWARD_MSG = (
    "flowconductor_amd: the UMNN kernel route (options 'umnn_training') is once differentiable; for a gradient of a "
    "gradient (create_graph=True) run the layer with options.override(umnn_training=False), the torch composition")


def umnn_grad_floats(hidden_layers):
    """float32 entries of ``fc_umnn_backward``'s gradient image (layout: include/flowcon_hip.h)."""
    return 64 * 32 + (hidden_layers - 1) * 64 * 64 + 64 * hidden_layers + 64 + 4


def pack_umnn_backward(linears, device):
    """The transposed image of ``fc_umnn_backward``: ``_hidden_layer_fragments`` of W_l^T for the hidden 64 x 64 layers,
    then of W1[:, 1:]^T (32 x 64, slot 0 -- t's -- zero), each with the power-of-two scale ``pack_umnn`` gave its layer
    (the largest entry of a matrix is that of its transpose), rows in accumulator order."""
    with torch.no_grad():
        perm = _hb_perm().to(device)
        mfma = linears[:-1]
        frags = []
        for lin in mfma[1:]:
            w = _pad_to(lin.weight.detach().to(device=device, dtype=torch.float32), (64, 64))
            sc, _ = _pow2_scale(w.abs().amax().reshape(1))
            frags.append(_hidden_layer_fragments(w.t().contiguous() * sc, perm))
        w = _pad_to(mfma[0].weight.detach().to(device=device, dtype=torch.float32), (64, 32)).clone()
        w[:, 0] = 0
        sc, _ = _pow2_scale(w.abs().amax().reshape(1))
        frags.append(_hidden_layer_fragments(w.t().contiguous() * sc, perm[:32]))
        fragt = torch.cat(frags).contiguous()
    assert fragt.numel() == (16 * (len(mfma) - 1) + 8) * 512
    return fragt


def umnn_backward_image(owner, linears, device):
    """``pack_umnn_backward`` of ``owner``'s integrand in the owner's run-time store, keyed as ``umnn_image``."""
    params = [t for lin in linears for t in (lin.weight, lin.bias)]
    key = cache_key(*params, extra=(device,))
    return memo(owner, "umnn_backward_image", key, lambda: pack_umnn_backward(linears, device))


def umnn_backward(x, h, image, image_t, grad_out, grad_jac, cond_size, nb_steps, inverse=False):
    """The raw ``fc_umnn_backward``: ``(grad_in [N, D], grad_h [N, D, cond_size], grad_params [umnn_grad_floats])`` for
    ``x`` the forward call's input (``inverse``: the root it returned), ``grad_out`` the gradient of the call's output and
    ``grad_jac`` that of ``jac`` with logabsdet's folded in."""
    lib = _hip.load()
    x = _prep_2d(x)
    emb = _hip.dev_f32(h, "h")
    go = _hip.dev_f32(grad_out, "grad_out")
    gj = _hip.dev_f32(grad_jac, "grad_jac")
    frag, aux = image
    n, d = x.shape
    hidden_layers = (frag.numel() // 512 - 8) // 16 + 1
    if emb.numel() != n * d * cond_size or go.shape != x.shape or gj.shape != x.shape:
        raise ValueError("flowconductor_amd: umnn_backward: the shapes of h / grad_out / grad_jac do not belong to x")
    if (frag.device != x.device or aux.device != x.device or image_t.device != x.device
            or aux.numel() != umnn_image_floats(hidden_layers) or image_t.numel() != (16 * (hidden_layers - 1) + 8) * 512):
        raise ValueError("flowconductor_amd: the integrand images do not belong to these inputs")
    gin = torch.empty_like(x)
    gh = torch.empty((n, d, cond_size), dtype=torch.float32, device=x.device)
    gp = torch.empty(umnn_grad_floats(hidden_layers), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        floats = lib.fc_umnn_backward_workspace(n, d, hidden_layers)
    if floats < 0:
        raise ValueError("flowconductor_amd: umnn_backward: outside the kernel's limits")
    ws = torch.empty(max(floats, 1), dtype=torch.float32, device=x.device)
    _call("fc_umnn_backward", lib.fc_umnn_backward, x.device, _hip.ptr(x), _hip.ptr(emb), _hip.ptr(frag), _hip.ptr(aux),
          _hip.ptr(image_t), _hip.ptr(go), _hip.ptr(gj), _hip.ptr(gin), _hip.ptr(gh), _hip.ptr(gp), _hip.ptr(ws), n, d,
          cond_size, hidden_layers, nb_steps, 1 if inverse else 0, _hip.stream_ptr(x.device))
    return gin, gh, gp


def umnn_unpack_grads(grad_params, linears):
    """The padded gradient image as tensors of the shapes of ``linears``' ``weight`` / ``bias``, in that order."""
    nl = len(linears) - 1
    o_wh = 64 * 32
    o_b = o_wh + (nl - 1) * 4096
    o_wl = o_b + 64 * nl
    out = []
    for i, lin in enumerate(linears[:-1]):
        rows, cols = lin.weight.shape
        if i == 0:
            w = grad_params[:o_wh].view(64, 32)
        else:
            w = grad_params[o_wh + (i - 1) * 4096:o_wh + i * 4096].view(64, 64)
        out += [w[:rows, :cols].contiguous(), grad_params[o_b + 64 * i:o_b + 64 * i + rows].clone()]
    last = linears[-1]
    out += [grad_params[o_wl:o_wl + last.weight.shape[1]].reshape(last.weight.shape).clone(),
            grad_params[o_wl + 64:o_wl + 65].reshape(last.bias.shape).clone()]
    return out


class _UMNNFunction(torch.autograd.Function):
    """``fc_umnn`` with ``fc_umnn_backward``: saves the input (or the root), ``h`` and ``jac`` -- nothing of size
    N D points exists in either pass."""

    @staticmethod
    def forward(ctx, inputs, h, owner, linears, cond_size, nb_steps, inverse, *params):
        device = inputs.device
        image = umnn_image(owner, linears, nb_steps, device)
        out, lad, jac = umnn(inputs, h, image, cond_size, nb_steps, inverse=inverse)
        ctx.image = image
        ctx.image_t = umnn_backward_image(owner, linears, device)
        ctx.linears = linears
        ctx.meta = (cond_size, nb_steps, bool(inverse), tuple(h.shape))
        ctx.save_for_backward(out if inverse else _prep_2d(inputs), h, jac)
        return out, lad, jac

    @staticmethod
    @once_differentiable(UMNN_DOUBLE_BACKWARD_MSG)
    def backward(ctx, grad_out, grad_lad, grad_jac):
        x, h, jac = ctx.saved_tensors
        cond_size, nb_steps, inverse, h_shape = ctx.meta
        fold = grad_lad.unsqueeze(1) / jac                       # logabsdet = +-sum log jac
        gj = grad_jac - fold if inverse else grad_jac + fold
        gin, gh, gp = umnn_backward(x, h, ctx.image, ctx.image_t, grad_out.contiguous(), gj.contiguous(), cond_size,
                                    nb_steps, inverse=inverse)
        need = ctx.needs_input_grad
        grads = [g if need[7 + i] else None for i, g in enumerate(umnn_unpack_grads(gp, ctx.linears))]
        return (gin if need[0] else None, gh.view(h_shape) if need[1] else None, None, None, None, None, None, *grads)


def umnn_autograd(inputs, h, linears, owner, cond_size, nb_steps, inverse=False):
    """``(outputs, logabsdet, jac)`` of ``umnn`` under autograd: gradients reach ``inputs``, ``h`` and the parameters of
    ``linears`` through ``fc_umnn_backward`` (the images live in ``owner``'s run-time store).  Once differentiable."""
    params = [t for lin in linears for t in (lin.weight, lin.bias)]
    return _UMNNFunction.apply(inputs, h, owner, linears, cond_size, nb_steps, inverse, *params)
