"""Unconstrained monotonic neural networks: the Clenshaw-Curtis integral of a small MLP on the matrix cores."""
import numpy as np
import torch

from flowconductor_amd import _hip
from ._core import LAD_STORE, _call, _logabsdet_target, _pad_to, _prep_2d, cache_key, memo
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
