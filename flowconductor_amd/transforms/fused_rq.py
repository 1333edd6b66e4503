"""The conditioner's final Linear evaluated inside the RQ-spline kernel: what the coupling, the conditional and the
autoregressive layer share of that path.

Two kernels: "k8" -- ``fc_rq_spline_fused_linear``, K = 8 with linear tails and hidden <= 64 -- and "general" --
``fc_rq_spline_fused_general``, K = 4..16, tails or a box, hidden <= 256.  Both take up to 32 transformed dims per launch
and whole 32-row rounds.  A layer decides whether it qualifies at all (grad state, hooks, options, its net), which weight
it packs, the spline's keyword arguments and how the < 32 leftover rows get their parameters; the rest is here."""
import torch

from flowconductor_amd import ops


def fused_mode(n, d, d_t, hidden, num_bins, tails, general_hidden):
    """None, "k8" or "general" for [n, d] inputs with ``d_t`` transformed dims per launch and a final Linear of ``hidden``
    inputs.  ``general_hidden``: the hidden width the layer would hand the general kernel (None: it has no such form)."""
    if ops.fused_linear_supported(n, d, d_t, hidden, num_bins, tails):
        return "k8"
    if general_hidden is not None and ops.fused_general_supported(n, d, d_t, general_hidden, num_bins, tails):
        return "general"
    return None


def packed_chunks(owner, lin, mode, num_bins, tails, spec):
    """The final Linear ``lin`` in the layout of ``mode``, cached on ``owner`` as ``{mode: chunks}`` per ``cache_key`` of
    the parameters: one ``(w_pad, bias_pad, cols)`` ("k8") or ``(w_frag, w_unscale, bias_pad, cols)`` ("general") per
    group of transformed dims.  Only a miss asks the layer what to pack: ``spec()`` -> ``(weight, hidden_pad, [(row slice
    of the weight, cols)])`` -- ``lin.weight`` or a MADE's ``weight * mask``, the hidden width "general" zero-pads to."""
    by_mode = ops.memo(owner, "packed", ops.cache_key(lin.weight, lin.bias), dict)
    packed = by_mode.get(mode)
    if packed is None:
        weight, hidden_pad, groups = spec()
        packed = []
        for rows, cols in groups:
            if mode == "k8":
                images = ops.pack_final_layer(weight[rows], lin.bias[rows], num_bins)
            else:
                images = ops.pack_final_layer_general(weight[rows], lin.bias[rows], num_bins, tails, hidden_pad)
            packed.append(tuple(images) + (cols,))
        by_mode[mode] = packed
    return packed


def run_chunks(inputs, hidden, chunks, mode, kw, logabsdet_accum=None):
    """One launch per chunk, each passing the columns of the others through and adding onto the logabsdet of the one before
    (the groups only depend on the identity columns: any order).  Rows a multiple of 32."""
    fn = ops.rq_spline_fused_linear if mode == "k8" else ops.rq_spline_fused_general
    rows, lad = inputs, logabsdet_accum
    for chunk in chunks:
        rows, lad = fn(rows, hidden, *chunk, logabsdet_accum=lad, **kw)
    return rows, lad


def apply(inputs, hidden, chunks, mode, kw, total, leftover_fn):
    """``(outputs, logabsdet)`` of the layer: the whole 32-row rounds through ``run_chunks``, the < 32 leftover rows through
    ``leftover_fn(rows, hidden_rows) -> (outputs, logabsdet)``.  With a running ``total`` [N] the layer's logabsdet is added
    onto it in place and ``total`` is returned."""
    n = inputs.shape[0]
    body = n - n % ops.FUSED_ROWS
    if body == n:
        if len(chunks) == 1:      # the usual layer, <= 32 transformed dims: nothing to chain or join, one call
            fn = ops.rq_spline_fused_linear if mode == "k8" else ops.rq_spline_fused_general
            return fn(inputs, hidden, *chunks[0], logabsdet_accum=total, **kw)
        return run_chunks(inputs, hidden, chunks, mode, kw, total)
    out_a, lad_a = run_chunks(inputs[:body], hidden[:body], chunks, mode, kw, None if total is None else total[:body])
    out_b, lad_b = leftover_fn(inputs[body:].contiguous(), hidden[body:])
    outputs = torch.cat((out_a, out_b))
    if total is None:
        return outputs, torch.cat((lad_a, lad_b))
    total[body:] += lad_b
    return outputs, total
