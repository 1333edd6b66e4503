"""Weights as the matrix-core kernels read them: power-of-two scaled, split into two f16 pieces, in fragment order.

The ``pack_*`` functions build an image with tensor ops; ``DevicePack`` and the ``device_pack_*`` builders make the
same images with one ``fc_pack_fragments`` launch that re-packs in place after every optimizer step.
"""
import ctypes

import torch

from flowconductor_amd import _hip
from flowconductor_amd.runtime_cache import cache_key
from ._core import _call, _pad_to, rq_param_count


FUSED_ROWS, FUSED_HIDDEN, FUSED_DT, FUSED_BINS = 32, 64, 32, 8


def pack_resnet_hidden(net):
    """Weights of the hidden layers of a ResidualNet (hidden <= 64, <= 4 blocks) as ``fc_resnet_hidden`` takes
    them: the nn.Linear tensors row-major, the block layers stacked [blocks, 2, 64, 64] / [blocks, 2, 64]; with a
    context also the blocks' ``context_layer`` stacked [blocks, 64, C] / [blocks, 64].  A narrower net is embedded
    in the 64-wide kernel by zero padding: the extra hidden units have zero weights and biases, stay 0 through ReLU
    and the residual stream, and meet zero columns in every following layer."""
    hw = FUSED_HIDDEN
    w0 = _pad_to(net.initial_layer.weight.detach(), (hw, net.initial_layer.in_features))
    b0 = _pad_to(net.initial_layer.bias.detach(), (hw,))
    ws, bs, wcs, bcs = [], [], [], []
    for block in net.blocks:
        for lin in block.linear_layers:
            ws.append(_pad_to(lin.weight.detach(), (hw, hw)))
            bs.append(_pad_to(lin.bias.detach(), (hw,)))
        if getattr(block, "context_layer", None) is not None:
            cl = block.context_layer
            wcs.append(_pad_to(cl.weight.detach(), (hw, cl.in_features)))
            bcs.append(_pad_to(cl.bias.detach(), (hw,)))
    wb = torch.stack(ws).contiguous() if ws else None
    bb = torch.stack(bs).contiguous() if bs else None
    wc = torch.stack(wcs).contiguous() if wcs else None
    bc = torch.stack(bcs).contiguous() if bcs else None
    return w0, b0, wb, bb, wc, bc


def _exact_pow2(shift):
    """2^shift as float32, built from the exponent bits (``torch.ldexp`` goes through ``pow`` and is not exact on every
    backend)."""
    return ((shift.to(torch.int32) + 127) << 23).view(torch.float32)


def _pow2_scale(m):
    """fc_split.h pow2_scale on a tensor of maxima: (scale, unscale), exact powers of two lifting each into [2^14, 2^15)."""
    _, exp = torch.frexp(m)                                   # m = mant * 2^exp, mant in [0.5, 1)
    ok = (m > 0) & torch.isfinite(m) & (exp >= -111)
    shift = torch.where(ok, 15 - exp, torch.zeros_like(exp))
    return _exact_pow2(shift), _exact_pow2(-shift)


def _a_fragments(w):
    """[rows (multiple of 16), K (multiple of 32)] f32, already scaled -> f16 [rows/16, K/32, 2 (hi, lo), 64, 8]: the
    matrix-core A fragments of v_mfma_f32_16x16x32_f16 (lane l holds row l & 15, k = 32 kstep + 8 (l >> 4) + j)."""
    rows, k = w.shape
    hi = w.to(torch.float16)
    lo = (w - hi.float()).to(torch.float16)

    def frag(piece):
        return piece.reshape(rows // 16, 16, k // 32, 4, 8).permute(0, 2, 3, 1, 4).reshape(rows // 16, k // 32, 64, 8)

    return torch.stack((frag(hi), frag(lo)), dim=2).contiguous()


FRAG_ELEMS = 2 * 64 * 8                 # f16 values of one A fragment: (hi, lo) pieces x 64 lanes x 8
FRAG_KSTEP = 4 * FRAG_ELEMS             # one 32-column k-step of a 64-row layer: four 16-row tiles


def _hb_perm():
    """Feature held by accumulator tile t, row rho of the hidden-layer kernels: 32 (t >> 1) + 8 g + 4 (t & 1) + r with
    g = rho >> 2, r = rho & 3 (the order in which the C layout of one layer is the B operand of the next)."""
    return torch.tensor([32 * (t >> 1) + 8 * (rho >> 2) + 4 * (t & 1) + (rho & 3) for t in range(4) for rho in range(16)])


def _hidden_layer_fragments(w_scaled, perm=None):
    """A scaled [rows, 32 ks] layer -> flat f16 fragments [ks][t][piece][lane][8]; row r of the image is row ``perm[r]``
    of ``w_scaled`` (``_hb_perm``: the accumulator order; None: the rows as they are)."""
    if perm is not None:
        w_scaled = w_scaled[perm]
    return _a_fragments(w_scaled).permute(1, 0, 2, 3, 4).reshape(-1)


def _bias_accumulator_order(b, perm=None):
    """A [64] bias as the hidden-layer kernels add it to their accumulators (``perm`` as in ``_hidden_layer_fragments``)."""
    if perm is not None:
        b = b[perm]
    return b.reshape(4, 4, 4).permute(1, 0, 2).reshape(-1)


def _hidden_linears(net):
    """The Linear layers of a ResidualNet's / MADE's hidden stack in the order the kernels walk them."""
    return [net.initial_layer] + [lin for block in net.blocks for lin in block.linear_layers]


def pack_resnet_hidden_wide(net, width):
    """Hidden layers of a ResidualNet with 64 < hidden_features <= 256 (no context) as ``fc_resnet_hidden_wide``
    streams them: every layer's weight zero-padded to ``width`` (128 / 256) rows and 32-multiples of columns, scaled
    by a power of two per layer, split into two f16 pieces, in fragment order; all layers in one flat f16 buffer.
    Returns (w_frag, w_unscale [1 + 2 blocks], bias [1 + 2 blocks, width])."""
    layers = _hidden_linears(net)
    frags, uns, biases = [], [], []
    for i, lin in enumerate(layers):
        kin = (32 if lin.in_features <= 32 else 64) if i == 0 else width
        w = _pad_to(lin.weight.detach().float(), (width, kin))
        sc, un = _pow2_scale(w.abs().amax().reshape(1))
        frags.append(_a_fragments(w * sc).reshape(-1))
        uns.append(un)
        biases.append(_pad_to(lin.bias.detach().float(), (width,)))
    return torch.cat(frags).contiguous(), torch.cat(uns).float().contiguous(), torch.stack(biases).contiguous()


PACK_FINAL, PACK_FINAL_T, PACK_HIDDEN, PACK_HIDDEN_T, PACK_HIDDEN_T0 = range(5)


class DevicePack:
    """A set of ``fc_pack_job``s with persistent output buffers: ``run()`` re-packs all of them in ONE launch (training
    re-packs every optimizer step; with tensor ops that is ~100 tiny launches per coupling layer).  The source pointers
    are the parameters' storages, which optimizers update in place."""

    def __init__(self, device):
        self.device = device
        self.jobs = []
        self.keep = []            # tensors the jobs point into
        self.sources = []         # the parameters the jobs read (their versions say when a refresh is due)
        self._jobs_dev = None
        self._root = None         # the pack this one was merged into
        self.children = []        # packs merged into this one (they keep their own jobs)
        self._key = None
        self.prepare = []         # callables run before every launch (staging copies the jobs read from)

    def add(self, mode, weight, bias, frag, unscale, bias_out=None, p=0, pp=0, nks=0, nt=0, group=0, track=True):
        """``track=False``: ``weight`` / ``bias`` are staging copies refreshed by a ``prepare`` callable -- the caller lists
        the tensors they are made from in ``sources`` instead."""
        if not weight.is_contiguous() or weight.dtype != torch.float32:
            raise ValueError("DevicePack sources must be contiguous float32 tensors")
        job = _hip.PackJob()
        job.w, job.b = weight.data_ptr(), (0 if bias is None else bias.data_ptr())
        job.frag, job.unscale = frag.data_ptr(), unscale.data_ptr()
        job.bias_out = 0 if bias_out is None else bias_out.data_ptr()
        job.rows, job.cols = weight.shape
        job.mode, job.p, job.pp, job.nks, job.nt, job.group = mode, p, pp, nks, nt, group
        self.jobs.append(job)
        self.keep += [weight, bias, frag, unscale, bias_out]
        if track:
            self.sources += [t for t in (weight, bias) if t is not None]

    def root(self):
        node = self
        while node._root is not None:
            node = node._root
        return node

    def _invalidate(self):
        self._jobs_dev = self._key = None

    def _walk(self):
        yield self
        for child in self.children:
            yield from child._walk()

    def merge(self, other):
        """Adopt ``other``: one launch then refreshes both (a coupling layer's final-layer and hidden-stack images change
        together, once per optimizer step).  Non-destructive: ``other`` keeps its jobs and can be re-parented later (its
        previous parent lets go of it), so a rebuilt parent never inherits jobs whose sources are gone."""
        mine = self.root()
        if other is mine or other._root is mine:
            return
        if other.device != mine.device:
            raise ValueError("DevicePack.merge: packs live on different devices")
        if any(node is other for node in mine._walk()) or any(node is mine for node in other._walk()):
            return
        if other._root is not None:
            other._root.children = [c for c in other._root.children if c is not other]
            other._root.root()._invalidate()
        other._root = mine
        mine.children.append(other)
        mine._invalidate()

    def all_jobs(self):
        return [job for node in self._walk() for job in node.jobs]

    def all_sources(self):
        return [t for node in self._walk() for t in node.sources]

    def run(self):
        pack = self.root()
        lib = _hip.load()
        if pack._jobs_dev is None:
            if lib.fc_pack_job_bytes() != ctypes.sizeof(_hip.PackJob):
                raise RuntimeError("fc_pack_job layout mismatch between the header and the ctypes mirror")
            jobs = pack.all_jobs()
            raw = b"".join(bytes(j) for j in jobs)
            pack._jobs_dev = (torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(pack.device), len(jobs))
        for node in pack._walk():
            for fn in node.prepare:
                fn()
        _call("fc_pack_fragments", lib.fc_pack_fragments, pack.device, _hip.ptr(pack._jobs_dev[0]), pack._jobs_dev[1],
              _hip.stream_ptr(pack.device))

    def refresh(self):
        """``run()`` if any source parameter changed since the last refresh (``cache_key``: versions + cache epoch)."""
        pack = self.root()
        seen, srcs = set(), []
        for t in pack.all_sources():
            if id(t) not in seen:
                seen.add(id(t))
                srcs.append(t)
        key = cache_key(*srcs)
        if pack._key != key:
            pack.run()
            pack._key = key


def device_pack_final_layer(weight, bias, num_bins, tails, cols_chunks):
    """Forward and W^T fragments of the final Linear (hidden <= 64) for every group of <= 32 transformed dims, packed on
    the device.  ``cols_chunks``: [(row slice of the weight, cols tensor)].  Returns ``(pack, chunks)`` with chunks =
    [(w_frag, w_unscale, bias_pad, wt_frag, cols, row slice)]; call ``pack.run()`` whenever the weights changed."""
    p = rq_param_count(num_bins, tails)
    pp = -(-p // 4) * 4
    t = pp // 4
    kk = -(-pp // 8)
    dev = weight.device
    pack = DevicePack(dev)
    chunks = []
    for rows, cols in cols_chunks:
        w, b = weight[rows], bias[rows]
        d_t = w.shape[0] // p
        groups = -(-d_t // 4)
        w_frag = torch.empty(groups, 2, t, 2, 64, 8, dtype=torch.float16, device=dev)
        wt_frag = torch.empty(groups, 4, kk, 2, 64, 8, dtype=torch.float16, device=dev)
        w_un = torch.empty(groups, dtype=torch.float32, device=dev)
        wt_un = torch.empty(groups, dtype=torch.float32, device=dev)       # (equal to w_un: the same group maximum)
        bias_pad = torch.empty(groups, 4, pp, dtype=torch.float32, device=dev)
        for g in range(groups):
            pack.add(PACK_FINAL, w, b, w_frag[g], w_un[g:g + 1], bias_pad[g], p=p, pp=pp, nks=2, nt=t, group=g)
            pack.add(PACK_FINAL_T, w, None, wt_frag[g], wt_un[g:g + 1], None, p=p, pp=pp, nks=kk, nt=4, group=g)
        chunks.append((w_frag, w_un, bias_pad, wt_frag, cols, rows))
    return pack, chunks


def _hidden_image(n_layers, k0s, device):
    """Empty LDS weight image of a 64-wide hidden stack, ``(w_frag, w_unscale [L], bias_acc [L, 64])``: ``k0s`` k-steps
    for the initial layer, two for every later one."""
    w_frag = torch.empty((k0s + 2 * (n_layers - 1)) * FRAG_KSTEP, dtype=torch.float16, device=device)
    w_un = torch.empty(n_layers, dtype=torch.float32, device=device)
    bias_acc = torch.empty(n_layers, 64, dtype=torch.float32, device=device)
    return w_frag, w_un, bias_acc


def _hidden_image_fragments(frag, k0s, i):
    """Layer ``i``'s slice of a fragment buffer laid out as ``_hidden_image`` lays out ``w_frag``."""
    lo = 0 if i == 0 else k0s + 2 * (i - 1)
    return frag[lo * FRAG_KSTEP:(lo + (k0s if i == 0 else 2)) * FRAG_KSTEP]


def _add_hidden_jobs(pack, image, k0s, sources):
    """One ``PACK_HIDDEN`` job per ``(weight, bias, track)`` of ``sources`` (layer order) into ``image``."""
    w_frag, w_un, bias_acc = image
    for i, (weight, bias, track) in enumerate(sources):
        pack.add(PACK_HIDDEN, weight, bias, _hidden_image_fragments(w_frag, k0s, i), w_un[i:i + 1], bias_acc[i],
                 nks=k0s if i == 0 else 2, nt=4, track=track)


def device_pack_resnet_hidden_backward(net):
    """``pack_resnet_hidden_backward`` on the device: returns ``(pack, packed)``; ``pack.run()`` refreshes ``packed``."""
    dev = net.initial_layer.weight.device
    k0s = 1 if net.initial_layer.in_features <= 32 else 2
    layers = _hidden_linears(net)
    image = w_frag, w_un, bias_acc = _hidden_image(len(layers), k0s, dev)
    wt_frag = torch.empty_like(w_frag)          # the same matrices transposed: layers 1.. first, W0^T last
    wt_un = torch.empty_like(w_un)
    pack = DevicePack(dev)
    _add_hidden_jobs(pack, image, k0s, [(lin.weight, lin.bias, True) for lin in layers])
    per_layer = 2 * FRAG_KSTEP
    for i, lin in enumerate(layers[1:]):
        pack.add(PACK_HIDDEN_T, lin.weight, None, wt_frag[i * per_layer:(i + 1) * per_layer], wt_un[i + 1:i + 2], None,
                 nks=2, nt=4)
    pack.add(PACK_HIDDEN_T0, layers[0].weight, None, wt_frag[(len(layers) - 1) * per_layer:], wt_un[0:1], None, nks=2,
             nt=2 * k0s)
    return pack, (w_frag, wt_frag, w_un, bias_acc, k0s)


def device_pack_resnet_hidden_forward(net):
    """The LDS weight image of ``fc_resnet_hidden_packed`` for a ResidualNet with hidden <= 64, <= 4 blocks, no context,
    made on the device: returns ``(pack, (w_frag, w_unscale [L], bias_acc [L, 64]))``; ``pack.run()`` refreshes it."""
    dev = net.initial_layer.weight.device
    k0s = 1 if net.initial_layer.in_features <= 32 else 2
    layers = _hidden_linears(net)
    image = _hidden_image(len(layers), k0s, dev)
    pack = DevicePack(dev)
    _add_hidden_jobs(pack, image, k0s, [(lin.weight, lin.bias, True) for lin in layers])
    return pack, image


def device_pack_affine_coupling(net, d_t, additive):
    """The LDS image of ``fc_affine_coupling_resnet``: the hidden layers of ``net`` (``device_pack_resnet_hidden_forward``)
    plus its final Linear as one more 64 x 64 layer with rows 0..31 = shift rows, rows 32..63 = scale rows.  The re-ordered
    copy of the final layer lives in a staging buffer refreshed before every pack launch.  Returns ``(pack, packed)``."""
    dev = net.initial_layer.weight.device
    k0s = 1 if net.initial_layer.in_features <= 32 else 2
    hidden_layers = _hidden_linears(net)
    image = _hidden_image(len(hidden_layers) + 1, k0s, dev)
    lin = net.final_layer
    stage_w = torch.zeros(64, 64, dtype=torch.float32, device=dev)
    stage_b = torch.zeros(64, dtype=torch.float32, device=dev)
    hf = lin.in_features

    def stage():
        with torch.no_grad():
            stage_w[:d_t, :hf].copy_(lin.weight[:d_t])
            stage_b[:d_t].copy_(lin.bias[:d_t])
            if not additive:
                stage_w[32:32 + d_t, :hf].copy_(lin.weight[d_t:2 * d_t])
                stage_b[32:32 + d_t].copy_(lin.bias[d_t:2 * d_t])

    pack = DevicePack(dev)
    _add_hidden_jobs(pack, image, k0s, [(layer.weight, layer.bias, True) for layer in hidden_layers]
                     + [(stage_w, stage_b, False)])
    pack.sources += [lin.weight, lin.bias]        # (the staging buffers' versions move only when these do)
    pack.prepare.append(stage)
    return pack, image


def device_pack_made_affine(made, features):
    """The LDS image of ``fc_affine_coupling_resnet`` for the DENSITY direction of a masked-autoregressive affine layer
    (autoregressive.py:97-129): every layer of the MADE with its mask multiplied in (staging copies, refreshed before each
    pack launch), the final masked Linear re-ordered from the interleaved [D, (u, shift)] rows to rows 0..31 = shift of dims
    0..31, rows 32..63 = u.  Returns ``(pack, packed)`` like ``device_pack_affine_coupling``."""
    dev = made.initial_layer.weight.device
    hidden_layers = _hidden_linears(made)
    n_layers = len(hidden_layers) + 1
    image = _hidden_image(n_layers, 1, dev)
    final = made.final_layer
    stage_w = [torch.zeros(64, 32 if i == 0 else 64, dtype=torch.float32, device=dev) for i in range(n_layers)]
    stage_b = [torch.zeros(64, dtype=torch.float32, device=dev) for _ in range(n_layers)]

    def stage():
        with torch.no_grad():
            for i, lin in enumerate(hidden_layers):
                stage_w[i][:lin.out_features, :lin.in_features].copy_(lin.weight * lin.mask)
                stage_b[i][:lin.out_features].copy_(lin.bias)
            w = final.weight * final.mask
            hf = final.in_features
            stage_w[-1][:features, :hf].copy_(w[1::2])            # shift rows (parameter 1 of every dim)
            stage_w[-1][32:32 + features, :hf].copy_(w[0::2])     # unconstrained-scale rows (parameter 0)
            stage_b[-1][:features].copy_(final.bias[1::2])
            stage_b[-1][32:32 + features].copy_(final.bias[0::2])

    pack = DevicePack(dev)
    _add_hidden_jobs(pack, image, 1, [(w, b, False) for w, b in zip(stage_w, stage_b)])
    for lin in hidden_layers + [final]:
        pack.sources += [lin.weight, lin.bias]
    pack.prepare.append(stage)
    return pack, image


def _made_pass_prefix(made, features, per_dim, hw):
    """Which hidden units pass d of the inverse reads, from the masks alone: the units the rows of dim d reach backwards
    through the hidden layers (and the residual identities).  Returns ``(order, need)``: ``order[rank]`` = hidden unit, sorted
    by the first pass that reads it (zero-padded units last), and ``need[d]`` = how many leading units of that order pass d
    reads -- for the reference's degrees (made.py:13-24: unit j has degree j % (D - 1) + 1) the units of degree <= d."""
    hidden = [lin for block in made.blocks for lin in block.linear_layers]
    step = torch.eye(hw, dtype=torch.bool)
    for lin in hidden:
        step |= _pad_to((lin.mask != 0).cpu(), (hw, hw))                     # [unit, the units it reads]
    reach = _pad_to((made.final_layer.mask != 0).cpu().reshape(features, per_dim, -1).any(dim=1), (features, hw))
    while True:
        wider = reach | ((reach.float() @ step.float()) > 0)
        if bool((wider == reach).all()):
            break
        reach = wider
    dims = torch.arange(features).reshape(-1, 1).expand(features, hw)
    first = torch.where(reach, dims, torch.full_like(dims, features)).amin(dim=0)      # [hw]; `features` = never read
    order = torch.argsort(first, stable=True)
    need = (first.reshape(1, -1) <= torch.arange(features).reshape(-1, 1)).sum(dim=1).to(torch.int32)
    return order, need


def pack_made_inverse(made, features, per_dim):
    """Everything ``fc_made_inverse`` needs of a residual-block MADE (hidden <= 64, <= 3 blocks, <= 64 inputs): the hidden
    stack's image on MASKED weights (rows in the accumulator order of the hidden-layer kernels, one power-of-two scale per
    layer) and the final layer as per-dim row tiles (``per_dim`` parameter rows of every dim padded to whole 16-row tiles,
    one scale per dim).  The hidden units are renumbered in the order the passes first read them (``_made_pass_prefix``:
    the same renumbering in every layer, so the residual sums stay unit-for-unit), which lets pass d compute only the
    leading 16-unit tiles / 32-unit k-steps that hold its ``units_needed[d]`` units.  Returns ``(hidden_frag,
    hidden_unscale [L], hidden_bias [L, 64], final_frag, final_unscale [D], final_bias [D, 16 PT], units_needed [D])``."""
    hw = 64
    dev = made.initial_layer.weight.device
    perm = _hb_perm().to(dev)
    k0s = 1 if features <= 32 else 2
    layers = _hidden_linears(made)
    wf, uns, biases = [], [], []
    with torch.no_grad():
        order, need = _made_pass_prefix(made, features, per_dim, hw)
        order = order.to(dev)
        # rank r sits where the accumulator layout keeps feature perm[r]: ranks 0..15 fill product tile 0, 16..31 tile 1
        # (both in k-step 0), 32..47 tile 2, 48..63 tile 3 (k-step 1)
        slot = perm
        for i, lin in enumerate(layers):
            w = _pad_to((lin.weight * lin.mask).detach().float(), (hw, 32 * k0s if i == 0 else hw))
            moved = torch.zeros_like(w)
            if i == 0:
                moved[slot] = w[order]
            else:
                moved[slot.reshape(-1, 1), slot.reshape(1, -1)] = w[order.reshape(-1, 1), order.reshape(1, -1)]
            sc, un = _pow2_scale(moved.abs().amax().reshape(1))
            uns.append(un)
            wf.append(_hidden_layer_fragments(moved * sc, perm))
            b = torch.zeros(hw, device=dev)
            b[slot] = _pad_to(lin.bias.detach().float(), (hw,))[order]
            biases.append(_bias_accumulator_order(b, perm))
        final = made.final_layer
        pt = -(-per_dim // 16)
        w = _pad_to((final.weight * final.mask).detach().float().reshape(features, per_dim, -1), (features, 16 * pt, hw))
        moved = torch.zeros_like(w)
        moved[:, :, slot] = w[:, :, order]
        w = moved
        sc, un = _pow2_scale(w.abs().amax(dim=(1, 2)))
        frag = _a_fragments((w * sc.reshape(-1, 1, 1)).reshape(features * 16 * pt, hw))           # [D PT, ks, piece, lane, 8]
        final_frag = frag.reshape(features, pt, 2, 2, 64, 8).permute(0, 2, 1, 3, 4, 5).contiguous()   # [D][ks][t][piece][lane][8]
        final_bias = _pad_to(final.bias.detach().float().reshape(features, per_dim), (features, 16 * pt)).contiguous()
    return (torch.cat(wf).contiguous(), torch.cat(uns).float().contiguous(), torch.stack(biases).contiguous(),
            final_frag, un.float().contiguous(), final_bias, need.to(dev).contiguous())


def pack_made_inverse_context(made, features, per_dim):
    """The context layers of a conditional residual-block MADE (``made.context_layer`` and every block's, made.py:153-162,
    108-118) as ``fc_made_inverse_context`` reads them: per layer the [hidden, C <= 32] weight with its rows in the unit
    order of ``pack_made_inverse`` (``_made_pass_prefix``'s ``order``: rank r is row r of the image, the row the
    accumulator layout ``_hb_perm`` keeps in slot r), zero-padded to [64, 32], one power-of-two scale per layer, two f16
    pieces in fragment order [t][piece][lane][8]; the biases in the accumulator order of ``hidden_bias``.  Returns
    ``(context_frag, context_unscale [1 + blocks], context_bias [1 + blocks, 64])``."""
    hw = 64
    layers = [made.context_layer] + [block.context_layer for block in made.blocks]
    dev = layers[0].weight.device
    wf, uns, biases = [], [], []
    with torch.no_grad():
        order, _ = _made_pass_prefix(made, features, per_dim, hw)
        order = order.to(dev)
        for lin in layers:
            if lin.in_features > 32 or lin.out_features > hw:
                raise ValueError("fc_made_inverse_context: at most 32 context features and 64 hidden units")
            w = _pad_to(lin.weight.detach().float(), (hw, 32))[order]              # row r = the unit of rank r
            sc, un = _pow2_scale(w.abs().amax().reshape(1))
            uns.append(un)
            wf.append(_hidden_layer_fragments(w * sc))                              # (one k-step)
            biases.append(_bias_accumulator_order(_pad_to(lin.bias.detach().float(), (hw,))[order]))
    return torch.cat(wf).contiguous(), torch.cat(uns).float().contiguous(), torch.stack(biases).contiguous()


def pack_resnet_hidden_backward(net):
    """Everything ``fc_resnet_hidden_backward`` needs of a ResidualNet with hidden <= 64, <= 2 ReLU blocks, no context:
    forward fragments (rows in accumulator order), fragments of the transposed weights for the W^T products, one
    power-of-two scale per layer shared by both, biases in accumulator order.  Returns
    ``(w_frag, wt_frag, w_unscale [L], bias_acc [L, 64], k0s)``."""
    hw = 64
    perm = _hb_perm().to(net.initial_layer.weight.device)
    k0 = net.initial_layer.in_features
    k0s = 1 if k0 <= 32 else 2
    layers = _hidden_linears(net)
    wf, wt, uns, biases = [], [], [], []
    scaled = []
    for i, lin in enumerate(layers):
        w = _pad_to(lin.weight.detach().float(), (hw, 32 * k0s if i == 0 else hw))
        sc, un = _pow2_scale(w.abs().amax().reshape(1))
        scaled.append(w * sc)
        uns.append(un)
        wf.append(_hidden_layer_fragments(scaled[-1], perm))
        biases.append(_bias_accumulator_order(_pad_to(lin.bias.detach().float(), (hw,)), perm))
    for w in scaled[1:]:
        wt.append(_hidden_layer_fragments(w.t().contiguous(), perm))
    wt.append(_hidden_layer_fragments(scaled[0].t().contiguous()))     # W0^T: rows natural
    return (torch.cat(wf).contiguous(), torch.cat(wt).contiguous(), torch.cat(uns).float().contiguous(),
            torch.stack(biases).contiguous(), k0s)


def pack_final_layer(weight, bias, num_bins=FUSED_BINS):
    """[d_t*23, H <= 64] weight / [d_t*23] bias of the conditioner's final Linear -> (w_pad [dp*24, 64], bias_pad
    [dp*24]): one zero row / entry appended per dim so that a dim is 24 = 6 x 4 accumulator registers, zero
    dims appended up to dp = ceil(d_t / 4) * 4 (a wave owns 4 dims), zero columns up to the kernel's 64 hidden
    units (they meet the zero activations of a zero-padded hidden stack)."""
    p = rq_param_count(num_bins, "linear")
    d_t = weight.shape[0] // p
    dp = -(-d_t // 4) * 4
    hidden = weight.shape[1]
    w = weight.detach().reshape(d_t, p, hidden)
    wpad = w.new_zeros(dp, p + 1, FUSED_HIDDEN)
    wpad[:d_t, :p, :hidden] = w
    bpad = bias.new_zeros(dp, p + 1)
    bpad[:d_t, :p] = bias.detach().reshape(d_t, p)
    return wpad.reshape(dp * (p + 1), FUSED_HIDDEN).contiguous(), bpad.reshape(-1).contiguous()


def pack_final_layer_general(weight, bias, num_bins, tails, hidden_pad):
    """The conditioner's final Linear ([d_t * P, H] weight, [d_t * P] bias, P = 3K -/+ 1) as
    ``fc_rq_spline_fused_general`` streams it: matrix-core A fragments of the power-of-two scaled weight split into
    two f16 pieces (fc_split.h), one scale per group of 4 dims --

        w_frag   f16 [groups, H/32, T, 2 (hi, lo), 64 lanes, 8]    T = ceil(P / 4) tiles of 16 rows: (dim g, param 4t + r)
        w_unscale f32 [groups]                                      2^-S of the group
        bias_pad f32 [groups, 4, 4 T]

    (zero rows / dims / columns pad P to 4 T, d_t to 4 * groups, H to ``hidden_pad``)."""
    p = rq_param_count(num_bins, tails)
    pp = -(-p // 4) * 4
    t = pp // 4
    d_t = weight.shape[0] // p
    groups = -(-d_t // 4)
    hidden = weight.shape[1]
    ks = hidden_pad // 32
    w = weight.new_zeros(groups * 4, pp, hidden_pad, dtype=torch.float32)
    w[:d_t, :p, :hidden] = weight.detach().reshape(d_t, p, hidden)
    b = bias.new_zeros(groups * 4, pp, dtype=torch.float32)
    b[:d_t, :p] = bias.detach().reshape(d_t, p)
    scale, unscale = _pow2_scale(w.reshape(groups, -1).abs().amax(dim=1))
    ws = w.reshape(groups, 4, pp, hidden_pad) * scale.reshape(groups, 1, 1, 1)
    hi = ws.to(torch.float16)
    lo = (ws - hi.float()).to(torch.float16)

    def frag(piece):
        # [G, dim 4, T, r 4, KS, gk 4, j 8] -> [G, KS, T, gk, dim, r, j] -> [G, KS, T, 64 lanes, 8]
        v = piece.reshape(groups, 4, t, 4, ks, 4, 8).permute(0, 4, 2, 5, 1, 3, 6)
        return v.reshape(groups, ks, t, 64, 8)

    w_frag = torch.stack((frag(hi), frag(lo)), dim=3).contiguous()
    return w_frag, unscale.float().contiguous(), b.reshape(groups, 4, pp).contiguous()


def pack_final_layer_transposed(weight, num_bins, tails):
    """W^T fragments of the final Linear for the backward product gh = W^T G (``fc_rq_fused_linear_backward`` role 0):
    f16 [groups, 4 hidden tiles, KK, 2 (hi, lo), 64 lanes, 8], KK = ceil(4T / 8); lane l of fragment (group, ht, kk)
    holds 2^S W[dim 4 group + (l >> 4)][param 8 kk + j][hidden 16 ht + (l & 15)] -- the k order in which a lane of the
    kernel holds its own parameter gradients.  Same per-group scale as ``pack_final_layer_general``.  hidden <= 64."""
    p = rq_param_count(num_bins, tails)
    pp = -(-p // 4) * 4
    pp8 = -(-pp // 8) * 8
    kk = pp8 // 8
    d_t = weight.shape[0] // p
    groups = -(-d_t // 4)
    hidden = weight.shape[1]
    w = weight.new_zeros(groups * 4, pp8, 64, dtype=torch.float32)
    w[:d_t, :p, :hidden] = weight.detach().reshape(d_t, p, hidden)
    sc, _ = _pow2_scale(w.reshape(groups, -1).abs().amax(dim=1))
    ws = w.reshape(groups, 4, pp8, 64) * sc.reshape(groups, 1, 1, 1)
    hi = ws.to(torch.float16)
    lo = (ws - hi.float()).to(torch.float16)

    def frag(piece):
        # [G, gk = dim 4, KK, j 8, HT 4, rho 16] -> [G, HT, KK, gk, rho, j] -> [G, HT, KK, 64 lanes, 8]
        v = piece.reshape(groups, 4, kk, 8, 4, 16).permute(0, 4, 2, 1, 5, 3)
        return v.reshape(groups, 4, kk, 64, 8)

    return torch.stack((frag(hi), frag(lo)), dim=3).contiguous()


def householder_matrix(q_vectors, reverse=False):
    """[D, D] float64 matrix M with ``householder(v, q, reverse) == v @ M`` (rows as vectors): the K reflections
    of orthogonal.py:144-171 applied to the identity.  Host-side helper for batch-independent parameters."""
    q = q_vectors.detach().double()
    if reverse:
        q = q.flip(0)
    m = torch.eye(q.shape[1], dtype=torch.float64, device=q.device)
    for i in range(q.shape[0]):
        qi = q[i]
        m = m - torch.outer(m @ qi, (2.0 / (qi @ qi)) * qi)
    return m


def pack_sylvester(q_vectors, r1, r2):
    """(W1, W2, r_diag_prod) of ``fc_sylvester_mm`` from the reference's parameters: with rows as vectors
    Q^T z = z @ Mr (reflections in reverse order) and Q v = v @ Mf, so W1 = R1 Mr^T and W2 = Mf^T R2; formed in
    float64, rounded once."""
    mr = householder_matrix(q_vectors, reverse=True)
    mf = householder_matrix(q_vectors, reverse=False)
    w1 = (r1.detach().double() @ mr.T).float().contiguous()
    w2 = (mf.T @ r2.detach().double()).float().contiguous()
    rdiag = (torch.diagonal(r1.detach()) * torch.diagonal(r2.detach())).float().contiguous()
    return w1, w2, rdiag
