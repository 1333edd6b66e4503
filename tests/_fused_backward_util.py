"""Inputs, float64 / float32 references and the per-slice comparison of the fused training kernels' tests
(``fc_rq_fused_linear_backward``: tests/test_gpu_fused_backward_grid.py groups A - C, tests/test_fused_backward_reference_host.py;
``fc_resnet_hidden_backward`` / ``_accum``: group D).  Importing it needs no GPU.

The comparison.  A gradient is cut into SLICES (``slices``): gW per transformed dim [P, 64], gb per transformed dim [P],
gh and the transformed columns of gx per row.  Per slice

    scale = max |float64|,  floor = max |float32 reference - float64|,  err = max |kernel - float64|
    scale < 1e-30:  the kernel's slice is exactly zero
    otherwise:      err <= MARGIN * floor + C * scale + cond  (+ ATOMIC * n * max |G| |h| for the float-atomic sums gW / gb)

so that a wrong contribution that is small next to the LARGEST entry of the whole gradient, but not next to its own dim or
row, fails.  MARGIN = 4 is the figure of tests/test_gpu_fused4.py.  C covers the slices at which the float32 reference
happens to be (nearly) exact.  It is taken from the float32 reference alone, never from a kernel: floor / scale over all
8 502 slices of the 45 group-A cases (``python tests/_fused_backward_util.py`` prints it) has

    median 1.36e-6   (90 %: 6.3e-6, max: 8.4e-4)

and C is that median rounded up to one significant digit, C = 2e-6 (a hundredth of the 2e-4 that
tests/test_gpu_fused_backward.py grants relative to the whole tensor).  ATOMIC = 1e-7 per summed term is the figure of
tools/probe/fuzz_backward.py: the absolute error of a cancelling float32 sum does not shrink with the sum.

cond (``conditioning``) is the derived part of the bound.  MARGIN * floor + C * scale alone fails on the GPU at single
rows and dims (err / floor up to 97): always a row with large h whose element sits in a narrow bin, where the gradient
is so sensitive to the parameter rows that ONE float32 run is no measure of float32 arithmetic -- the float32 reference
itself moves by 90 times its own floor there when its inputs move by one ulp.  The kernel recomputes the parameter rows
from two-piece f16 operands that share one power-of-two scale per row of h and per group of four dims of W; cond is the
response of the float64 gradient to exactly that residual, so it is stated in terms of the quantities the scales are
shared over, and it is negligible (median 1e-6 .. 2e-5 of the slice's scale) wherever the element is well conditioned.

Rows holding an element within 2^-18 (right - left) of an interior knot (``near_knot``) are left out of the per-row gx / gh
comparison only: d logabsdet / d params jumps there and float32 and float64 may take different sides.  The seeds
(``SEED_BUMP``) are chosen so that no row of a small case is flagged and at most 0.5 % of the rows of a multi-tile case; the
host test asserts both."""
import collections
import copy

import torch

from oracle import torch_oracle as O

HIDDEN = 64
WH_DIVISOR = 8.0
TAIL_BOUND = 3.0
MARGIN = 4.0
C = 2e-6
ATOMIC = 1e-7
ZERO_SCALE = 1e-30
KNOT_WINDOW = 2.0 ** -18
CUS_MI355X = 256

INSTANCES = [(k, "linear") for k in range(4, 12)] + [(k, None) for k in range(4, 11)]      # launch_backward512_any
SHAPES = [(24, 11, 64), (63, 18, 96), (128, 32, 64)]
EDGE_INSTANCES = [(8, "linear"), (9, None), (11, "linear")]       # T = 6 resident fragments; T = 7 ring; P = PP = 32
EDGES = ["gl_none", "all_zero", "gy_zero", "gl_zero", "padded", "outside", "on_edge", "h_edges", "w_zero", "w_mixed"]
MULTI = ["ascending", "descending", "onehot_first", "onehot_last"]
ON_EDGE_ROWS = (5, 6)
H_ZERO_ROW, H_TINY_ROWS, H_HUGE_ROWS = 7, slice(8, 12), slice(12, 16)
MIXED_DIM = 1

Case = collections.namedtuple("Case", "k tails d d_t n edge x h w b cols gy gl")
Reference = collections.namedtuple("Reference", "gx gh gw gb g rows")


def tails_name(tails):
    return "linear" if tails == "linear" else "box"


def param_count(k, tails):
    return 3 * k - 1 if tails == "linear" else 3 * k + 1


def case_id(k, tails, d, d_t, n, edge=None):
    return "K%d-%s-d%d-dt%d-n%d%s" % (k, tails_name(tails), d, d_t, n, "" if edge is None else "-" + edge)


def multi_rows(cus=CUS_MI355X):
    """Rows of a group-C batch: workgroup 0 walks the tiles 0, cus and 2 cus, most workgroups two."""
    return (2 * cus + 1) * 32


def grid_cases(cus=CUS_MI355X):
    """Every case of the GPU file as (group, k, tails, d, d_t, n, edge)."""
    out = [("A", k, tails, d, d_t, n, None) for (k, tails) in INSTANCES for (d, d_t, n) in SHAPES]
    for (k, tails) in EDGE_INSTANCES:
        out += [("B", k, tails, 24, 11, 64, e) for e in EDGES if not (e == "outside" and tails is None)]
        out += [("C", k, tails, 64, 32, multi_rows(cus), e) for e in MULTI]
    return out


# seed = 7 K + d + 1000 * bump: the first bump at which the near-knot conditions hold (test_fused_backward_reference_host.py)
SEED_BUMP = {"K5-box-d128-dt32-n64": 1, "K8-box-d128-dt32-n64": 1, "K10-box-d24-dt11-n64": 1}


def seed_of(k, tails, d, d_t, n, edge=None):
    return 7 * k + d + 1000 * SEED_BUMP.get(case_id(k, tails, d, d_t, n, edge), 0)


def case(k, tails, d, d_t, n, seed=None, edge=None):
    """x [n, d], h [n, 64], W [d_t P, 64], b [d_t P], cols (sorted random subset of the columns), gy [n, d], gl [n]: the
    recipe of test_fused_linear_backward_operator_vs_float64_autograd (rows of h over three decades, two rows outside the
    tails), then the ``edge`` variant."""
    gen = torch.Generator().manual_seed(seed_of(k, tails, d, d_t, n, edge) if seed is None else seed)
    p = param_count(k, tails)
    x = torch.rand(n, d, generator=gen) if tails is None else torch.randn(n, d, generator=gen) * 1.5
    if tails == "linear" and n >= 8:
        x[3], x[4] = 4.0, -3.5
    h = torch.relu(torch.randn(n, HIDDEN, generator=gen)) * 1.5 + torch.randn(n, HIDDEN, generator=gen) * 0.2
    if edge != "h_edges":
        h *= torch.logspace(-2, 1, n).unsqueeze(1)
    w = torch.randn(d_t * p, HIDDEN, generator=gen) * (1.0 / HIDDEN ** 0.5)
    b = torch.randn(d_t * p, generator=gen) * 0.3
    cols = torch.randperm(d, generator=gen)[:d_t].sort().values.to(torch.int32)
    gy = torch.randn(n, d, generator=gen)
    gl = torch.randn(n, generator=gen)
    tc = cols.long()
    if edge in ("all_zero", "gy_zero"):
        gy.zero_()
    if edge in ("all_zero", "gl_zero"):
        gl.zero_()
    if edge == "gl_none":
        gl = None
    elif edge == "padded":              # the module's padding to 128 rows: zero rows with a zero upstream gradient
        x[n - 32:] = 0.0
        gy[n - 32:] = 0.0
        gl[n - 32:] = 0.0
    elif edge == "outside":
        x = torch.where(torch.rand(n, d, generator=gen) < 0.5, torch.tensor(4.0), torch.tensor(-4.0))
    elif edge == "on_edge":
        lo, hi = (-TAIL_BOUND, TAIL_BOUND) if tails == "linear" else (0.0, 1.0)
        x[ON_EDGE_ROWS[0], tc] = hi
        x[ON_EDGE_ROWS[1], tc] = lo
        gl[list(ON_EDGE_ROWS)] = 0.0
    elif edge == "h_edges":
        h[H_ZERO_ROW] = 0.0
        h[H_TINY_ROWS] *= 1e-20
        h[H_HUGE_ROWS] *= 1e4
    elif edge == "w_zero":
        w.zero_()
    elif edge == "w_mixed":             # one dim of a group of four at 1e-4 of its neighbours
        w[MIXED_DIM * p:(MIXED_DIM + 1) * p] *= 1e-4
    elif edge in ("ascending", "descending"):
        s = torch.logspace(-6, 3, n)
        s = s if edge == "ascending" else s.flip(0)
        gy *= s.unsqueeze(1)
        gl *= s
    elif edge in ("onehot_first", "onehot_last"):
        keep = onehot_rows(n, edge)
        mask = torch.zeros(n)
        mask[keep] = 1.0
        gy *= mask.unsqueeze(1)
        gl *= mask
    elif edge is not None and edge not in EDGES:
        raise ValueError(edge)
    return Case(k, tails, d, d_t, n, edge, x, h, w, b, cols, gy, gl)


def onehot_rows(n, edge):
    """The 32 rows that carry the upstream gradient: tile 0, or the last tile (2 cus when n = (2 cus + 1) 32)."""
    return slice(0, 32) if edge == "onehot_first" else slice(n - 32, n)


def take_rows(cs, rows):
    """The sub-batch of ``rows`` (same weights)."""
    x, h, gy = cs.x[rows], cs.h[rows], cs.gy[rows]
    return cs._replace(n=x.shape[0], x=x, h=h, gy=gy, gl=None if cs.gl is None else cs.gl[rows])


def forward(cs, x, h, w, b):
    """(y [n, d], logabsdet per element [n, d_t], parameter rows [n, d_t, P]) of Linear + ``O.rq_from_rows`` in the dtype of
    its arguments."""
    n, p = x.shape[0], param_count(cs.k, cs.tails)
    tc = cs.cols.long()
    rows = (h @ w.T + b).view(n, cs.d_t, p)
    out, lad_e = O.rq_from_rows(x[:, tc], rows.clone(), cs.k, cs.tails, TAIL_BOUND, False, wh_divisor=WH_DIVISOR)
    return x.clone().index_copy(1, tc, out), lad_e, rows


def loss(cs, x, h, w, b):
    y, lad_e, rows = forward(cs, x, h, w, b)
    total = (y * cs.gy.to(x.dtype)).sum()
    if cs.gl is not None:
        total = total + (lad_e.sum(dim=1) * cs.gl.to(x.dtype)).sum()
    return total, rows


def reference(cs, dtype, full=False):
    """(gx, gh, gW, gb) by torch autograd on the CPU in ``dtype``; ``full``: a Reference that also carries G = dL / d rows
    [n, d_t, P] and the parameter rows."""
    x, h, w, b = (t.to(dtype).requires_grad_(True) for t in (cs.x, cs.h, cs.w, cs.b))
    total, rows = loss(cs, x, h, w, b)
    leaves = (x, h, w, b, rows)
    got = torch.autograd.grad(total, leaves, allow_unused=True)       # (a batch wholly outside the tails uses no parameter)
    gx, gh, gw, gb, g = (torch.zeros_like(t) if v is None else v for t, v in zip(leaves, got))
    return Reference(gx, gh, gw, gb, g, rows.detach()) if full else (gx, gh, gw, gb)


def conditioning(cs, r64, trials=3):
    """Per slice, how far the FLOAT64 gradient moves when the inputs move by what the kernel's documented arithmetic
    (fc_split.h, include/flowcon_hip.h) does to them before the first product:

        h   each entry by +-2^-22 of the largest |h| of its ROW         (two f16 pieces under one power-of-two scale per row)
        W   each entry by +-2^-22 of the largest |W| of its GROUP of four dims          (one scale per group of four dims)
        x   each transformed entry by +-sqrt(K) 2^-24 (right - left)
            (x - knot in float32: a knot is a cumulative sum of up to K widths, one rounding of the interval's size each,
            adding up like a random walk; the float32 REFERENCE's own knots are 3e-7 .. 7e-7 = 2 .. 4 such roundings
            off in the late bins of K = 9 and 11)

    with random signs, the largest change over ``trials`` draws: {kind: [slices]}.  A single float32 reference can sit
    two orders of magnitude below this at an element whose bin is narrow (its roundings cancel by chance); float32
    arithmetic as such cannot."""
    p = param_count(cs.k, cs.tails)
    gen = torch.Generator().manual_seed(cs.n + cs.d)
    groups = -(-cs.d_t // 4)
    wpad = torch.zeros(groups * 4, p * HIDDEN, dtype=torch.float64)
    wpad[:cs.d_t] = cs.w.double().reshape(cs.d_t, -1)
    wmax = wpad.reshape(groups, -1).abs().amax(dim=1).repeat_interleave(4)[:cs.d_t].repeat_interleave(p).unsqueeze(1)
    hmax = cs.h.double().abs().amax(dim=1, keepdim=True)
    step = (2 * TAIL_BOUND if cs.tails == "linear" else 1.0) * cs.k ** 0.5 * 2.0 ** -24
    tmask = torch.zeros(cs.d, dtype=torch.float64)
    tmask[cs.cols.long()] = 1.0
    base = dict(zip(("gx", "gh", "gw", "gb"), r64[:4]))
    worst = {kind: torch.zeros(slices(kind, t, cs).shape[0], dtype=torch.float64) for kind, t in base.items()}

    def sign(t):
        return torch.randint(0, 2, t.shape, generator=gen).double() * 2 - 1

    for _ in range(trials):
        xm = cs.x.double() + sign(cs.x) * step * tmask
        moved = cs._replace(x=xm.clamp(0.0, 1.0) if cs.tails is None else xm,          # (the box has no outside)
                            h=cs.h.double() + sign(cs.h) * 2.0 ** -22 * hmax,
                            w=cs.w.double() + sign(cs.w) * 2.0 ** -22 * wmax)
        for kind, t in zip(("gx", "gh", "gw", "gb"), reference(moved, torch.float64)):
            worst[kind] = torch.maximum(worst[kind], (slices(kind, t, cs) - slices(kind, base[kind], cs)).abs().amax(dim=1))
    return worst


def near_knot(cs, rows64):
    """bool [n, d_t]: transformed elements within 2^-18 (right - left) of an interior knot of their float64 spline."""
    lo, hi = (-TAIL_BOUND, TAIL_BOUND) if cs.tails == "linear" else (0.0, 1.0)
    knots, _ = O._knots(rows64[..., :cs.k].double() / WH_DIVISOR, lo, hi, 1e-3, cs.k)
    xt = cs.x[:, cs.cols.long()].double().unsqueeze(-1)
    return ((xt - knots[..., 1:-1]).abs() <= KNOT_WINDOW * (hi - lo)).any(dim=-1)


def slices(kind, t, cs):
    """``t`` as [slices, entries]: the norms of the comparison."""
    p = param_count(cs.k, cs.tails)
    t = t.detach().double().cpu()
    if kind == "gw":
        return t.reshape(cs.d_t, p * HIDDEN)
    if kind == "gb":
        return t.reshape(cs.d_t, p)
    if kind == "gh":
        return t.reshape(-1, HIDDEN)
    if kind == "gx":
        return t[:, cs.cols.long()]
    raise ValueError(kind)


def identity_columns(cs):
    taken = set(cs.cols.tolist())
    return [c for c in range(cs.d) if c not in taken]


def atomic_term(kind, cs, ref):
    """Per dim: n * max over the slice of the float64 per-sample term |G| |h| (|G| for the bias)."""
    g = ref.g.abs().amax(dim=2)                                         # [n, d_t]
    if kind == "gw":
        g = g * cs.h.double().abs().amax(dim=1, keepdim=True)
    return cs.n * g.amax(dim=0)


Result = collections.namedtuple("Result", "ok worst worst_floor where detail")


def compare(got, ref64, ref32, c=C, extra=None, keep=None, margin=MARGIN, cond=None):
    """Per-slice comparison of [slices, entries] tensors: ``ok``, the worst err / bound, the worst err / floor (over the
    slices with a floor above 1e-3 C scale), the worst slice and a line that says so."""
    got, ref64, ref32 = (t.detach().double().cpu() for t in (got, ref64, ref32))
    scale = ref64.abs().amax(dim=1)
    floor = (ref32 - ref64).abs().amax(dim=1)
    err = (got - ref64).abs().amax(dim=1)
    finite = bool(torch.isfinite(got).all())
    bound = margin * floor + c * scale + (0.0 if extra is None else ATOMIC * extra) + (0.0 if cond is None else cond)
    zero = scale < ZERO_SCALE
    bad = torch.where(zero, got.abs().amax(dim=1) != 0, err > bound)
    if keep is not None:
        bad &= keep
    ratio = torch.where(zero, torch.zeros_like(err), err / bound.clamp_min(1e-300))
    rfloor = torch.where(zero | (floor <= 1e-3 * c * scale), torch.zeros_like(err), err / floor.clamp_min(1e-300))
    if keep is not None:
        ratio, rfloor = ratio * keep, rfloor * keep
    if ratio.numel() == 0:
        return Result(finite, 0.0, 0.0, -1, "empty")
    i = int(ratio.argmax()) if not bool(bad.any()) else int(bad.float().argmax())
    detail = "slice %d: err %.3g, floor %.3g, scale %.3g, bound %.3g; %d of %d slices fail" % (
        i, err[i], floor[i], scale[i], bound[i], int(bad.sum()), bad.numel())
    return Result(finite and not bool(bad.any()), float(ratio.max()), float(rfloor.max()), i, detail)


# ---- fc_resnet_hidden_backward (group D) ---------------------------------------------------------------------------------

HIDDEN_SHAPES = [(64, 32, 2, 64, 128), (64, 64, 2, 128, 256), (64, 33, 1, 70, 128), (64, 1, 0, 5, 128), (20, 7, 2, 15, 384)]
ACCUM_CASES = [("parity0", 32, 64), ("parity1", 32, 64), ("parity0", 64, 128), ("parity1", 64, 128),
               ("half", 32, 64), ("random", 32, 64), ("random", 33, 70)]


def hidden_ids(kind, in_f, d, gen):
    if kind == "parity0":
        return torch.arange(0, 2 * in_f, 2)
    if kind == "parity1":
        return torch.arange(1, 2 * in_f, 2)
    if kind == "half":
        return torch.arange(in_f)
    return torch.randperm(d, generator=gen)[:in_f].sort().values


def hidden_case(hidden, in_f, blocks, d, n, ids="random"):
    """(net, id columns, x [n, d], gh [n, 64]) as test_hidden_backward_kernel_vs_float64_autograd draws them."""
    from flowconductor_amd.nn import nets

    torch.manual_seed(hidden + in_f + blocks)
    net = nets.ResidualNet(in_f, 8, hidden_features=hidden, num_blocks=blocks)
    with torch.no_grad():
        for prm in net.parameters():
            prm.mul_(2.0)
    gen = torch.Generator().manual_seed(hidden + in_f + blocks + d)
    idc = hidden_ids(ids, in_f, d, gen)
    x = torch.randn(n, d, generator=gen) * torch.logspace(-1, 0.5, n).unsqueeze(1)
    gh = torch.randn(n, 64, generator=gen) * torch.logspace(-2, 1, n).flip(0).unsqueeze(1)
    gh[:, hidden:] = 0
    return net, idc, x, gh


def hidden_reference(net, idc, x, gh, dtype):
    """[gxid, gW0, gb0, gW of block linear 0, its gb, ...] by autograd through the same nn.Module in ``dtype``."""
    hidden = net.initial_layer.out_features
    net = copy.deepcopy(net).to(dtype)
    xid = x[:, idc].to(dtype).requires_grad_(True)
    params = [net.initial_layer.weight, net.initial_layer.bias] + [p for b in net.blocks for l in b.linear_layers
                                                                   for p in (l.weight, l.bias)]
    return torch.autograd.grad(net.hidden(xid), [xid] + params, gh[:, :hidden].to(dtype))


def _measure_c():
    """floor / scale of the float32 reference over every slice of every group-A case."""
    ratios = []
    for (_, k, tails, d, d_t, n, edge) in grid_cases():
        if edge is not None:
            continue
        cs = case(k, tails, d, d_t, n)
        r64, r32 = reference(cs, torch.float64), reference(cs, torch.float32)
        for kind, a, b in zip(("gx", "gh", "gw", "gb"), r64, r32):
            a, b = slices(kind, a, cs), slices(kind, b, cs)
            scale = a.abs().amax(dim=1)
            ratios.append(((b - a).abs().amax(dim=1) / scale)[scale >= ZERO_SCALE])
    r = torch.cat(ratios)
    print("floor / scale over %d slices: median %.3g, 90 %% %.3g, max %.3g" % (r.numel(), r.median(), r.quantile(0.9), r.max()))


if __name__ == "__main__":
    _measure_c()
