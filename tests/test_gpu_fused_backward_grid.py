"""The two backward kernels of a training step against float64 autograd, slice by slice (tests/_fused_backward_util.py):

A  ``fc_rq_fused_linear_backward`` at every ``<K, tails>`` instantiation of ``rq_fused_backward512_kernel`` (K = 4..11 with
   linear tails, 4..10 in the box) at three small shapes: an idle wave and a partly filled dim group, a second sweep with
   one group of two dims, both sweeps full with D > 64;
B  the edges the kernel branches on (no grad_logabsdet, zero upstream gradients, the module's zero padding rows, a batch
   outside the tails, rows on the ends of the interval, zero / tiny / huge rows of h, W = 0, mixed scales of W in one group);
C  several tiles per workgroup with upstream gradients over nine decades, rising and falling, and with one live tile;
D  ``fc_resnet_hidden_backward`` and ``fc_resnet_hidden_backward_accum`` at operator level, both parities of the 16-byte
   read-modify-write of the accumulating entry.

Every check prints its figures (``pytest -s``) before it asserts: the worst err / bound and the worst err / floor."""
import pytest
import torch

import _fused_backward_util as U
from flowconductor_amd import ops

pytestmark = pytest.mark.gpu

KINDS = ("gx", "gh", "gw", "gb")


def _launch(cs, device, gl="case"):
    packed = ops.pack_final_layer_general(cs.w.to(device), cs.b.to(device), cs.k, cs.tails, 64)
    packed_t = ops.pack_final_layer_transposed(cs.w.to(device), cs.k, cs.tails)
    gl = cs.gl if gl == "case" else gl
    out = ops.rq_fused_linear_backward(cs.x.to(device), cs.h.to(device), cs.gy.to(device), None if gl is None else gl.to(device),
                                       packed, packed_t, cs.cols.to(device), num_bins=cs.k, tails=cs.tails,
                                       tail_bound=U.TAIL_BOUND, wh_divisor=U.WH_DIVISOR)
    return tuple(t.cpu() for t in out)


def _references(cs):
    return U.reference(cs, torch.float64, full=True), U.reference(cs, torch.float32, full=True)


def _check(tag, cs, got, r64, r32, kinds=KINDS, rows=None, trials=3):
    """The per-slice comparison of ``kinds``; ``rows``: bool [n], the rows of gx / gh that take part (default: all but the
    rows ``near_knot`` flags).  The identity columns of gx are gy bit for bit.  Returns the conditioning terms."""
    flagged = U.near_knot(cs, r64.rows).any(dim=1)
    cond = U.conditioning(cs, r64, trials)
    keep = ~flagged if rows is None else rows & ~flagged
    failures = []
    for kind in kinds:
        i = KINDS.index(kind)
        extra = U.atomic_term(kind, cs, r64) if kind in ("gw", "gb") else None
        res = U.compare(U.slices(kind, got[i], cs), U.slices(kind, r64[i], cs), U.slices(kind, r32[i], cs), extra=extra,
                        keep=keep if kind in ("gx", "gh") else None, cond=cond[kind])
        print("fused-backward-grid %s %s: err/bound %.3f err/floor %.2f (%s)" % (tag, kind, res.worst, res.worst_floor, res.detail))
        if not res.ok:
            failures.append((kind, res.detail))
    assert not failures, (tag, failures)
    if "gx" in kinds:
        ident = U.identity_columns(cs)
        assert torch.equal(got[0][:, ident], cs.gy[:, ident]), tag
    return cond


# ---- A: every instantiation ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("d,d_t,n", U.SHAPES, ids=["d%d-dt%d-n%d" % s for s in U.SHAPES])
@pytest.mark.parametrize("k,tails", U.INSTANCES, ids=["K%d-%s" % (k, U.tails_name(t)) for k, t in U.INSTANCES])
def test_every_instantiation_per_slice(k, tails, d, d_t, n, device):
    cs = U.case(k, tails, d, d_t, n)
    r64, r32 = _references(cs)
    _check("A " + U.case_id(k, tails, d, d_t, n), cs, _launch(cs, device), r64, r32)


@pytest.mark.parametrize("k,tails", [(12, "linear"), (11, None)], ids=["K12-linear", "K11-box"])
def test_more_than_32_parameters_per_dim_raise(k, tails, device):
    """The dispatcher's ``default:`` cases (P = 35 and 34): an error, not another kernel."""
    cs = U.case(k, tails, 24, 11, 64)
    with pytest.raises(RuntimeError, match="fc_rq_fused_linear_backward"):
        _launch(cs, device)


# ---- B: edges --------------------------------------------------------------------------------------------------------------

_EDGE_IDS = ["K%d-%s" % (k, U.tails_name(t)) for k, t in U.EDGE_INSTANCES]
_LINEAR_IDS = [i for i, (_, t) in zip(_EDGE_IDS, U.EDGE_INSTANCES) if t == "linear"]
_SMALL = (24, 11, 64)


def _edge(k, tails, edge):
    return U.case(k, tails, *_SMALL, edge=edge), "B " + U.case_id(k, tails, *_SMALL, edge)


@pytest.mark.parametrize("k,tails", U.EDGE_INSTANCES, ids=_EDGE_IDS)
def test_without_grad_logabsdet(k, tails, device):
    cs, tag = _edge(k, tails, "gl_none")
    assert cs.gl is None
    r64, r32 = _references(cs)
    _check(tag, cs, _launch(cs, device), r64, r32)


@pytest.mark.parametrize("k,tails", U.EDGE_INSTANCES, ids=_EDGE_IDS)
def test_zero_upstream_gradient_gives_exact_zeros(k, tails, device):
    cs, _ = _edge(k, tails, "all_zero")
    for t in _launch(cs, device):
        assert bool(torch.isfinite(t).all()) and float(t.abs().max()) == 0.0


@pytest.mark.parametrize("edge", ["gy_zero", "gl_zero"])
@pytest.mark.parametrize("k,tails", U.EDGE_INSTANCES, ids=_EDGE_IDS)
def test_one_zero_upstream_gradient(k, tails, edge, device):
    cs, tag = _edge(k, tails, edge)
    r64, r32 = _references(cs)
    _check(tag, cs, _launch(cs, device), r64, r32)


@pytest.mark.parametrize("k,tails", U.EDGE_INSTANCES, ids=_EDGE_IDS)
def test_padding_rows_add_nothing(k, tails, device):
    """The last tile as the module pads a batch (_FusedRQCouplingFunction.forward): x = 0, no upstream gradient.  Zero-gradient
    rows in the same workgroup as live ones: exact zeros on them, gW / gb those of the un-padded batch."""
    cs, tag = _edge(k, tails, "padded")
    got = _launch(cs, device)
    live = cs.n - 32
    assert float(got[0][live:][:, cs.cols.long()].abs().max()) == 0.0 and float(got[1][live:].abs().max()) == 0.0
    r64, r32 = _references(cs)
    _check(tag, cs, got, r64, r32)
    short = U.take_rows(cs, slice(0, live))
    s64, s32 = _references(short)
    _check(tag + " un-padded", short, (got[0][:live], got[1][:live], got[2], got[3]), s64, s32)


@pytest.mark.parametrize("k,tails", [kt for kt in U.EDGE_INSTANCES if kt[1] == "linear"], ids=_LINEAR_IDS)
def test_batch_outside_the_tails_is_the_identity(k, tails, device):
    cs, _ = _edge(k, tails, "outside")
    gx, gh, gw, gb = _launch(cs, device)
    assert torch.equal(gx, cs.gy)
    for t in (gh, gw, gb):
        assert bool(torch.isfinite(t).all()) and float(t.abs().max()) == 0.0


@pytest.mark.parametrize("k,tails", U.EDGE_INSTANCES, ids=_EDGE_IDS)
def test_rows_on_the_ends_of_the_interval(k, tails, device):
    """Rows exactly on +-tail_bound / on 0.0 and 1.0 with gl = 0 (test_float64_reference_on_the_ends_of_the_interval: they add
    nothing to gW / gb / gh; gx = gy with linear tails, gy times the free end derivative in the box -- the float64 gx)."""
    cs, tag = _edge(k, tails, "on_edge")
    got = _launch(cs, device)
    r64, r32 = _references(cs)
    rows, tc = list(U.ON_EDGE_ROWS), cs.cols.long()
    rest = torch.ones(cs.n, dtype=torch.bool)
    rest[rows] = False
    cond = _check(tag, cs, got, r64, r32, rows=rest)
    want = cs.gy.double() if tails == "linear" else r64.gx
    for r in rows:
        err = float((got[0][r, tc].double() - want[r, tc]).abs().max())
        floor = float((r32.gx[r, tc].double() - r64.gx[r, tc]).abs().max())
        scale = float(r64.gx[r, tc].abs().max())
        # the float64 gh of such a row is rounding noise around zero: it has no scale of its own, the batch's stands in
        gh_err = float((got[1][r].double() - r64.gh[r]).abs().max())
        gh_floor = float((r32.gh[r].double() - r64.gh[r]).abs().max())
        print("fused-backward-grid %s row %d: gx err %.3g floor %.3g scale %.3g; gh err %.3g floor %.3g" % (
            tag, r, err, floor, scale, gh_err, gh_floor))
        assert err <= U.MARGIN * floor + U.C * scale + float(cond["gx"][r]), (tag, r, err, floor, scale)
        assert gh_err <= U.MARGIN * gh_floor + U.C * float(r64.gh.abs().max()) + float(cond["gh"][r]), (tag, r, gh_err, gh_floor)


@pytest.mark.parametrize("k,tails", U.EDGE_INSTANCES, ids=_EDGE_IDS)
def test_zero_tiny_and_huge_rows_of_h(k, tails, device):
    cs, tag = _edge(k, tails, "h_edges")
    got = _launch(cs, device)
    for t in got:
        assert bool(torch.isfinite(t).all())
    r64, r32 = _references(cs)
    _check(tag, cs, got, r64, r32)


@pytest.mark.parametrize("k,tails", U.EDGE_INSTANCES, ids=_EDGE_IDS)
def test_zero_final_weight(k, tails, device):
    cs, tag = _edge(k, tails, "w_zero")
    got = _launch(cs, device)
    assert float(got[1].abs().max()) == 0.0
    r64, r32 = _references(cs)
    _check(tag, cs, got, r64, r32)


@pytest.mark.parametrize("k,tails", U.EDGE_INSTANCES, ids=_EDGE_IDS)
def test_mixed_weight_scales_in_one_dim_group(k, tails, device):
    """One dim's rows of W at 1e-4 of its three neighbours', which share its power-of-two scale.  gh and gx are sums over
    the dims, so they are compared per row as everywhere; gW / gb per dim."""
    cs, tag = _edge(k, tails, "w_mixed")
    r64, r32 = _references(cs)
    _check(tag, cs, _launch(cs, device), r64, r32)


# ---- C: several tiles per workgroup ------------------------------------------------------------------------------------------

def _cus(device):
    return torch.cuda.get_device_properties(device).multi_processor_count


@pytest.mark.parametrize("edge", ["ascending", "descending"])
@pytest.mark.parametrize("k,tails", U.EDGE_INSTANCES, ids=_EDGE_IDS)
def test_upstream_gradients_over_nine_decades(k, tails, edge, device):
    """n = (2 CUs + 1) 32 rows: workgroup 0 walks the tiles 0, CUs and 2 CUs.  Rising gradients lower the running shift of the
    gW accumulators on every later tile (the rescale through LDS), falling ones leave it where the first tile put it."""
    cus = _cus(device)
    n = U.multi_rows(cus)
    cs = U.case(k, tails, 64, 32, n, edge=edge)
    r64, r32 = _references(cs)
    rows = torch.zeros(n, dtype=torch.bool)
    rows[::61] = True
    for t in (0, cus, 2 * cus):
        rows[32 * t:32 * t + 32] = True
    _check("C " + U.case_id(k, tails, 64, 32, n, edge), cs, _launch(cs, device), r64, r32, rows=rows, trials=2)


@pytest.mark.parametrize("edge", ["onehot_first", "onehot_last"])
@pytest.mark.parametrize("k,tails", U.EDGE_INSTANCES, ids=_EDGE_IDS)
def test_one_live_tile_among_zero_gradient_tiles(k, tails, edge, device):
    """Only tile 0, or only tile 2 CUs (the third of workgroup 0), has an upstream gradient: gW / gb are the float64 gradient
    of those 32 rows alone, every other row of gh and of gx's transformed columns is exactly zero."""
    n = U.multi_rows(_cus(device))
    cs = U.case(k, tails, 64, 32, n, edge=edge)
    gx, gh, gw, gb = _launch(cs, device)
    live = U.onehot_rows(n, edge)
    dead = torch.ones(n, dtype=torch.bool)
    dead[live] = False
    assert float(gx[dead][:, cs.cols.long()].abs().max()) == 0.0 and float(gh[dead].abs().max()) == 0.0
    ident = U.identity_columns(cs)
    assert torch.equal(gx[:, ident], cs.gy[:, ident])
    tile = U.take_rows(cs, live)
    t64, t32 = _references(tile)
    _check("C " + U.case_id(k, tails, 64, 32, n, edge), tile, (gx[live], gh[live], gw, gb), t64, t32)


# ---- D: the hidden stack's backward --------------------------------------------------------------------------------------------

def _hidden_slices(hidden, blocks, gxid, gw0, gwb, gb):
    """[(name, [slices, entries])]: gxid per row, weight gradients per output unit, bias gradients per layer."""
    out = [("gxid", gxid), ("gw0", gw0[:hidden])]
    out += [("gwb%d" % i, gwb[i, :hidden, :hidden]) for i in range(2 * blocks)]
    out.append(("gb", gb[:, :hidden]))
    return out


def _hidden_reference_slices(ref):
    out = [("gxid", ref[0]), ("gw0", ref[1])]
    out += [("gwb%d" % i, ref[3 + 2 * i]) for i in range((len(ref) - 3) // 2)]
    out.append(("gb", torch.stack([ref[2]] + [ref[4 + 2 * i] for i in range((len(ref) - 3) // 2)])))
    return out


def _hidden_check(tag, hidden, blocks, got, r64, r32, skip=()):
    failures = []
    for (name, g), (_, a), (_, b) in zip(_hidden_slices(hidden, blocks, *got), _hidden_reference_slices(r64),
                                         _hidden_reference_slices(r32)):
        if name in skip:
            continue
        res = U.compare(g, a, b)
        print("fused-backward-grid %s %s: err/bound %.3f err/floor %.2f (%s)" % (tag, name, res.worst, res.worst_floor, res.detail))
        if not res.ok:
            failures.append((name, res.detail))
    assert not failures, (tag, failures)


@pytest.mark.parametrize("hidden,in_f,blocks,d,n", U.HIDDEN_SHAPES,
                         ids=["hidden%d-in%d-blocks%d-d%d-n%d" % s for s in U.HIDDEN_SHAPES])
def test_hidden_backward_per_slice(hidden, in_f, blocks, d, n, device):
    net, ids, x, gh = U.hidden_case(hidden, in_f, blocks, d, n)
    r64, r32 = U.hidden_reference(net, ids, x, gh, torch.float64), U.hidden_reference(net, ids, x, gh, torch.float32)
    netd = net.to(device)
    assert netd.hip_hidden_backward_supported()
    got = ops.resnet_hidden_backward(x.to(device), gh.to(device), ids.to(device), netd.hidden_backward_packed(), in_f, blocks)
    got = tuple(t.cpu() for t in got)
    _hidden_check("D hidden%d-in%d-blocks%d-d%d-n%d" % (hidden, in_f, blocks, d, n), hidden, blocks, got, r64, r32)
    if hidden < 64:      # zero-padded units: no gradient leaks into them
        assert float(got[1][hidden:].abs().max()) == 0.0 and float(got[3][:, hidden:].abs().max()) == 0.0


@pytest.mark.parametrize("ids_kind,in_f,d", U.ACCUM_CASES, ids=["%s-in%d-d%d" % a for a in U.ACCUM_CASES])
def test_hidden_backward_accumulates_into_the_identity_columns_only(ids_kind, in_f, d, device):
    """``grad_inputs_accum`` pre-filled with random values: afterwards the identity columns hold prefill + gxid of the plain
    entry (one float32 rounding of the sum, on top of the rounding gxid itself carries: the kernel adds the unrounded
    product), every other column its prefill bit for bit.  parity0 / parity1: identity columns 2 j / 2 j + 1 with
    D = 2 in_features, the 16-byte read-modify-write; the others take the scalar one."""
    hidden, blocks, n = 64, (1 if in_f == 33 else 2), (256 if d == 128 else 128)
    net, ids, x, gh = U.hidden_case(hidden, in_f, blocks, d, n, ids=ids_kind)
    r64, r32 = U.hidden_reference(net, ids, x, gh, torch.float64), U.hidden_reference(net, ids, x, gh, torch.float32)
    netd = net.to(device)
    packed = netd.hidden_backward_packed()
    args = (x.to(device), gh.to(device), ids.to(device), packed, in_f, blocks)
    plain = tuple(t.cpu() for t in ops.resnet_hidden_backward(*args))
    prefill = torch.randn(n, d, generator=torch.Generator().manual_seed(in_f + d))
    acc = prefill.to(device).clone()
    none, gw0, gwb, gb = ops.resnet_hidden_backward(*args, grad_inputs_accum=acc)
    assert none is None
    acc = acc.cpu()
    other = [c for c in range(d) if c not in set(ids.tolist())]
    assert torch.equal(acc[:, other], prefill[:, other])
    want = prefill[:, ids].double() + plain[0].double()
    slack = 2.0 ** -24 * (acc[:, ids].double().abs() + plain[0].double().abs())
    assert bool(((acc[:, ids].double() - want).abs() <= slack).all())
    tag = "D accum %s-in%d-d%d" % (ids_kind, in_f, d)
    same = all(torch.equal(a.cpu(), b) for a, b in zip((gw0, gwb, gb), plain[1:]))
    print("fused-backward-grid %s: weight / bias gradients of the two entries bit-identical: %s" % (tag, same))
    _hidden_check(tag, hidden, blocks, (plain[0], gw0.cpu(), gwb.cpu(), gb.cpu()), r64, r32)
