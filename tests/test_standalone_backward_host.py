"""The truth of tests/test_gpu_standalone_backward.py checked without a GPU (tests/_standalone_backward_util.py): the case ids
are unique, both references are finite on every case, the exclusions keep their caps, the recorded C constants are what the
float32 reference gives, the route predictors place a case on every branch the GPU file is there for, the float64 gradients
agree with central finite differences of the float64 forward, and rows on the ends of the interval or outside linear tails
have the closed-form gradient the GPU file's edge cases expect."""
import math

import pytest
import torch

import _standalone_backward_util as U
from flowconductor_amd import ops
from flowconductor_amd.ops import rq as rq_ops

IDS = list(U.SPECS)


def test_case_ids_are_unique_and_name_their_entry():
    assert len(set(IDS)) == len(IDS)
    assert all(i.startswith(U.SPECS[i].entry + "-") for i in IDS)
    assert {s.entry for s in U.SPECS.values()} == set(U.ENTRIES)


@pytest.mark.parametrize("cid", IDS)
def test_references_are_finite_and_exclusions_keep_their_caps(cid):
    cs = U.case(cid)
    flagged = int(U.excluded(cs).sum())
    if cs.n <= U.SMALL_ROWS:
        assert flagged == 0
    else:
        assert flagged <= U.MAX_SHARE * cs.distinct * cs.d_t
    for pair in U.reference(cid):
        for t in pair:
            assert bool(torch.isfinite(t).all())
    assert cs.x.shape == (cs.distinct, cs.d) and cs.params.shape == (cs.distinct, cs.d_t * U.params_per_dim(cs.spec))
    assert (cs.idx is None) == (cs.distinct == cs.n)


@pytest.mark.parametrize("entry", U.ENTRIES)
def test_recorded_constants_are_the_measured_ones(entry):
    c, median, p90, worst, count = U.measure_c(entry)
    print("%s: C %g, floor / scale median %.3g, 90 %% %.3g, max %.3g over %d slices" % (entry, c, median, p90, worst, count))
    assert U.C[entry] == c
    assert U.MARGIN == 4.0 and U.KNOT_WINDOW == 2.0 ** -18 and U.MAX_SHARE == 0.005


@pytest.mark.parametrize("entry", U.ENTRIES)
def test_the_derived_term_is_the_recorded_one(entry):
    """cond is a statement about single ill-conditioned elements.  Its median over an entry's grid, relative to the slice's
    scale, is recorded like C (rounded up to one digit) so that a change that loosens the net shows here; it is float64
    arithmetic on fixed seeds throughout, and finite everywhere."""
    median, p90 = U.measure_cond(entry)
    print("%s: cond / scale median %.3g, 90 %% %.3g" % (entry, median, p90))
    assert U.round_up_one_digit(median) == U.COND_MEDIAN[entry]
    assert U.ULP == 2.0 ** -23 and U.Rounded.HALF_ULP == 2.0 ** -24
    for cid in U.ids(entry):
        assert all(bool(torch.isfinite(t).all()) for t in U.conditioning(cid).values())


@pytest.mark.parametrize("cid", U.ids("rq"))
def test_the_restated_rq_adjoint_is_the_autograd_gradient(cid):
    """``rq_adjoint`` follows the kernel's formulas: its values are the float64 reference, and its error bound is at least
    half an ulp of every value (the last rounding)."""
    cs = U.case(cid)
    (gx, gp), _ = U.reference(cid)
    ax, ap, a_gx, a_gp = U.rq_adjoint(cs)
    assert float((ax - gx).abs().max()) <= 1e-9 * max(float(gx.abs().max()), 1e-30)
    assert float((ap - gp).abs().max()) <= 1e-9 * max(float(gp.abs().max()), 1e-30)
    inside = a_gx > 0
    assert bool((a_gx[inside] >= 2.0 ** -24 * ax[inside].abs()).all()) and bool((a_gp >= 2.0 ** -24 * ap.abs() * (1 - 1e-9)).all())
    assert bool(torch.isfinite(a_gx).all()) and bool(torch.isfinite(a_gp).all())


@pytest.mark.parametrize("entry", U.ENTRIES)
def test_the_grid_reaches_every_branch(entry):
    reached = set()
    for cid in U.ids(entry):
        reached |= U.branches(U.SPECS[cid])
    missing = [b for b in U.REQUIRED_BRANCHES[entry] if b not in reached]
    assert not missing, missing


def test_route_predictors_at_the_thresholds():
    # rq: 64 groups are the threshold of the wave kernel; the leftover rows are n mod G
    assert U.rq_route(512, 12, 8, 8, True) == (512, 0, "vector", True)
    assert U.rq_route(511, 12, 8, 8, True) == (0, 511, None, True)
    assert U.rq_route(517, 12, 8, 8, True) == (512, 5, "vector", True)
    assert U.rq_route(131, 33, 32, 8, True) == (130, 1, "scalar", True)
    assert U.rq_route(70, 65, 64, 4, False) == (70, 0, "scalar", True)
    assert U.rq_route(4103, 3, 1, 8, True) == (4096, 7, "vector", True)
    assert U.rq_route(4096, 64, 1, 16, False) == (0, 4096, None, True)          # 64 x 64 floats per strip: above 64 KB
    assert U.rq_route(512, 12, 8, 8, True, aligned_rows=False) == (0, 512, None, True)
    assert U.rq_route(512, 12, 8, 8, True, aligned_params=False) == (0, 512, None, True)
    assert U.rq_route(131, 33, 32, 8, True, aligned_rows=False)[0] == 130        # the scalar strip needs no alignment
    assert U.rq_route(512, 12, 8, 5, True) == (0, 512, None, False)
    assert U.rq_route(512, 12, 6, 8, True) == (0, 512, None, True)               # d_t no power of two
    assert U.rq_trips(8192, 0, 64) == (1, 0) and U.rq_trips(8192 + 130, 0, 64) == (2, 0)
    assert U.rq_trips(0, 43690, 48) == (0, 1) and U.rq_trips(0, 43800, 48) == (0, 2)
    # sos: the tile kernel up to S = 159 (one 160 KB tile per CU), the direct kernel from 160
    assert U.sos_route(210, 159, 256) == ("tile", 4, 4)
    assert U.sos_route(210, 160, 256) == ("direct", 1, 1)
    assert U.sos_route(256 * 5 * 64, 30, 256)[1:] == (1280, 1280) and U.sos_route(256 * 5 * 64 + 8, 30, 256)[1:] == (1281, 1280)
    # splines, affine
    assert U.splines_trips(256 * 8 * 256, 256) == 1 and U.splines_trips(256 * 8 * 256 + 1, 256) == 2
    trip2 = U.SPECS["spline-linear-K8-box-trip2"]
    assert U.splines_trips(trip2.n * 16 * 9, 256) == 2
    assert U.affine_trips(8192 * 256) == 1 and U.affine_trips(262200 * 8) == 2


def test_largest_bin_counts_are_those_of_the_operator():
    assert [U.largest_k(kind, tails) for (kind, tails) in U.SPLINE_MID] == [32, 32, 15, 16, 15, 15]
    for (kind, tails) in U.SPLINE_MID:
        k = U.largest_k(kind, tails)
        assert ops.spline_multiplier(U.KIND_CODE[kind], k, "linear" if tails else None) <= 32
        assert not ops.piecewise_spline_backward_supported(U.KIND_CODE[kind], k + 1, "linear" if tails else None)


@pytest.mark.parametrize("name", list(U.KNOT_CASES))
def test_knot_cases_sit_on_the_knots_with_room_on_either_side(name):
    """63 rows per case: every interior float64 knot's float32 rounding and 4 float32 neighbours on either side, all distinct
    and within 4 ulps of the knot; no bin narrower than 4 delta, so that x -+ 2 delta stays inside the neighbouring bin; the
    one-sided references are finite and their bound is positive."""
    cs = U.knot_case(name)
    lo, hi = U.interval(cs.spec)
    assert cs.x.shape == (63, 2) and cs.x.dtype == torch.float32 and cs.d_t == cs.d == 2
    assert U.narrowest_bin(cs) >= 4 * U.KNOT_SHIFT
    knots = U.inner_knots(cs)[0]                                      # [d_t, K - 1]
    x = cs.x.t().reshape(2, U.KNOT_K - 1, 9).double()
    assert bool((x[..., 1:] > x[..., :-1]).all())
    assert torch.equal(x[..., 4].float(), knots.float())
    ulp = torch.finfo(torch.float32).eps * (hi - lo)
    assert float((x - knots.unsqueeze(-1)).abs().max()) <= 4.5 * ulp < U.KNOT_SHIFT * (hi - lo) / 16
    assert not cs.cfg["tails"] or (lo, hi) == (-2.0, 2.0)
    for side in ("left", "right"):
        g64, bound = U.knot_reference(name)[side]
        assert bool(torch.isfinite(g64).all()) and float(bound.min()) > 0
    # the two sides are different answers, further apart than the two bounds together at every element: logabsdet's gradient
    # with respect to the parameters jumps at a knot, so a gradient that passes on one side cannot pass on the other, and
    # one that mixes the two bins passes on neither
    (left, bound_left), (right, bound_right) = U.knot_reference(name)["left"], U.knot_reference(name)["right"]
    gap = (left - right).abs().amax(dim=1)
    assert bool((gap > 10 * (bound_left + bound_right)).all()), float((gap / (bound_left + bound_right)).min())


FD_CASES = ["rq-K5-tails-d12-dt8-n512", "rq-K10-box-d12-dt8-n512", "sos-S6-n515-d5", "sos-S6-postact"] \
    + ["spline-%s-K%d-%s-d5-dt3-n400" % (kind, k, U._tn(tails)) for (kind, tails), k in U.SPLINE_MID.items()] \
    + [act + "-d10-dt6-n300" for act in ("affine-" + a for a in U.AFFINE_ACTS)]


@pytest.mark.parametrize("cid", FD_CASES)
def test_float64_reference_against_central_differences(cid):
    """<grad, v> against (L(p + e v) - L(p - e v)) / 2 e in float64, 32 random directions v in (x, params), an 8-row
    sub-batch: relative 1e-6.  A direction does not move an element that lies outside linear tails (y = x exactly there and a
    step must not carry it inside)."""
    full = U.case(cid)
    cs = U.take_rows(full, slice(0, 8))
    gx, gp = U.gradients(cs, torch.float64)
    xt, p = cs.x[:, U.tcols(cs)].double(), cs.params.double()
    inside = torch.ones_like(xt)
    if cs.entry in ("rq", "spline"):
        lo, hi = U.interval(cs.spec)
        inside = ((xt >= lo) & (xt <= hi)).double()
        assert bool(((U.inner_knots(cs) - xt.unsqueeze(-1)).abs().amin(-1) > 1e-4).all()), "an element a step away from a knot"
    gen = torch.Generator().manual_seed(len(cid))
    eps = 1e-6
    scale = float((gx.abs().sum() + gp.abs().sum()))
    with torch.no_grad():
        for _ in range(32):
            vx = torch.randn(xt.shape, generator=gen, dtype=torch.float64) * inside
            vp = torch.randn(p.shape, generator=gen, dtype=torch.float64)
            fd = float(U.loss(cs, xt + eps * vx, p + eps * vp) - U.loss(cs, xt - eps * vx, p - eps * vp)) / (2 * eps)
            an = float((gx * vx).sum() + (gp * vp).sum())
            assert abs(fd - an) <= 1e-6 * max(abs(an), 1e-3 * scale), (fd, an)


@pytest.mark.parametrize("cid", U.ids("rq", "edges") + U.ids("spline", "edges"))
def test_float64_reference_on_the_ends_and_outside(cid):
    """Outside linear tails the bijector is the identity: gx = gy exactly and no parameter gradient.  An RQ row exactly on an
    end of the interval with gl = 0: y is the pinned end whatever the parameters are, gp = 0; the end derivative is the
    constant's with linear tails (1, so gx = gy, unless enable_identity_init changes beta) and the free end derivative in
    the box.  On the ends of the clamped splines gy = 0
    (only logabsdet carries a gradient there)."""
    cs = U.case(cid)
    (gx, gp), _ = U.reference(cid)
    gyt = cs.gy[:, U.tcols(cs)].double()
    rows = gp.view(cs.distinct, cs.d_t, -1)
    if cs.cfg["tails"]:
        for r in (U.ROW_ABOVE, U.ROW_BELOW):
            assert torch.equal(gx[r], gyt[r]) and float(rows[r].abs().max()) == 0.0
    ends = [U.ROW_HI, U.ROW_LO]
    if cs.entry == "rq":
        assert float(cs.gl[ends].abs().max()) == 0.0
        assert float(rows[ends].abs().max()) <= 1e-12 * float(rows.abs().max())
        k = cs.cfg["k"]
        raw = cs.params.double().view(cs.distinct, cs.d_t, -1)
        beta = math.log(2.0) / (1 - 1e-3) if cs.cfg.get("ident") else 1.0
        if cs.cfg["tails"]:     # the padded constant log(exp(1 - 1e-3) - 1): derivative 1 at beta = 1, 1.295 under identity init
            u_end = torch.full((2, cs.d_t), math.log(math.exp(1 - 1e-3) - 1), dtype=torch.float64)
        else:
            u_end = torch.stack((raw[U.ROW_HI, :, 3 * k], raw[U.ROW_LO, :, 2 * k]))
        d_end = 1e-3 + torch.nn.functional.softplus(u_end * beta) / beta
        if cs.cfg["tails"] and not cs.cfg.get("ident"):
            assert float((d_end - 1.0).abs().max()) <= 1e-12
        assert float((gx[ends] - gyt[ends] * d_end).abs().max()) <= 1e-12
    elif cs.cfg["kind"] != "cubic":
        assert float(gyt[ends].abs().max()) == 0.0
    assert not bool(U.excluded(cs).any())


def test_rq_autograd_names_the_bin_limit_of_its_backward_kernel():
    """More than 32 bins: fc_rq_spline_backward would answer hipErrorInvalidValue in the middle of a backward pass; the
    autograd entry refuses up front, as piecewise_spline_autograd does."""
    x = torch.zeros(4, 2, requires_grad=True)
    params = torch.zeros(4, 2 * (3 * 33 - 1), requires_grad=True)
    with pytest.raises(NotImplementedError, match="32"):
        ops.rq_spline_autograd(x, params, None, num_bins=33, tails="linear", tail_bound=3.0)
    assert rq_ops.RQ_BACKWARD_MAX_BINS == 32
