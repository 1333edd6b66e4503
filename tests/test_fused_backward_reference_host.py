"""The float64 truth of tests/test_gpu_fused_backward_grid.py checked without a GPU: the seeds keep the inputs away from the
knots (the conditions of ``near_knot``), both references are finite on every case, the float64 gradient agrees with central
finite differences of the float64 forward, and a row exactly on the end of the spline's interval has the gradient the GPU
file's exact-edge case expects."""
import pytest
import torch

import _fused_backward_util as U

CASES = U.grid_cases()
IDS = [U.case_id(*c[1:]) for c in CASES]


def test_ids_name_every_instantiation_once_per_shape():
    assert len(set(IDS)) == len(IDS)
    for (k, tails) in U.INSTANCES:
        assert sum(i.startswith("K%d-%s-" % (k, U.tails_name(tails))) and i.count("-") == 4 for i in IDS) == len(U.SHAPES)
        assert U.param_count(k, tails) <= 32
    assert U.param_count(12, "linear") > 32 and U.param_count(11, None) > 32        # the dispatcher's default: cases


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_inputs_keep_away_from_the_knots_and_references_are_finite(c):
    cs = U.case(*c[1:6], edge=c[6])
    r64, r32 = U.reference(cs, torch.float64, full=True), U.reference(cs, torch.float32, full=True)
    flagged = U.near_knot(cs, r64.rows).any(dim=1)
    if c[0] == "C":
        assert float(flagged.float().mean()) <= 0.005
    else:
        assert not bool(flagged.any())
    for t in tuple(r64[:5]) + tuple(r32[:5]):
        assert bool(torch.isfinite(t).all())


@pytest.mark.parametrize("k,tails", [(6, "linear"), (7, None)])
def test_float64_reference_against_central_differences(k, tails):
    """<grad, v> against (L(p + e v) - L(p - e v)) / 2 e in float64, 64 random directions v in (x, h, W, b), an 8-row
    sub-batch (rows 3 and 4 outside the tails): relative 1e-6."""
    cs = U.take_rows(U.case(k, tails, 24, 11, 64), slice(0, 8))
    grads = U.reference(cs, torch.float64)
    point = [t.double() for t in (cs.x, cs.h, cs.w, cs.b)]
    gen = torch.Generator().manual_seed(k)
    eps = 1e-6
    with torch.no_grad():
        for _ in range(64):
            v = [torch.randn(t.shape, generator=gen, dtype=torch.float64) for t in point]
            if tails == "linear":
                v[0][3:5] = 0.0             # (outside the tails y = x exactly; a step must not carry a row inside)
            up = U.loss(cs, *[t + eps * d for t, d in zip(point, v)])[0]
            down = U.loss(cs, *[t - eps * d for t, d in zip(point, v)])[0]
            fd = float(up - down) / (2 * eps)
            an = float(sum((g * d).sum() for g, d in zip(grads, v)))
            assert abs(fd - an) <= 1e-6 * abs(an), (fd, an)
    if tails == "linear":
        assert torch.equal(grads[0][3:5], cs.gy[3:5].double())


@pytest.mark.parametrize("k,tails", [(8, "linear"), (11, "linear"), (9, None)])
def test_float64_reference_on_the_ends_of_the_interval(k, tails):
    """A row exactly on +-tail_bound (linear tails) or on 0.0 / 1.0 (box) with gl = 0: y is the pinned end of the interval
    whatever the parameters are, so the row adds nothing to gW, gb and gh; with linear tails the end derivative is the
    constant 1 and gx = gy there; in the box it is the free end derivative d_0 / d_K, gx = gy d."""
    cs = U.case(k, tails, 24, 11, 64, edge="on_edge")
    gx = U.reference(cs, torch.float64)[0]
    tc = cs.cols.long()
    rows = list(U.ON_EDGE_ROWS)
    if tails == "linear":
        assert float((gx[rows][:, tc] - cs.gy[rows][:, tc].double()).abs().max()) <= 1e-12
    else:
        p = U.param_count(k, tails)
        raw = (cs.h.double() @ cs.w.double().T + cs.b.double()).view(cs.n, cs.d_t, p)[rows]
        ends = 1e-3 + torch.nn.functional.softplus(torch.stack((raw[0, :, p - 1], raw[1, :, 2 * k])))
        assert float((gx[rows][:, tc] - cs.gy[rows][:, tc].double() * ends).abs().max()) <= 1e-12
    only = U.take_rows(cs, rows)
    _, gh, gw, gb = U.reference(only, torch.float64)
    assert float(gw.abs().max()) <= 1e-12 and float(gb.abs().max()) <= 1e-12 and float(gh.abs().max()) <= 1e-12
