"""What tests/test_gpu_affine_tail.py and tests/test_gpu_hidden_passes.py rest on, checked without a GPU: the fixture
conditions of every case on the reference alone, and the launch decisions of the hidden-stack kernels read through
fc_hidden_route (the host functions launch_coupling_tail, dispatch_hidden and launch_wide themselves call)."""
import ctypes
import os
import re

import pytest
import torch

import _affine_tail_util as U
import _ar_sampler_util as A
from flowconductor_amd import _hip, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = 4096


def _ok(kind, n, d, in_features, ctx=0, blocks=2, hidden=64):
    code, r = U.route(kind, n, d, in_features, ctx, blocks, hidden)
    assert code == 0 and r.code == 0, (kind, n, d, in_features, ctx, blocks, hidden, code)
    return r


@pytest.mark.parametrize("case", U.CASES, ids=U.case_id)
def test_fixture_conditions(case):
    """Float64 finite and at most 1 % of the rows beyond 1e3, both directions, on the reference alone; the float32 oracle
    leaves the other columns alone and has a floor above zero (a floor of zero would make the bound a demand for
    exactness; an additive layer's log-determinant is exactly 0 in both precisions)."""
    for inverse in U.directions(case):
        t, x, refs = U.references(case, ROWS, inverse)
        U.check_fixture(case, refs)
        cols = U.transformed_columns(case)
        rest = torch.ones(x.shape[1], dtype=torch.bool)
        rest[cols] = False
        assert torch.equal(refs[0][:, rest], x[:, rest]) and int(rest.sum()) == x.shape[1] - U.dims(case)[2]
        assert float(A.row_error(refs[0][:, cols], refs[2][:, cols]).median()) > 0.0
        assert (float(A.row_error(refs[1], refs[3]).max()) > 0.0) == (case.kind != "additive")


def test_the_widths_the_cases_cover():
    widths = {U.dims(c)[0] for c in U.CASES}
    assert {0, 1, 2, 3} <= {w % 4 for w in widths} and {32, 33, 64, 65, 96, 128} <= widths
    assert {1, 32} <= {U.dims(c)[2] for c in U.CASES} and {1, 33, 64} <= {U.dims(c)[1] for c in U.CASES}
    assert {2, 7, 32} <= {c.d for c in U.CASES if c.kind == "maf"}
    assert any(c.mask is not None and c.mask[0] == "random" for c in U.CASES)
    assert {c.kind for c in U.CASES} == {"affine", "general", "additive", "maf"}
    assert sorted(U.IMAGES) == sorted({(nb, k0s) for nb in range(4) for k0s in (1, 2)})
    for nb, k0s in U.IMAGES:
        for kind in ("affine", "maf"):
            if kind == "maf" and k0s == 2:
                continue
            c = U.image_case(nb, k0s, kind)
            assert (c.blocks, 1 if U.dims(c)[1] <= 32 else 2) == (nb, k0s)


def test_the_case_table_covers_every_reachable_instantiation():
    """Every (NB, K0S, blocks per wave, XVT) fc_hidden_route reports for some width at n_big rows is the route of a case
    (the one-block forms are also all run at 213 rows); one case loses its pair form to the LDS rule and still runs as
    one launch; a batch between the two thresholds walks several passes of single blocks."""
    n = U.n_big()
    body = n - n % 16
    reachable = U.reachable(body)
    covered = {U.instantiation(c, n) for c in U.CASES}
    assert {r for r in reachable if r[2] == 2} <= covered, sorted(reachable - covered)
    assert {(nb, k0s, 2, xvt) for nb, k0s, bpw, xvt in reachable if bpw == 2} == {
        (nb, k0s, 2, xvt) for nb in range(4) for k0s in (1, 2) for xvt in (2, 4)
        if not (k0s == 2 and (xvt == 2 or nb == 3))}                     # 2 k-steps: D >= 33; with 3 blocks no second tile fits
    assert {2, 4} <= {r[3] for r in covered if r[2] == 2}
    for c in U.pair_cases(n):
        r = U.tail_route(c, n)[1]
        assert r.repeats == 1 and r.passes >= 2 and (n // 16) % 2 == 1
        assert U.tail_route(c, n + 16)[1].repeats == 0
    dropped = [c for c in U.CASES if U.dims(c)[0] <= 64 and U.instantiation(c, n)[2] == 1]
    assert len(dropped) == 1 and dropped[0].blocks == 3 and U.tail_route(dropped[0], n)[1].passes == 3
    for c in U.CASES:
        if U.dims(c)[0] > 64:
            r = U.tail_route(c, n)[1]
            assert (r.bpw, r.xvt, r.passes) == (1, 8, 3)
    mid = U.tail_route(U.CASES[-1], U.n_mid())[1]
    assert U.dims(U.CASES[-1])[0] <= 64 and (mid.bpw, mid.passes) == (1, 2)


def test_declaration_and_binding_agree():
    text = open(os.path.join(ROOT, "include", "flowcon_hip.h")).read()
    decl = re.search(r"\bint\s+fc_hidden_route\s*\(([^)]*)\)", text)
    assert decl and "fc_hidden_route" in _hip.SIGNATURES
    assert len(decl.group(1).split(",")) == len(_hip.SIGNATURES["fc_hidden_route"]) == 8
    kinds = dict(re.findall(r"#define\s+FC_ROUTE_(\w+)\s+(\d+)", text))
    assert {k: int(v) for k, v in kinds.items()} == {"HIDDEN": U.STACK, "HIDDEN_GLU": U.GLU, "HIDDEN_ADDITIVE": U.ADDITIVE,
                                                    "COUPLING_TAIL": U.TAIL, "HIDDEN_WIDE": U.WIDE}
    assert _hip.ABI_VERSION == 3


def test_refused_arguments():
    lib = _hip.load()
    out = (ctypes.c_int64 * 8)()
    assert lib.fc_hidden_route(U.TAIL, 64, 32, 16, 0, 2, 64, None) != 0
    bad = [(5, 64, 32, 16, 0, 2, 64), (-1, 64, 32, 16, 0, 2, 64),      # kind
           (U.TAIL, -16, 32, 16, 0, 2, 64), (U.TAIL, 65, 32, 16, 0, 2, 64),   # rows
           (U.TAIL, 64, 0, 16, 0, 2, 64), (U.TAIL, 64, 129, 16, 0, 2, 64),    # width
           (U.TAIL, 64, 32, 0, 0, 2, 64), (U.TAIL, 64, 32, 33, 0, 2, 64), (U.TAIL, 64, 128, 65, 0, 2, 64),
           (U.TAIL, 64, 32, 16, 0, 4, 64), (U.TAIL, 64, 32, 16, 0, -1, 64), (U.TAIL, 64, 32, 16, 0, 2, 128),
           (U.TAIL, 64, 32, 16, 3, 2, 64),                                     # a context where the entry has none
           (U.STACK, 64, 32, 16, 0, 5, 64), (U.STACK, 64, 32, 16, 0, 2, 32),
           (U.GLU, 64, 32, 16, 0, 2, 64), (U.GLU, 64, 32, 16, 33, 2, 64), (U.GLU, 64, 64, 40, 25, 2, 64),
           (U.GLU, 64, 32, 16, 8, 4, 64), (U.ADDITIVE, 64, 32, 16, 0, 2, 64),
           (U.WIDE, 48, 32, 16, 0, 2, 128), (U.WIDE, 64, 32, 16, 0, 2, 64), (U.WIDE, 64, 32, 16, 0, 17, 256)]
    for args in bad:
        assert lib.fc_hidden_route(*args, out) != 0 and out[7] != 0 and list(out)[:7] == [0] * 7, args
    assert U.route(U.ADDITIVE, 64, 64, 40, 25, 2) [0] == 0                    # the additive context is not concatenated
    assert U.route(U.TAIL, 0, 32, 16, 0, 2) == (0, U.Route(0, 0, 0, 0, 0, 0, 0, 0))
    # the one-block form of 3 blocks + 2 k-steps needs 131 KB + a [16][D | 1] tile per wave: over 160 KB from D 56 on
    code, r = U.route(U.TAIL, 64, 65, 64, 0, 3)
    assert code != 0 and r.code == code and r.lds > U.LDS_PER_CU and not ops.affine_tail_fits(64, 3, 65)


def test_thresholds_of_the_coupling_tail():
    """Pairs from exactly 2 x 8 x CUs blocks on and up to D 64; 2 row pieces per lane up to D 32, 4 beyond."""
    cus = U.cus()
    edge = 2 * 8 * cus * 16
    for d, in_features in ((8, 4), (32, 16), (33, 16), (64, 32), (64, 33)):
        below, at = _ok(U.TAIL, edge - 16, d, in_features, blocks=1), _ok(U.TAIL, edge, d, in_features, blocks=1)
        assert (below.bpw, below.xvt, below.grid, below.passes) == (1, 8, cus, 2)
        assert (at.bpw, at.xvt, at.grid, at.passes, at.repeats) == (2, 2 if d <= 32 else 4, cus, 1, 0)
        assert _ok(U.TAIL, edge + 16, d, in_features, blocks=1).repeats == 1
        assert at.lds - below.lds == 8 * 16 * (d | 1) * 4
    for d in (65, 96, 128):
        r = _ok(U.TAIL, 4 * edge, d, 32)
        assert (r.bpw, r.xvt, r.passes) == (1, 8, 8)
    small = _ok(U.TAIL, 208, 12, 6)
    assert (small.bpw, small.grid, small.waves, small.passes) == (1, 2, 16, 1)
    # one pass of single blocks ends at 128 rows per CU
    assert _ok(U.TAIL, 128 * cus, 48, 24).passes == 1 and _ok(U.TAIL, 128 * cus + 16, 48, 24).passes == 2


def test_the_lds_rule_is_the_kernels_own_sum():
    """The pair form goes where the image + two tiles per wave exceed 160 KB; the one-block form fits exactly where
    ops.affine_tail_fits says so.  The image: 1 KB fragments (8 per k-step of the initial layer, 16 per later layer), 256 B of
    biases per layer, 64 + 128 K0S + 512 B of scales, column indices and scratch."""
    n = 2 * 8 * U.cus() * 16
    for nb in range(4):
        for in_features in (1, 32, 33, 64):
            k0s = 1 if in_features <= 32 else 2
            image = (8 * k0s + 16 * (2 * nb + 1)) * 1024 + (2 + 2 * nb) * 256 + 64 + 128 * k0s + 512
            for d in range(in_features, 129):
                code, r = U.route(U.TAIL, n, d, in_features, 0, nb)
                pair = d <= 64 and image + 2 * 8 * 16 * (d | 1) * 4 <= U.LDS_PER_CU
                assert r.bpw == (2 if pair else 1), (nb, in_features, d)
                assert r.lds == image + r.bpw * 8 * 16 * (d | 1) * 4
                assert (code == 0) == ops.affine_tail_fits(in_features, nb, d) == (r.lds <= U.LDS_PER_CU), (nb, in_features, d)


def test_invariants_over_a_sweep():
    """grid x 8 waves x passes covers all groups and one pass less does not; never more workgroups than the route's
    share of the CUs; LDS within 160 KB whenever the launch is accepted."""
    cus = U.cus()
    shapes = [(U.TAIL, d, k, 0, nb, 64) for d, k in ((2, 2), (12, 6), (33, 20), (64, 33), (65, 64), (128, 40)) for nb in range(4)]
    shapes += [(U.STACK, 64, k, 0, nb, 64) for k in (7, 32, 48) for nb in range(5)]
    shapes += [(kind, 64, k, c, nb, 64) for kind in (U.GLU, U.ADDITIVE) for k, c in ((16, 8), (40, 24), (12, 5)) for nb in range(4)]
    shapes += [(U.WIDE, 64, k, 0, nb, h) for k in (16, 48) for nb in (0, 2, 16) for h in (128, 256)]
    for kind, d, k, c, nb, hidden in shapes:
        rows = 64 if kind == U.WIDE else 16
        for units in (1, 7, 8, 9, 8 * cus - 1, 8 * cus, 8 * cus + 1, 16 * cus - 1, 16 * cus, 16 * cus + 3, 40 * cus + 5):
            code, r = U.route(kind, units * rows, d, k, c, nb, hidden)
            what = (kind, d, k, c, nb, hidden, units, r)
            assert r.code == code, what
            if code != 0:
                assert kind == U.TAIL and r.lds > U.LDS_PER_CU, what
                continue
            assert r.lds <= U.LDS_PER_CU and r.waves == 8 * r.grid and 1 <= r.grid <= 2 * cus, what
            groups = units if kind == U.WIDE else -(-units // r.bpw)
            walkers = r.grid if kind == U.WIDE else r.waves
            assert walkers * (r.passes - 1) < groups <= walkers * r.passes, what
            assert r.repeats == (1 if kind != U.WIDE and r.bpw == 2 and units % 2 else 0), what
            assert (r.xvt != 0) == (kind == U.TAIL) and (r.bpw == 4) == (kind == U.WIDE), what
            if kind in (U.STACK, U.GLU, U.ADDITIVE):
                assert r.bpw == 1, what
                # two workgroups per CU only where two images fit: no context, <= 2 blocks at <= 32 inputs
                two = kind == U.STACK and (8 if k <= 32 else 16) + 32 * nb + 2 <= 80
                assert r.grid == min((2 if two else 1) * cus, -(-units // 8)), what
            if kind == U.WIDE:
                assert r.grid == min(2 * cus, units) and r.lds == 2 * 64 * (hidden + 8) * 2 + 64 * 4 + 2 * 64 * 4 + 64 * 4, what
