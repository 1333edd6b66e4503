"""fc_affine_coupling_resnet (hidden stack + final Linear + affine bijector in one launch: the kTail form of
resnet_hidden_kernel) held to float64 on EVERY row of both launch routes: one 16-row block per wave (one pass and several),
and two blocks per wave at 256 rows per CU and more (2 and 4 row pieces per lane, odd and even block counts).

Every test first asks fc_hidden_route which route its batch takes and asserts the one it is named for, then prints one line
per case: the route, and the population summary of the row errors next to the float32 oracle's on the same rows.  The
bound is the row-wise one of tests/_ar_sampler_util.py, on the transformed columns and on the log-determinant separately;
every other column carries the input's bits."""
import copy
import gc

import pytest
import torch

import _affine_tail_util as U
from flowconductor_amd import ops

pytestmark = pytest.mark.gpu

ENTRY = "fc_affine_coupling_resnet"
KINDS = ("affine", "general", "additive", "maf")
SMALL = 208 + 5               # 13 blocks: one pass of single blocks; 5 rows left over for the stand-alone path
_RUNS = {}


@pytest.fixture(scope="module", autouse=True)
def _device_memory_given_back():
    """The large launches are kept for the tests that share them (about 1 GB of device tensors).  They go with the module,
    and the allocator's cached blocks of their odd sizes with them: the files after this one find the allocator as they
    always did (tests/test_gpu_batch_statistics.py::test_saved_memory counts a reused larger block as its own peak)."""
    yield
    _RUNS.clear()
    gc.collect()
    if torch.cuda.is_available():
        torch.cuda.empty_cache()


def _leftover(case):
    return 0 if case.ride else 5          # ops.affine_coupling_resnet itself takes whole blocks only


def _report(label, case, n, want):
    """Asserts the route ``want`` = dict of Route fields for the whole blocks of an ``n``-row batch; prints it."""
    code, r = U.tail_route(case, n)
    print(U.format_route(label, case, n, r))
    assert code == 0 and {k: getattr(r, k) for k in want} == want, (label, n, r)
    return r


def _launch(t, case, xd, inverse, total=None):
    with ops.KernelTimer(ENTRY) as timer:
        out = U.run(t, case, xd, inverse, total)
    assert len(timer.pairs) == 1, "%s did not run as one launch" % ENTRY
    return out


def _run(case, inverse, n, device):
    """The case's layer on its ``n`` input rows, once per (case, direction, n): ``(layer, x, x on the device, y, lad)``."""
    key = (case, inverse, n)
    if key not in _RUNS:
        t = U.build(case).to(device)
        x = U.inputs(case, n)
        xd = x.to(device)
        _RUNS[key] = (t, x, xd) + tuple(_launch(t, case, xd, inverse))
    return _RUNS[key]


def _big(case):
    return U.n_big(_leftover(case))


def _label(case, inverse):
    return U.case_id(case) + (" inverse" if inverse else " forward")


def _both(cases):
    return [pytest.param(c, inv, id=_label(c, inv).replace(" ", "-")) for c in cases for inv in U.directions(c)]


# ---- one block per wave, one pass: every instantiation ---------------------------------------------------------------------
SMALL_CASES = [U.image_case(nb, k0s, kind) for nb, k0s in U.IMAGES for kind in KINDS if not (kind == "maf" and k0s == 2)]


@pytest.mark.parametrize("case,inverse", _both(SMALL_CASES))
def test_one_block_route_every_weight_image(case, inverse, device):
    """NB 0..3 x one / two k-steps of the initial layer x the four scale activations, 213 rows: one launch of the kernel,
    the 5 leftover rows on the stand-alone path under the same bound."""
    _report(_label(case, inverse), case, SMALL, dict(bpw=1, xvt=8, passes=1, repeats=0))
    assert U.instantiation(case, SMALL)[:2] in U.IMAGES
    t, x, refs = U.references(case, SMALL, inverse)
    got = _launch(t.to(device), case, x.to(device), inverse)
    U.check(_label(case, inverse), case, x, got, refs)


# ---- the large routes: float64 on all rows ---------------------------------------------------------------------------------
def _all_rows(case, inverse, n, device):
    t, x, xd, y, lad = _run(case, inverse, n, device)
    refs = U.oracle(U.build(case), case, x, inverse)
    return U.check(_label(case, inverse), case, x, (y, lad), refs)


ONE_BLOCK_BIG = [c for c in U.CASES if U.dims(c)[0] > 64]
BETWEEN = U.CASES[-1]


@pytest.mark.parametrize("case,inverse", _both(ONE_BLOCK_BIG))
def test_one_block_route_several_passes_wide_rows(case, inverse, device):
    """D 65, 96 and 128 at 256 rows per CU + 3 blocks: three passes of single blocks, the rows of a later pass fetched one
    iteration ahead."""
    assert sorted(U.dims(c)[0] for c in ONE_BLOCK_BIG) == [65, 96, 128]
    _report(_label(case, inverse), case, _big(case), dict(bpw=1, xvt=8, passes=3, repeats=0))
    _all_rows(case, inverse, _big(case), device)


@pytest.mark.parametrize("inverse", [False, True])
def test_one_block_route_between_the_thresholds(inverse, device):
    """D <= 64 at 192 rows per CU + 3 blocks: past one pass of single blocks, not yet pairs."""
    _report(_label(BETWEEN, inverse), BETWEEN, U.n_mid(), dict(bpw=1, xvt=8, passes=2, repeats=0))
    _all_rows(BETWEEN, inverse, U.n_mid(), device)


def _pair_cases():
    return U.pair_cases(U.n_big())


def _dropped():
    return [c for c in U.CASES if U.dims(c)[0] <= 64 and c not in _pair_cases()]


@pytest.mark.parametrize("case,inverse", _both(_pair_cases()))
def test_pair_route_all_rows(case, inverse, device):
    """Every (NB, K0S, XVT) whose pair form exists, at an odd number of blocks: the last group repeats a block."""
    n = _big(case)
    r = _report(_label(case, inverse), case, n, dict(bpw=2, repeats=1))
    assert r.xvt == (2 if U.dims(case)[0] <= 32 else 4) and r.passes >= 2
    _all_rows(case, inverse, n, device)


def test_pair_route_covers_every_reachable_instantiation():
    n = U.n_big()
    want = {r for r in U.reachable(n - n % 16) if r[2] == 2}
    assert want and want <= {U.instantiation(c, n) for c in _pair_cases()}


@pytest.mark.parametrize("case,inverse", _both(_dropped()))
def test_large_batch_whose_pair_form_the_table_drops(case, inverse, device):
    """3 blocks at D 64: two row tiles per wave do not fit next to the weight image, so the large batch stays on the
    one-block kernel -- one launch, three passes."""
    _report(_label(case, inverse), case, _big(case), dict(bpw=1, xvt=8, passes=3, repeats=0))
    _all_rows(case, inverse, _big(case), device)


def _one_per_xvt():
    seen, picked = set(), []
    for c in _pair_cases():
        xvt = U.instantiation(c, U.n_big())[3]
        if xvt not in seen and c.kind != "maf":
            seen.add(xvt)
            picked.append(c)
    return picked


@pytest.mark.parametrize("case,inverse", _both(_one_per_xvt()))
def test_pair_route_even_count_gives_the_rows_of_the_odd_count(case, inverse, device):
    """One more block makes the count even (no repeated block): the rows the two launches share come out bit for bit the
    same."""
    n = _big(case)
    body = n - n % 16
    t, x, xd, y, lad = _run(case, inverse, n, device)
    _report(_label(case, inverse) + " odd", case, body, dict(bpw=2, repeats=1))
    _report(_label(case, inverse) + " even", case, body + 16, dict(bpw=2, repeats=0))
    y_even, lad_even = _launch(t, case, torch.cat((xd[:body], xd[:16])), inverse)
    assert torch.equal(y_even[:body], y[:body]) and torch.equal(lad_even[:body], lad[:body])
    assert torch.equal(y_even[body:], y[:16]) and torch.equal(lad_even[body:], lad[:16])


LARGE = [(c, None) for c in _pair_cases() + ONE_BLOCK_BIG + _dropped()] + [(BETWEEN, "mid")]


@pytest.mark.parametrize("case,inverse,mid", [pytest.param(c, inv, m, id=_label(c, inv).replace(" ", "-") + ("-mid" if m else ""))
                                              for c, m in LARGE for inv in U.directions(c)])
def test_rows_of_a_large_launch_equal_single_pass_launches(case, inverse, mid, device):
    """The large batch again in contiguous pieces of at most 128 rows per CU -- one pass, one block per wave: every row's
    outputs and log-determinant are the same bits on either route."""
    n = U.n_mid() if mid else _big(case)
    t, x, xd, y, lad = _run(case, inverse, n, device)
    body = n - n % 16
    piece = 128 * U.cus()
    ys, lads = [], []
    for lo in range(0, body, piece):
        rows = xd[lo:min(lo + piece, body)]
        _report("%s rows %d.." % (_label(case, inverse), lo), case, rows.shape[0], dict(bpw=1, xvt=8, passes=1, repeats=0))
        out = _launch(t, case, rows, inverse)
        ys.append(out[0])
        lads.append(out[1])
    assert len(ys) >= 2
    assert torch.equal(torch.cat(ys), y[:body]), "outputs differ between the large launch and single-pass launches"
    assert torch.equal(torch.cat(lads), lad[:body]), "log-determinants differ between the large launch and single-pass launches"


# ---- the running total --------------------------------------------------------------------------------------------------
TOTAL_CASES = [U.CASES[0], U.CASES[4], U.CASES[7], ONE_BLOCK_BIG[1], ONE_BLOCK_BIG[2]]


@pytest.mark.parametrize("case,inverse", _both(TOTAL_CASES))
def test_running_total_gets_every_row_added_once(case, inverse, device):
    """logabsdet_accum on the pair route with an odd count (the repeated block must not be added twice) and on the
    several-pass one-block route: total == prior + lad on every row, the outputs unchanged."""
    n = _big(case)
    t, x, xd, y, lad = _run(case, inverse, n, device)
    r = _report(_label(case, inverse) + " accumulate", case, n, dict())
    assert (r.bpw == 2 and r.repeats == 1) or (r.bpw == 1 and r.passes == 3)
    prior = (torch.randn(n, generator=torch.Generator().manual_seed(3)) * 5.0).to(device)
    total = prior.clone()
    y_acc, returned = _launch(t, case, xd, inverse, total)
    assert returned.data_ptr() == total.data_ptr() and torch.equal(y_acc, y)
    expect = prior.double() + lad.double()
    err = (total.double() - expect).abs() / expect.abs().clamp(min=1.0)
    worst = int(err.argmax())
    print("running total %s: max relative error %.3g at row %d of %d (block %d of %d)"
          % (_label(case, inverse), float(err.max()), worst, n, worst // 16, -(-n // 16)))
    assert float(err.max()) <= 1e-6
    last = slice(n - n % 16 - 16, n - n % 16)         # the block the last group of an odd count repeats
    assert float(err[last].max()) <= 1e-6 and not torch.equal(total[last], prior[last])


# ---- saturated scale activations -----------------------------------------------------------------------------------------
def _final(t, case):
    return (t.autoregressive_net if case.kind == "maf" else t.transform_net).final_layer


def _scale_row(case, j):
    """Row of the final Linear that gives the raw scale of transformed dim ``j``."""
    return 2 * j if case.kind == "maf" else U.dims(case)[2] + j


def _saturated(case, low, high):
    t = U.build(case)
    final = _final(t, case)
    with torch.no_grad():
        for dims_, value in ((low, -40.0), (high, 40.0)):
            for j in dims_:
                final.weight[_scale_row(case, j)].zero_()
                final.bias[_scale_row(case, j)] = value
    return t


SATURATED = [U.CASES[0], U.CASES[1], U.CASES[5]]       # sigmoid(u + 2) + 1e-3, the clamp at 3, the MAF softplus + 1e-3


@pytest.mark.parametrize("case,inverse", _both(SATURATED))
@pytest.mark.parametrize("big", [False, True], ids=["small", "pair-route"])
def test_saturated_scale_activations(case, inverse, big, device):
    """Raw scales of -40 and +40 (zero final weights, so every row gets them): sigmoid(-38) + 1e-3 and sigmoid(42) + 1e-3,
    softplus(40) + 1e-3 clamped to exactly 3 (log-determinant log 3), softplus(-40) + 1e-3.  The inverse divides by the
    scale, and a scale of 1e-3 on a fifth of the dims would put most rows beyond the fixture's 1e3: it gets the +40 dims."""
    d_t = U.dims(case)[2]
    high, low = [1, d_t - 1], ([] if inverse else [2, d_t // 2])
    n = _big(case) if big else SMALL
    _report(_label(case, inverse) + " saturated", case, n, dict(bpw=2, repeats=1) if big else dict(bpw=1, passes=1))
    t = _saturated(case, low, high)
    x = U.inputs(case, n)
    refs = U.oracle(t, case, x, inverse)
    got = _launch(copy.deepcopy(t).to(device), case, x.to(device), inverse)
    U.check(_label(case, inverse) + " saturated", case, x, got, refs)


@pytest.mark.parametrize("case", [U.CASES[0], U.CASES[1], U.CASES[5]], ids=U.case_id)
def test_zero_weight_conditioner_gives_every_row_the_same_parameters(case, device):
    """All weights of the conditioner zero, its biases kept: shift and scale are the final biases on every row, so the
    log-determinant is one number."""
    t = U.build(case)
    net = t.autoregressive_net if case.kind == "maf" else t.transform_net
    with torch.no_grad():
        for name, p in net.named_parameters():
            if name.endswith("weight"):
                p.zero_()
    x = U.inputs(case, SMALL)
    refs = U.oracle(t, case, x, False)
    assert float((refs[3] - refs[3][0]).abs().max()) == 0.0
    _report(U.case_id(case) + " zero weights", case, SMALL, dict(bpw=1, passes=1))
    got = _launch(copy.deepcopy(t).to(device), case, x.to(device), False)
    U.check(U.case_id(case) + " zero weights", case, x, got, refs)
    body = SMALL - SMALL % 16
    assert bool((got[1][:body] == got[1][0]).all()), "rows of one launch with the same parameters, different log-determinants"


# ---- row scales ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,inverse", _both([U.CASES[0], U.CASES[8], U.CASES[4], ONE_BLOCK_BIG[1]]))
def test_row_scales_over_eleven_decades(case, inverse, device):
    """Rows multiplied by logspace(-6, 5): the row maximum that scales the split-f16 operands of the initial layer.  The
    bound is relative to each row's own scale, so it holds a row of 1e5 as it holds a row of 1e-6; the fixture's share of
    rows beyond 1e3 does not apply to inputs that are beyond it by construction (float64 finite does)."""
    n = 2048 + 5 * bool(_leftover(case))
    _report(_label(case, inverse) + " row scales", case, n, dict(bpw=1, passes=1))
    t = U.build(case)
    x = U.inputs(case, n) * torch.logspace(-6, 5, n).unsqueeze(1)
    refs = U.oracle(t, case, x, inverse)
    got = _launch(t.to(device), case, x.to(device), inverse)
    y, lad = got[0].cpu(), got[1].cpu()
    cols = U.transformed_columns(case)
    assert bool(torch.isfinite(refs[2]).all()) and bool(torch.isfinite(refs[3]).all()) and bool(torch.isfinite(refs[0]).all())
    bad_y, stats_y = U.A.quantity_violations("y", y[:, cols], refs[0][:, cols], refs[2][:, cols])
    bad_l, stats_l = U.A.quantity_violations("lad", lad, refs[1], refs[3])
    print(U.A.format_stats(_label(case, inverse) + " row scales", {"y": stats_y, "lad": stats_l}))
    rest = torch.ones(x.shape[1], dtype=torch.bool)
    rest[cols] = False
    assert torch.equal(y[:, rest], x[:, rest])
    assert not bad_y + bad_l, "; ".join(bad_y + bad_l)


# ---- a non-finite row stays alone ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,inverse", _both([U.CASES[0], U.CASES[7], ONE_BLOCK_BIG[1]]))
def test_a_non_finite_row_stays_alone(case, inverse, device):
    """One NaN in an identity column of a row in a first-pass block, of a row in the second block of a first-pass pair
    (the first pass's second block on the one-block route) and of a row in a later pass: those rows' transformed columns and
    log-determinant are NaN, their other identity columns and every other row of the batch keep the clean run's bits."""
    n = _big(case)
    t, x, xd, y, lad = _run(case, inverse, n, device)
    r = _report(_label(case, inverse) + " NaN rows", case, n, dict())
    assert r.passes >= 2
    later = r.waves * r.bpw * 16                      # the first row of the second pass
    rows = [5, 16 + 3, later + 16 * (r.bpw - 1) + 9]
    assert rows[-1] < n - n % 16
    ident = t.identity_features.cpu()
    col = int(ident[len(ident) // 2])
    dirty = xd.clone()
    dirty[rows, col] = float("nan")
    yd, ladd = _launch(t, case, dirty, inverse)
    cols = U.transformed_columns(case).to(device)
    hit = torch.tensor(rows, device=device)
    assert bool(torch.isnan(yd[hit][:, cols]).all()) and bool(torch.isnan(ladd[hit]).all())
    others = ident[ident != col].to(device)
    assert torch.equal(yd[hit][:, others], xd[hit][:, others]) and bool(torch.isnan(yd[hit, col]).all())
    clean = torch.ones(n, dtype=torch.bool, device=device)
    clean[hit] = False
    assert torch.equal(yd[clean], y[clean]) and torch.equal(ladd[clean], lad[clean])


# ---- a row-sliced view ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,inverse", _both([U.CASES[1], U.CASES[2], U.CASES[3]]))
def test_misaligned_view_gives_the_rows_of_the_full_batch(case, inverse, device):
    """x[1:] at a row of 124 / 116 / 72 bytes starts off a 16-byte boundary: the rows of the full batch, under the same
    bound (and within the older test's tolerance of the full batch's own outputs)."""
    assert (4 * U.dims(case)[0]) % 16 != 0
    t, x, refs = U.references(case, SMALL + 1, inverse)
    t = t.to(device)
    xd = x.to(device)
    y, lad = _launch(t, case, xd, inverse)
    view = xd[1:]
    assert view.data_ptr() % 16 != 0
    _report(_label(case, inverse) + " view", case, SMALL, dict(bpw=1, passes=1))
    yv, ladv = _launch(t, case, view, inverse)
    U.check(_label(case, inverse) + " x[1:]", case, x[1:], (yv, ladv), tuple(r[1:] for r in refs))
    tol = 1e-4 if inverse else 2e-5
    assert float((yv - y[1:]).abs().max()) <= tol * max(1.0, float(refs[0].abs().max()))
    assert float((ladv - lad[1:]).abs().max()) <= 1e-5 * max(1.0, float(refs[1].abs().max()))
