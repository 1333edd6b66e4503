"""The forward kernels of the row-per-wavefront family (``fc_householder``, ``fc_planar``, ``fc_sylvester``) and the
matrix-core Sylvester kernel (``fc_sylvester_mm``) against float64 on every route: every instantiation at its width edges
(a), later iterations of every persistent loop (b), the matrix-core kernel's edges and the module glue around it (c),
non-finite rows in the kernels that pack several samples into a wave (d), unaligned views (e) and the modules' own
host-side arithmetic (f).

References, the row-wise bound (max(e) <= 4 max(f) + 1e-5, quantile lines from 1000 rows on, finite wherever float64 is; y
and logabsdet separately), the mirror of the dispatch and the case tables are in tests/_rowwave_forward_util.py;
tests/test_rowwave_forward_host.py counts that the tables reach every instantiation.  Every call goes through the public
wrappers and asserts with ``ops.KernelTimer`` which C entries launched, and how often."""
import contextlib
import copy

import pytest
import torch

import _rowwave_forward_util as U
from flowconductor_amd import ops
from flowconductor_amd import transforms as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _worst_ratios():
    yield
    for entry, (ratio, label) in sorted(U.RATIOS.items()):
        print("worst max(e) / (4 max(f) + 1e-5) of %s: %.4f (%s)" % (entry, ratio, label))


def _run(fn, **expected):
    """``fn()`` without autograd; the launches of every entry of ``U.ENTRIES`` must be exactly ``expected``."""
    with torch.no_grad(), contextlib.ExitStack() as stack:
        timers = {name: stack.enter_context(ops.KernelTimer(name)) for name in U.ENTRIES}
        out = fn()
    launches = {name: len(timer.pairs) for name, timer in timers.items()}
    assert launches == {name: expected.get(name, 0) for name in U.ENTRIES}, launches
    return out


def _check(entry, label, got, ref32, ref64, **kw):
    """One quantity, or ``(y, logabsdet)``."""
    if isinstance(got, tuple):
        return U.check_pair(entry, label, got, ref32, ref64, **kw)
    return U.check(entry, label, got, ref32, ref64, **kw)


def _bit_equal(a, b, what):
    for got, ref in zip(a if isinstance(a, tuple) else (a,), b if isinstance(b, tuple) else (b,)):
        assert got.shape == ref.shape and torch.equal(got, ref), what


def _form(per_sample):
    return "per-sample" if per_sample else "shared"


FORMS = pytest.mark.parametrize("per_sample", (False, True), ids=_form)


# ---- a. widths -----------------------------------------------------------------------------------------------------------

@FORMS
@pytest.mark.parametrize("d,inst", U.PLANAR_WIDTHS, ids=lambda v: str(v))
def test_planar_widths(d, inst, per_sample, device):
    assert U.planar_instantiation(d) == inst
    for n in U.WIDTH_ROWS:
        inputs = U.planar_inputs(n, d, per_sample)
        on_device = [t.to(device) for t in inputs]
        got = _run(lambda: ops.planar(*on_device, per_sample=per_sample), fc_planar=1)
        _check(U.PLANAR, "%s %s d=%d n=%d" % (inst, _form(per_sample), d, n), got, *U.both(U.planar_ref, *inputs))


@FORMS
@pytest.mark.parametrize("d,k,inst", U.HOUSEHOLDER_WIDTHS, ids=lambda v: str(v))
def test_householder_widths(d, k, inst, per_sample, device):
    """The wide kernel: shared q (``householder``) and per-sample q (``householder_rows``, eight reflections requested at
    a time and one batch ahead), both orders; K = 0 returns the input bit for bit."""
    assert U.householder_instantiation(d) == inst
    for n in U.WIDTH_ROWS:
        x, q = U.householder_inputs(n, d, k, per_sample)
        xd, qd = x.to(device), q.to(device)
        for reverse in (False, True):
            got = _run(lambda: ops.householder(xd, qd, reverse=reverse), fc_householder=1)
            _check(U.HOUSEHOLDER, "%s %s d=%d K=%d n=%d reverse=%d" % (inst, _form(per_sample), d, k, n, reverse), got,
                   *U.both(U.householder_ref, x, q, reverse=reverse))
            if k == 0:
                _bit_equal(got.cpu(), x, "K = 0 must return the input")


@pytest.mark.parametrize("d,m,inst", U.SYLVESTER_SHARED_WIDTHS, ids=lambda v: str(v))
def test_sylvester_shared_widths(d, m, inst, device):
    assert U.sylvester_instantiation(d, False) == inst
    for n in U.WIDTH_ROWS:
        inputs = U.sylvester_inputs(n, d, m, False)
        on_device = [t.to(device) for t in inputs]
        got = _run(lambda: ops.sylvester(*on_device), fc_sylvester=1)
        _check(U.SYLVESTER, "%s d=%d M=%d n=%d" % (inst, d, m, n), got, *U.both(U.sylvester_ref, *inputs))


@pytest.mark.parametrize("d,m,inst", U.SYLVESTER_PER_SAMPLE_WIDTHS, ids=lambda v: str(v))
def test_sylvester_per_sample_widths(d, m, inst, device):
    """Row-major per-sample matrices with junk below the diagonal, which is never read."""
    assert U.sylvester_instantiation(d, True) == inst
    for n in (U.WIDE_PER_SAMPLE_ROWS if d >= 257 else U.WIDTH_ROWS):
        inputs = U.sylvester_inputs(n, d, m, True)
        assert d == 1 or float(torch.tril(inputs[2], -1).abs().max()) > 10.0
        on_device = [t.to(device) for t in inputs]
        got = _run(lambda: ops.sylvester(*on_device), fc_sylvester=1)
        _check(U.SYLVESTER, "%s d=%d M=%d n=%d" % (inst, d, m, n), got, *U.both(U.sylvester_ref, *inputs))


def test_shared_sylvester_multiplies_by_the_whole_matrix(device):
    """The contract of ``ops.sylvester``'s shared form: entries below the diagonal of R1 / R2 enter the outputs."""
    x, q, r1, r2, bias = U.sylvester_inputs(67, 40, 5, False)
    junk = torch.tril(torch.randn(40, 40, generator=torch.Generator().manual_seed(1)) * 0.3, -1)
    on_device = [t.to(device) for t in (x, q, r1 + junk, r2 + junk, bias)]
    got = _run(lambda: ops.sylvester(*on_device), fc_sylvester=1)
    _check(U.SYLVESTER, "shared form, full matrices", got, *U.both(U.sylvester_ref, x, q, r1 + junk, r2 + junk, bias))
    assert float((got[0].cpu().double() - U.sylvester_ref(x.double(), q.double(), r1.double(), r2.double(),
                                                          bias.double())[0]).abs().max()) > 1e-2


# ---- b. sweeps -----------------------------------------------------------------------------------------------------------

def _sweep_case(entry, shape, device):
    """``(call(rows) -> outputs of the rows ``rows`` sent on their own, (float32, float64) references)``."""
    n, d = shape["n"], shape["d"]
    if entry == U.HOUSEHOLDER:
        x, q = U.householder_inputs(n, d, shape["k"], False)
        xd, qd = x.to(device), q.to(device)
        return (lambda rows: ops.householder(xd[rows], qd)), U.both(U.householder_ref, x, q)
    if entry == U.PLANAR:
        inputs = U.planar_inputs(n, d, False)
        xd, wd, ud, bd = (t.to(device) for t in inputs)
        return (lambda rows: ops.planar(xd[rows], wd, ud, bd)), U.both(U.planar_ref, *inputs)
    inputs = U.sylvester_inputs(n, d, shape["m"], shape["per_sample"])
    on_device = [t.to(device) for t in inputs]
    if shape["per_sample"]:
        return (lambda rows: ops.sylvester(*[t[rows] for t in on_device])), U.both(U.sylvester_ref, *inputs)
    return (lambda rows: ops.sylvester(on_device[0][rows], *on_device[1:])), U.both(U.sylvester_ref, *inputs)


@pytest.mark.parametrize("name,entry,inst,sweeps,shape", U.SWEEP_CASES, ids=[c[0] for c in U.SWEEP_CASES])
def test_row_kernel_sweeps(name, entry, inst, sweeps, shape, device):
    """More wave-units than one sweep of the capped grid, the last sweep partial: every row within the bound, and the
    last sweep's rows bit-equal to the same rows sent on their own (rows are independent)."""
    n = shape["n"]
    count, first, partial = U.row_sweeps(inst, n)
    assert count == sweeps and partial and U.row_sweeps(inst, n - first)[0] == 1
    call, (ref32, ref64) = _sweep_case(entry, shape, device)
    whole = _run(lambda: call(slice(None)), **{entry: 1})
    _check(entry, "%s %s n=%d, %d sweeps" % (name, inst, n, count), whole, ref32, ref64)
    alone = _run(lambda: call(slice(first, n)), **{entry: 1})
    _bit_equal(tuple(t[first:] for t in whole) if isinstance(whole, tuple) else whole[first:], alone,
               "rows %d.. of %s differ from the same rows on their own" % (first, name))


def _mm_call(t, device):
    """``(module on the device, call(x on the device) -> ops.sylvester_mm with the module's folded weights)``."""
    td = copy.deepcopy(t).to(device)
    with torch.no_grad():
        w1, w2, rdiag = td._mm_weights()
    return td, lambda x: ops.sylvester_mm(x, w1, w2, td.bias, rdiag)


@pytest.mark.parametrize("d,m,inst", U.SYLVESTER_MM_WIDTHS, ids=lambda v: str(v))
def test_sylvester_mm_sweeps(d, m, inst, device):
    """One full sweep of the device's grid plus 16 rows: the waves of the first workgroup run their loop twice (``znext``,
    ``grp += nwaves``); the last 16 rows are bit-equal to the same rows in a launch of their own."""
    cus = torch.cuda.get_device_properties(device).multi_processor_count
    full = U.sylvester_mm_full_sweep_rows(d, cus)
    n = full + 16
    grid, sweep, sweeps, partial = U.sylvester_mm_plan(n, d, cus)
    assert (sweep, sweeps, partial) == (full, 2, True) and U.sylvester_mm_instantiation(d) == inst
    t = U.sylvester_module(d, m, seed=d)
    x = U.mm_rows(n, d, 11)
    td, call = _mm_call(t, device)
    xd = x.to(device)
    whole = _run(lambda: call(xd), fc_sylvester_mm=1)
    _check(U.SYLVESTER_MM, "%s n=%d, two sweeps of %d workgroups" % (inst, n, grid), whole, *U.module_refs(t, x))
    alone = _run(lambda: call(xd[full:]), fc_sylvester_mm=1)
    _bit_equal(tuple(v[full:] for v in whole), alone, "the second sweep's rows differ from the same rows on their own")


# ---- c. fc_sylvester_mm edges ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", U.SYLVESTER_MM_EDGE_ROWS)
@pytest.mark.parametrize("d,m,inst", U.SYLVESTER_MM_WIDTHS, ids=lambda v: str(v))
def test_sylvester_mm_block_counts(d, m, inst, n, device):
    """One block (seven idle waves), nine (a second workgroup with one live wave) and 23 (odd, three workgroups)."""
    t = U.sylvester_module(d, m, seed=d + 1)
    x = U.mm_rows(n, d, 12)
    td, call = _mm_call(t, device)
    got = _run(lambda: call(x.to(device)), fc_sylvester_mm=1)
    _check(U.SYLVESTER_MM, "%s n=%d" % (inst, n), got, *U.module_refs(t, x))


@pytest.mark.parametrize("d,m,inst", U.SYLVESTER_MM_WIDTHS, ids=lambda v: str(v))
def test_sylvester_module_body_and_tail(d, m, inst, device):
    """n = 1024 + 5 through SylvesterTransform: the body in one fc_sylvester_mm launch, the tail in one fc_sylvester launch,
    each within the bound on its own and the rows in order."""
    t = U.sylvester_module(d, m, seed=d + 2)
    x = U.mm_rows(U.SEAM_ROWS, d, 13)
    td = copy.deepcopy(t).to(device)
    got = _run(lambda: td(x.to(device)), fc_sylvester_mm=1, fc_sylvester=1)
    assert got[0].shape == (U.SEAM_ROWS, d) and got[1].shape == (U.SEAM_ROWS,)
    ref32, ref64 = U.module_refs(t, x)
    _check(U.SYLVESTER_MM, "module d=%d body" % d, got, ref32, ref64, rows=slice(0, 1024))
    _check(U.SYLVESTER, "module d=%d tail (%s)" % (d, U.sylvester_instantiation(d, False)), got, ref32, ref64,
           rows=slice(1024, U.SEAM_ROWS))


@pytest.mark.parametrize("d,m", ((64, 16), (128, 32)))
def test_sylvester_mm_strained_operands(d, m, device):
    """The strain rows of test_gpu_linear.py::test_split_f16_route_inputs, each group held to the bound on its own, and
    ordinary rows that share a 16-row tile with rows holding 7e4: the operand scale is the row's, not the tile's."""
    t = U.sylvester_module(d, m, seed=d + 3)
    x = U.strain_rows(d, 14)
    td, call = _mm_call(t, device)
    got = _run(lambda: call(x.to(device)), fc_sylvester_mm=1)
    ref32, ref64 = U.module_refs(t, x)
    for name, rows in U.STRAIN_GROUPS.items():
        _check(U.SYLVESTER_MM, "strain d=%d %s" % (d, name), got, ref32, ref64, rows=rows)


@pytest.mark.parametrize("d,m,inst", U.SYLVESTER_MM_WIDTHS, ids=lambda v: str(v))
def test_sylvester_mm_saturated_tanh(d, m, inst, device):
    t = U.sylvester_module(d, m, seed=d + 4)
    x = U.mm_rows(U.SEAM_ROWS - 5, d, 15, scale=40.0)
    td, call = _mm_call(t, device)
    got = _run(lambda: call(x.to(device)), fc_sylvester_mm=1)
    _check(U.SYLVESTER_MM, "%s inputs times 40" % inst, got, *U.module_refs(t, x))


@pytest.mark.parametrize("d", (32, 64, 96, 128))
def test_near_singular_sylvester_layer(d, device):
    """diag(R1) diag(R2) ~ -0.9987 on half of the features: the logarithm's argument comes close to zero.  On the
    matrix-core kernel and on the row kernel."""
    t = U.sylvester_module(d, 8, seed=7, near_singular=True)
    x = U.mm_rows(U.SEAM_ROWS - 5, d, 8)
    ref32, ref64 = U.module_refs(t, x)
    td, call = _mm_call(t, device)
    xd = x.to(device)
    got = _run(lambda: call(xd), fc_sylvester_mm=1)
    _check(U.SYLVESTER_MM, "near-singular d=%d" % d, got, ref32, ref64)
    got = _run(lambda: ops.sylvester(xd, td.Q_orth.q_vectors, td._create_R1(), td._create_R2(), td.bias), fc_sylvester=1)
    _check(U.SYLVESTER, "near-singular d=%d" % d, got, ref32, ref64)


def test_parameter_update_reaches_the_folded_weights(device):
    """After a forward every parameter is changed in place without a graph, as an optimizer step does: the next forward is
    the float64 result of the NEW parameters (the folded weights are memoised per parameter version)."""
    d, m, n = 64, 16, 1024
    td = U.sylvester_module(d, m, seed=21).to(device)
    x = U.mm_rows(n, d, 16)
    xd = x.to(device)
    before = _run(lambda: td(xd), fc_sylvester_mm=1)
    _check(U.SYLVESTER_MM, "before the update", before, *U.module_refs(td, x))
    g = torch.Generator().manual_seed(22)
    with torch.no_grad():
        for p in td.parameters():
            p.add_((torch.randn(p.shape, generator=g) * 0.2).to(device))
    after = _run(lambda: td(xd), fc_sylvester_mm=1)
    assert float((after[0] - before[0]).abs().max()) > 1e-2
    _check(U.SYLVESTER_MM, "after the update", after, *U.module_refs(td, x))


# ---- d. non-finite rows stay in their row ------------------------------------------------------------------------------------

def _poisoned(entry, label, call, reference, x, nan_row, inf_row):
    """One row of NaN and one row holding an Inf among ordinary rows: every other row bit-equal to the run with those two
    rows zeroed, the two rows non-finite only where float64 is, and both runs within the bound."""
    bad, zeroed = U.poison(x, nan_row, inf_row)
    got_bad = _run(lambda: call(bad), **{entry: 1})
    got_zeroed = _run(lambda: call(zeroed), **{entry: 1})
    others = torch.ones(x.shape[0], dtype=torch.bool)
    others[[nan_row, inf_row]] = False
    pick = lambda out: tuple(t.cpu()[others] for t in (out if isinstance(out, tuple) else (out,)))      # noqa: E731
    _bit_equal(pick(got_bad), pick(got_zeroed), "%s: a non-finite row changed another row" % label)
    _check(entry, label + " poisoned", got_bad, *reference(bad), poisoned=True)
    _check(entry, label + " zeroed", got_zeroed, *reference(zeroed))


def test_sylvester_mm_non_finite_rows(device):
    """The MFMA carries 16 samples per tile."""
    t = U.sylvester_module(64, 16, seed=64)
    td, call = _mm_call(t, device)
    _poisoned(U.SYLVESTER_MM, "sylvester_mm d=64", lambda x: call(x.to(device)), lambda x: U.module_refs(t, x),
              U.mm_rows(64, 64, 4), 5, 21)


@FORMS
def test_narrow_householder_non_finite_rows(per_sample, device):
    """Four samples per wave, one per 16-lane row."""
    x, q = U.householder_inputs(67, 5, 3, per_sample)
    qd = q.to(device)
    _poisoned(U.HOUSEHOLDER, "householder_narrow_kernel %s" % _form(per_sample), lambda v: ops.householder(v.to(device), qd),
              lambda v: U.both(U.householder_ref, v, q), x, 5, 10)


@FORMS
@pytest.mark.parametrize("d,lanes", ((16, 4), (64, 16)))
def test_planar_rows4_non_finite_rows(d, lanes, per_sample, device):
    """64 / L samples per wave."""
    assert U.planar_instantiation(d) == "planar_rows4_kernel<%d>" % lanes
    x, w, u, b = U.planar_inputs(67, d, per_sample)
    wd, ud, bd = w.to(device), u.to(device), b.to(device)
    _poisoned(U.PLANAR, "planar_rows4_kernel<%d> %s" % (lanes, _form(per_sample)),
              lambda v: ops.planar(v.to(device), wd, ud, bd, per_sample=per_sample),
              lambda v: U.both(U.planar_ref, v, w, u, b), x, 5, 10)


# ---- e. alignment --------------------------------------------------------------------------------------------------------------

def _off_by_four_bytes(x, device):
    """The rows of ``x`` as a contiguous device view that starts 4 bytes into its buffer."""
    buffer = torch.empty(x.numel() + 1, dtype=torch.float32, device=device)
    view = buffer[1:].view(x.shape)
    view.copy_(x)
    assert view.is_contiguous() and view.data_ptr() % 16 == 4
    return view


@pytest.mark.parametrize("d", (64, 256))
def test_planar_on_an_unaligned_view(d, device):
    """The float4 kernel needs 16-byte rows: such a view takes the scalar kernel, and gives the aligned run's result within
    the bound."""
    inputs = U.planar_inputs(67, d, False)
    x, w, u, b = (t.to(device) for t in inputs)
    refs = U.both(U.planar_ref, *inputs)
    view = _off_by_four_bytes(inputs[0], device)
    _check(U.PLANAR, "d=%d unaligned view (%s)" % (d, U.planar_instantiation(d, aligned16=False)),
           _run(lambda: ops.planar(view, w, u, b), fc_planar=1), *refs)
    _check(U.PLANAR, "d=%d aligned (%s)" % (d, U.planar_instantiation(d)), _run(lambda: ops.planar(x, w, u, b), fc_planar=1),
           *refs)


def test_sylvester_module_on_an_unaligned_view(device):
    d, m = 64, 16
    t = U.sylvester_module(d, m, seed=31)
    x = U.mm_rows(U.SEAM_ROWS, d, 17)
    td = copy.deepcopy(t).to(device)
    view = _off_by_four_bytes(x, device)
    got = _run(lambda: td(view), fc_sylvester_mm=1, fc_sylvester=1)
    _check(U.SYLVESTER_MM, "module on an unaligned view", got, *U.module_refs(t, x))


# ---- f. modules ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("d", (64, 130))
def test_planar_module_with_an_active_constraint(d, device):
    """w . u = -3 < -1: ``get_constrained_u`` changes u.  Against planar.py:30-69 written out in float64."""
    x, w, u, b = U.planar_module_inputs(d, U.SEAM_ROWS)
    t = T.PlanarTransform(features=d)
    with torch.no_grad():
        t.w.copy_(w)
        t.u.copy_(u)
        t.b.copy_(b)
    td = t.to(device)
    got = _run(lambda: td(x.to(device)), fc_planar=1)
    _check(U.PLANAR, "PlanarTransform d=%d (%s)" % (d, U.planar_instantiation(d)), got,
           *U.both(U.planar_module_ref, x, w, u, b))


@pytest.mark.parametrize("inverse", (False, True))
def test_householder_sequence_body_and_tail(inverse, device):
    """n = 1024 + 5 at d = 64: a dense body on the matrix cores and a row-kernel tail."""
    d, k = 64, 9
    x, q = U.householder_inputs(U.SEAM_ROWS, d, k, False)
    t = T.HouseholderSequence(features=d, num_transforms=k)
    with torch.no_grad():
        t.q_vectors.copy_(q)
    td = t.to(device)
    got, lad = _run(lambda: (td.inverse if inverse else td)(x.to(device)), fc_dense_mm=1, fc_householder=1)
    assert lad.shape == (U.SEAM_ROWS,) and float(lad.abs().max()) == 0.0
    ref32, ref64 = U.both(U.householder_ref, x, q, reverse=inverse)
    body, tail = slice(0, 1024), slice(1024, U.SEAM_ROWS)
    U.check(U.DENSE_MM, "HouseholderSequence body inverse=%d" % inverse, got[body], ref32[body], ref64[body])
    U.check(U.HOUSEHOLDER, "HouseholderSequence tail inverse=%d" % inverse, got[tail], ref32[tail], ref64[tail])
