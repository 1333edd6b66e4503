"""The row-wise bound of tests/_ar_sampler_util.py has teeth: on the oracle alone (no GPU), for every case of
tests/test_gpu_ar_sampler_rows.py, the float32 oracle passes as "got" and three subtly wrong outputs are rejected --
two of which the batch-maximum bound of the older device-loop tests lets through."""
import pytest
import torch

import _ar_sampler_util as U
from _util import maxdiff


def _old_bound_accepts(y, lad, y32, lad32, y64, lad64):
    """The bound of test_gpu_ar_inverse.py, test_gpu_ar_inverse_context.py and test_gpu_ar_device_loop_forms.py, copied
    here as the thing the row-wise bound replaces: maxima over the whole batch, so one ill-conditioned row sets the
    allowance of all the others."""
    tol_y = 1e-4 * max(1.0, float(y32.abs().max())) + 4 * maxdiff(y32, y64)
    tol_l = 1e-3 * max(1.0, float(lad32.abs().max()) / 10) + 4 * maxdiff(lad32, lad64)
    return maxdiff(y, y64) <= tol_y and maxdiff(lad, lad64) <= tol_l


def _mutants(y32, lad32, y64, lad64):
    """``name -> (y, lad, must the old bound accept it)``: the float32 oracle's output, wrong in a way a kernel can be."""
    rowscale = y64.abs().amax(dim=1).clamp(min=1.0)
    last = y32.shape[1] - 1
    # 1. the last column slightly off on every row (a wrong last pass, a dropped bias in the padded units)
    y1 = y32.double().clone()
    y1[:, last] += 3e-6 * rowscale
    # 2. the last column clearly off on 2 % of the rows (a bin edge off by one in a single parameter tile)
    y2 = y32.double().clone()
    hit = torch.arange(y32.shape[0]) % 50 == 7
    y2[hit, last] += 1e-4 * rowscale[hit]
    # 3. every log-determinant slightly off
    lad3 = lad32.double() + 3e-5 * lad64.abs().clamp(min=1.0)
    return {"last_column_every_row": (y1, lad32, True), "last_column_2_percent": (y2, lad32, None),
            "logabsdet_every_row": (y32, lad3, True)}


# Every case of the GPU file but the sum of sigmoids at D = 40: the oracle's root search there (40 passes over 40 columns in
# two precisions) takes most of a minute on the CPU; the family keeps its two other cases here, and the GPU file asserts the
# fixture conditions of that case like those of every other.
HOST_CASES = [c for c in U.CASES + [U.NO_PAIR_CASE] if not (c[1] == "sos" and c[3] == 40)]


@pytest.mark.parametrize("case", HOST_CASES, ids=U.case_id)
def test_row_wise_bound_rejects_what_the_batch_maximum_accepts(case):
    _, _, _, (y32, lad32, y64, lad64) = U.references(case)
    assert y64.shape == (U.ROWS, case[3])
    # the float32 oracle as "got": passes, fixture conditions included
    U.check_routes(U.case_id(case), {"float32 oracle": (y32, lad32)}, y32, lad32, y64, lad64)
    assert _old_bound_accepts(y32, lad32, y32, lad32, y64, lad64)
    for name, (y, lad, old_accepts) in _mutants(y32, lad32, y64, lad64).items():
        bad, stats = U.violations(y, lad, y32, lad32, y64, lad64)
        print(U.format_stats(name, stats))
        assert bad, "%s slipped through the row-wise bound: the fixture is too ill-conditioned to test anything" % name
        if old_accepts:
            assert _old_bound_accepts(y, lad, y32, lad32, y64, lad64), "%s: the old bound was expected to accept it" % name


def test_bound_on_hand_made_populations():
    """The helper's arithmetic on errors whose quantiles are known."""
    n = 1000
    y64 = torch.zeros(n, 3, dtype=torch.float64)
    y64[:, 0] = torch.linspace(0.5, 200.0, n, dtype=torch.float64)
    lad64 = torch.linspace(-30.0, 30.0, n, dtype=torch.float64)
    scale = y64.abs().amax(dim=1).clamp(min=1.0)
    y32 = y64.clone()
    y32[:, 1] += 1e-7 * scale                      # the reference: 1e-7 of every row's scale
    lad32 = lad64 + 1e-7 * lad64.abs().clamp(min=1.0)
    e_y, e_l = U.row_errors(y32, lad32, y64, lad64)
    assert torch.allclose(e_y, torch.full_like(e_y, 1e-7), rtol=1e-6) and torch.allclose(e_l, torch.full_like(e_l, 1e-7), rtol=1e-6)
    assert U.summary(e_y) == pytest.approx((1e-7,) * 4, rel=1e-6)
    assert not U.violations(y32, lad32, y32, lad32, y64, lad64)[0]
    # just inside 4 x + one ulp of the row, just outside
    for factor, ok in ((3.9, True), (5.3, False)):
        y = y64.clone()
        y[:, 2] -= (factor * 1e-7 + (U.ULP if ok else 0.0)) * scale
        assert (not U.violations(y, lad32, y32, lad32, y64, lad64)[0]) == ok
    # one row at 4 x + 1e-5 passes, a little more does not; a NaN never does
    for extra, ok in ((0.99e-5, True), (1.2e-5, False), (float("nan"), False)):
        y = y32.clone()
        y[17, 1] = y64[17, 1] + (4e-7 + extra) * scale[17]
        assert (not U.violations(y, lad32, y32, lad32, y64, lad64)[0]) == ok
    # fixture conditions: more than 1 % of the rows beyond 1e3, a non-finite reference
    far = y64.clone()
    far[:11, 0] = 2e3
    with pytest.raises(AssertionError, match="fixture"):
        U.check_fixture(far, lad64)
    far[11:, 0] = 1.0
    far[10, 0] = 1.0
    U.check_fixture(far, lad64)
    with pytest.raises(AssertionError, match="fixture"):
        U.check_fixture(y64, lad64 * float("inf"))
