"""Row-wise error bound for the one-launch autoregressive samplers, shared by tests/test_ar_sampler_bounds_host.py and
tests/test_gpu_ar_sampler_rows.py, with the cases both files run.

The rows of an autoregressive inverse are independent, so the errors of the rows form a population whose median and upper
quantiles are statistics of the arithmetic that produced them, not of one unlucky row.  ``check_routes`` compares that
population with the float32 oracle's on the very same rows:

    e_y[r] = max_j |got[r, j] - y64[r, j]| / max(1, max_j |y64[r, j]|)
    e_l[r] = |got_lad[r] - lad64[r]| / max(1, |lad64[r]|)
    f_y, f_l: the same two quantities for the float32 oracle

    Q_p(e) <= 4 Q_p(f) + 2^-23        for p in {0.5, 0.9, 0.99}
    max(e) <= 4 max(f) + 1e-5         (the rule of tests/test_gpu_golden.py::_check, relative to the row)
    got is finite wherever the float64 oracle is

The multiple 4 is the suite's own (test_gpu_golden.py: the largest multiple any fixture needs is 3.4); 2^-23 is one ulp of
the row's scale: the oracle's median can sit at half an ulp where another order of summation legitimately lands at one.
Neither number is fitted to a kernel.  The fixture conditions are asserted on the reference alone."""
import copy

import torch

from oracle import torch_oracle as O

QUANTILES = (0.5, 0.9, 0.99)
MULTIPLE = 4.0
ULP = 2.0 ** -23
MAX_SLACK = 1e-5
LARGE_ROW = 1e3          # a row whose float64 inverse exceeds this ...
LARGE_ROW_SHARE = 0.01   # ... is allowed for at most this share of the rows
ROWS = 2053              # not a whole 16-row block, enough rows for a 99 % quantile

# ---- the cases: (family, form, bins / sigmoids or None, D, hidden, context features or None, blocks, seed, parameter scale) --
# The smallest set that spans the kernels' template axes: one or two k-steps of the initial layer (D <= 32 / D > 32), every
# parameter-tile count, 0-3 blocks, hidden < 64.  Seeds and inputs are those of test_gpu_ar_inverse.py (features + hidden),
# test_gpu_ar_inverse_context.py and test_gpu_ar_device_loop_forms.py (its CASES table).
CASES = [
    ("affine", "maf", None, 6, 64, None, 2, 70, 1.5),
    ("affine", "maf", None, 2, 4, None, 2, 6, 1.5),                 # the README flow's layer
    ("affine", "maf", None, 40, 50, None, 2, 90, 1.5),
    ("affine", "maf", None, 64, 64, None, 3, 128, 1.5),
    ("affine", "maf", None, 9, 16, None, 1, 25, 1.5),
    ("rq", "rq_tails", 8, 6, 64, None, 2, 70, 1.5),
    ("rq", "rq_tails", 8, 33, 24, None, 2, 57, 1.5),
    ("rq", "rq_box", 10, 8, 64, None, 2, 72, 1.5),
    ("rq", "rq_tails", 16, 7, 32, None, 2, 39, 1.5),
    ("rq", "rq_tails", 4, 64, 64, None, 3, 128, 1.5),
    ("rq", "rq_box", 5, 5, 24, None, 0, 29, 1.5),
    ("context", "maf", None, 8, 64, 4, 2, 72, 1.5),
    ("context", "maf", None, 33, 40, 32, 1, 73, 1.5),
    ("context", "rq_tails", 8, 8, 64, 4, 2, 72, 1.5),
    ("sos", "sos", 6, 6, 64, None, 2, 70, 1.5),
    ("sos", "sos", 30, 8, 64, None, 2, 72, 1.5),
    ("sos", "sos", 10, 40, 50, None, 2, 90, 1.5),
    ("spline", "linear", 8, 6, 64, None, 2, 70, 1.5),
    ("spline", "linear", 20, 33, 24, None, 2, 57, 1.5),
    ("spline", "quadratic_tails", 6, 6, 64, None, 2, 2, 1.5),
    ("spline", "quadratic", 10, 5, 24, None, 2, 1, 1.5),
    ("spline", "cubic", 6, 6, 64, None, 2, 4, 1.5),
    ("spline", "cubic", 10, 9, 16, None, 1, 2, 1.5),
]
# the two-blocks-per-wave route: one shape per entry whose pair instantiation exists (fc_made_inverse.h
# ``mi_*_pairs_fit_registers``), and one whose table entry drops the pair
PAIR_CASES = [
    ("affine", "maf", None, 6, 64, None, 2, 70, 1.5),
    ("affine", "maf", None, 40, 50, None, 2, 90, 1.5),
    ("rq", "rq_tails", 8, 6, 64, None, 2, 70, 1.5),
    ("rq", "rq_tails", 16, 7, 32, None, 2, 39, 1.5),
    ("context", "maf", None, 8, 64, 4, 2, 72, 1.5),
    ("sos", "sos", 6, 6, 64, None, 2, 70, 1.5),
    ("spline", "linear", 8, 6, 64, None, 2, 70, 1.5),
    ("spline", "quadratic_tails", 6, 6, 64, None, 2, 2, 1.5),
    ("spline", "cubic", 6, 6, 64, None, 2, 4, 1.5),
]
NO_PAIR_CASE = ("spline", "cubic", 10, 40, 50, None, 2, 90, 1.5)
ENTRY = {"affine": "fc_made_inverse", "rq": "fc_made_inverse", "context": "fc_made_inverse_context",
         "sos": "fc_made_inverse_sos", "spline": "fc_made_inverse_spline"}


def case_id(case):
    family, form, k, features, hidden, ctx, blocks = case[:7]
    return "%s-%s%s-D%d-H%d%s-b%d" % (family, form, "" if k is None else "-k%d" % k, features, hidden,
                                      "" if ctx is None else "-ctx%d" % ctx, blocks)


def build(case):
    """The case's layer on the CPU, in eval mode, its parameters times the case's scale."""
    from flowconductor_amd import transforms as T

    family, form, k, features, hidden, ctx, blocks, seed, scale = case
    torch.manual_seed(seed)
    kw = dict(num_blocks=blocks)
    if ctx is not None:
        kw["context_features"] = ctx
    if form == "maf":
        t = T.MaskedAffineAutoregressiveTransform(features, hidden, **kw)
    elif form in ("rq_tails", "rq_box"):
        t = T.MaskedPiecewiseRationalQuadraticAutoregressiveTransform(
            features, hidden, num_bins=k, tails="linear" if form == "rq_tails" else None, tail_bound=3.0, **kw)
    elif form == "sos":
        t = T.MaskedSumOfSigmoidsTransform(features, hidden, n_sigmoids=k, **kw)
    elif form == "linear":
        t = T.MaskedPiecewiseLinearAutoregressiveTransform(k, features, hidden, **kw)
    elif form == "quadratic_tails":
        t = T.MaskedPiecewiseQuadraticAutoregressiveTransform(k, features, hidden, tails="linear", tail_bound=3.0, **kw)
    elif form == "quadratic":
        t = T.MaskedPiecewiseQuadraticAutoregressiveTransform(k, features, hidden, **kw)
    elif form == "cubic":
        t = T.MaskedPiecewiseCubicAutoregressiveTransform(k, features, hidden, **kw)
    else:
        raise KeyError(form)
    t = t.eval()
    with torch.no_grad():
        for p in t.parameters():
            p.mul_(scale)
    return t


def inputs(case, n):
    """``(x [n, D], context [n, C] or None)``: the inputs of the existing files' ``_inputs``."""
    form, features, ctx = case[1], case[3], case[5]
    g = torch.Generator().manual_seed(5)
    if form in ("linear", "quadratic", "cubic"):
        x = torch.rand(n, features, generator=g) * 0.98 + 0.01
    elif form == "rq_box":
        x = torch.rand(n, features, generator=g) * 2.2 - 1.1
    elif form == "sos":
        x = torch.randn(n, features, generator=g) * 0.6
    else:
        x = torch.randn(n, features, generator=g) * 1.2
    return x, (None if ctx is None else torch.randn(n, ctx, generator=g))


def oracle(t, x, context=None):
    """The oracle's inverse of the CPU layer ``t`` on ``x`` in float32 and float64: ``(y32, lad32, y64, lad64)``."""
    with torch.no_grad():
        y32, lad32 = O.transform_apply(t, x.clone(), context, inverse=True)
        y64, lad64 = O.transform_apply(copy.deepcopy(t).double(), x.double(), None if context is None else context.double(),
                                       inverse=True)
    return y32, lad32, y64, lad64


_REFS = {}


def references(case, n=ROWS):
    """``(layer on the CPU, x, context, (y32, lad32, y64, lad64))`` of a case; computed once and never changed."""
    key = (case, n)
    if key not in _REFS:
        t = build(case)
        x, context = inputs(case, n)
        _REFS[key] = (t, x, context, oracle(t, x, context))
    t, x, context, refs = _REFS[key]
    return copy.deepcopy(t), x.clone(), None if context is None else context.clone(), refs


def _f64(t):
    return t.detach().cpu().double()


def row_error(got, ref64):
    """Per-row error of one quantity, ``[N, H]`` or ``[N]``, relative to the row's own scale (float64, on the CPU)."""
    got, ref64 = _f64(got), _f64(ref64)
    if ref64.dim() == 1:
        return (got - ref64).abs() / ref64.abs().clamp(min=1.0)
    return (got - ref64).abs().amax(dim=1) / ref64.abs().amax(dim=1).clamp(min=1.0)


def row_errors(y, lad, y64, lad64):
    """``(e_y, e_l)``: per-row errors relative to the row's own scale (float64, on the CPU)."""
    return row_error(y, y64), row_error(lad, lad64)


def summary(e):
    """p50 / p90 / p99 / max of a row-error population."""
    q = torch.quantile(e, torch.tensor(QUANTILES, dtype=e.dtype))
    return tuple(float(v) for v in q) + (float(e.max()),)


def check_fixture(y64, lad64):
    """Conditions on the reference alone: an ill-conditioned fixture makes any bound vacuous."""
    y64, lad64 = _f64(y64), _f64(lad64)
    assert bool(torch.isfinite(y64).all()) and bool(torch.isfinite(lad64).all()), "fixture: non-finite float64 oracle"
    share = float((y64.abs().amax(dim=1) > LARGE_ROW).double().mean())
    assert share <= LARGE_ROW_SHARE, "fixture: %.2f %% of the rows exceed %g in float64" % (100 * share, LARGE_ROW)


def quantity_violations(what, got, ref32, ref64):
    """The bound on ONE quantity (``[N, H]`` or ``[N]``, the float64 reference finite): ``(messages of the violated
    conditions, (got's summary, float32 oracle's summary))``."""
    se, sf = summary(row_error(got, ref64)), summary(row_error(ref32, ref64))
    bad = []
    if not bool(torch.isfinite(_f64(got)).all()):
        bad.append("%s: non-finite output where the float64 oracle is finite" % what)
    for name, e, f in zip(("p50", "p90", "p99"), se, sf):
        if not e <= MULTIPLE * f + ULP:
            bad.append("%s %s: %.3g > 4 x %.3g + 2^-23" % (what, name, e, f))
    if not se[3] <= MULTIPLE * sf[3] + MAX_SLACK:
        bad.append("%s max: %.3g > 4 x %.3g + 1e-5" % (what, se[3], sf[3]))
    return bad, (se, sf)


def violations(got_y, got_lad, y32, lad32, y64, lad64):
    """``(messages of the violated conditions, {what: (got's summary, float32 oracle's summary)})``."""
    bad, stats = [], {}
    for what, got, ref32, ref64 in (("y", got_y, y32, y64), ("lad", got_lad, lad32, lad64)):
        b, stats[what] = quantity_violations(what, got, ref32, ref64)
        bad += b
    return bad, stats


def format_stats(label, stats):
    return "  ".join("%s %s p50 %.2e p90 %.2e p99 %.2e max %.2e (f32 oracle %.2e %.2e %.2e %.2e)"
                     % ((label, what) + stats[what][0] + stats[what][1]) for what in stats)


def check_routes(label, routes, y32, lad32, y64, lad64):
    """``routes``: name -> ``(y, lad)``.  Asserts the fixture conditions, then the row-wise bound on every route, each
    against float64 (never against each other); every route's line is printed before any is judged."""
    check_fixture(y64, lad64)
    assert bool(torch.isfinite(_f64(y32)).all()) and bool(torch.isfinite(_f64(lad32)).all()), \
        "fixture: non-finite float32 oracle"
    failures = []
    for route, (y, lad) in routes.items():
        bad, stats = violations(y, lad, y32, lad32, y64, lad64)
        print(format_stats("%s [%s]" % (label, route), stats))
        failures += ["%s: %s" % (route, b) for b in bad]
    assert not failures, "%s: %s" % (label, "; ".join(failures))
