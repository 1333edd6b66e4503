"""What the six device-loop entries (fc_made_inverse, _context, _sos, _spline, fc_made_mog_sample, _context) answer before
they touch the device: every refusal is hipErrorInvalidValue (1), and an empty batch with valid sizes is a success (0)
before any pointer is looked at.  All of it is decided on the host, so the rows below run without a GPU; none of them is a
tuple that launches: every row is refused by an argument check, or has ``n == 0``."""
import ctypes

import pytest

from flowconductor_amd import _hip

_BUF = ctypes.create_string_buffer(4096)
PTR = (ctypes.addressof(_BUF) + 63) & ~63          # a 64-byte aligned, non-null address (never read: nothing launches)
OFF4 = PTR + 4                                      # the same, 4 bytes off the 16-byte alignment

STACK = ["hidden_frag", "hidden_unscale", "hidden_bias", "final_frag", "final_unscale", "final_bias"]
CONTEXT = ["context", "context_frag", "context_unscale", "context_bias"]
ALIGNED = ["hidden_frag", "final_frag", "final_bias"]


def _rq(num_bins=8, tails=1):
    return _hip.RQConfig(num_bins=num_bins, tails=tails, left=-3.0, right=3.0, bottom=-3.0, top=3.0, min_bin_width=1e-3,
                         min_bin_height=1e-3, min_derivative=1e-3, wh_divisor=1.0, softplus_beta=1.0)


def _spline(kind, num_bins, tails=0):
    return _hip.SplineConfig(kind=kind, num_bins=num_bins, tails=tails, inverse=1, left=0.0, right=1.0, bottom=0.0, top=1.0,
                             min_bin_width=1e-3, min_bin_height=1e-3, width_divisor=1.0, height_divisor=1.0)


LINEAR, QUADRATIC, CUBIC = 0, 1, 2

# entry -> (argument names in the order of the C signature, a tuple that passes every check: it is only ever called with one
# of its values replaced, see `_call`)
_SIZES = dict(n=16, d=6, num_blocks=2)
ENTRIES = {
    "fc_made_inverse": (
        ["z", "y", "logabsdet"] + STACK + ["units_needed", "err_flag", "n", "d", "num_blocks", "params_per_dim", "kind", "cfg",
                                            "stream"],
        dict(_SIZES, params_per_dim=2, kind=0, cfg=None)),
    "fc_made_inverse_context": (
        ["z", "context", "y", "logabsdet"] + STACK[:3] + CONTEXT[1:] + STACK[3:] + [
            "units_needed", "err_flag", "n", "d", "context_features", "num_blocks", "params_per_dim", "kind", "cfg", "stream"],
        dict(_SIZES, context_features=3, params_per_dim=2, kind=0, cfg=None)),
    "fc_made_inverse_sos": (
        ["z", "y", "logabsdet"] + STACK + ["units_needed", "err_flag", "n", "d", "num_blocks", "n_sigmoids", "iterations", "lim",
                                            "offset", "log_scale_postact", "lad_flags", "stream"],
        dict(_SIZES, n_sigmoids=6, iterations=50, lim=120.0, offset=0.5, log_scale_postact=0.0, lad_flags=0)),
    "fc_made_inverse_spline": (
        ["z", "y", "logabsdet"] + STACK + ["units_needed", "err_flag", "n", "d", "num_blocks", "cfg", "lad_flags", "stream"],
        dict(_SIZES, cfg=_spline(LINEAR, 8), lad_flags=0)),
    "fc_made_mog_sample": (
        ["normal", "uniform", "x", "logp"] + STACK + ["units_needed", "n", "d", "num_blocks", "c", "epsilon", "stream"],
        dict(_SIZES, c=5, epsilon=1e-2)),
    "fc_made_mog_sample_context": (
        ["normal", "uniform", "context", "x", "logp"] + STACK[:3] + CONTEXT[1:] + STACK[3:] + [
            "units_needed", "n", "d", "context_features", "num_blocks", "c", "epsilon", "stream"],
        dict(_SIZES, context_features=3, c=5, epsilon=1e-2)),
}
RQ_ENTRIES = ["fc_made_inverse", "fc_made_inverse_context"]
MOG_ENTRIES = ["fc_made_mog_sample", "fc_made_mog_sample_context"]
CONTEXT_ENTRIES = ["fc_made_inverse_context", "fc_made_mog_sample_context"]
RQ23 = dict(params_per_dim=23, kind=1)      # K = 8 with linear tails: 3K - 1


def _pointers(entry):
    """Names of the entry's device pointers that must not be null (``units_needed`` and ``err_flag`` may be)."""
    names, _ = ENTRIES[entry]
    return [a for a in names if a in STACK + CONTEXT + ["z", "y", "logabsdet", "normal", "uniform", "x", "logp"]]


@pytest.fixture(scope="module")
def lib():
    lib = ctypes.CDLL(_hip.LIB_PATH)
    for name in ENTRIES:
        fn = getattr(lib, name)
        fn.argtypes = _hip.SIGNATURES[name]
        fn.restype = ctypes.c_int
    return lib


def _call(lib, entry, **changed):
    """The entry on its valid tuple with ``changed`` put in; ``pointers=None`` nulls every device pointer."""
    assert changed, "the unchanged tuple would launch"
    names, values = ENTRIES[entry]
    values = dict(values, stream=None, units_needed=PTR, err_flag=PTR)
    values.update({p: changed.get("pointers", PTR) for p in _pointers(entry)})
    changed.pop("pointers", None)
    assert set(changed) <= set(names), "not an argument of %s: %s" % (entry, sorted(set(changed) - set(names)))
    values.update(changed)
    cfg = values.get("cfg")
    if cfg is not None:
        values["cfg"] = ctypes.byref(cfg)
    return getattr(lib, entry)(*[values[a] for a in names])


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_sizes_every_entry_refuses(lib, entry):
    for change in (dict(d=0), dict(d=65), dict(num_blocks=-1), dict(num_blocks=4), dict(n=-16), dict(n=17)):
        assert _call(lib, entry, **change) == 1, change
        assert _call(lib, entry, pointers=None, **change) == 1, change


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_empty_batch_is_a_success_before_any_pointer_is_looked_at(lib, entry):
    assert _call(lib, entry, n=0) == 0
    assert _call(lib, entry, n=0, pointers=None) == 0
    assert _call(lib, entry, n=0, pointers=OFF4) == 0
    optional = {a: None for a in ("units_needed", "err_flag") if a in ENTRIES[entry][0]}
    assert _call(lib, entry, n=0, pointers=None, **optional) == 0
    # ... but not before the sizes
    for change in (dict(d=0), dict(d=65), dict(num_blocks=-1), dict(num_blocks=4)):
        assert _call(lib, entry, n=0, pointers=None, **change) == 1, change


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_null_and_misaligned_pointers(lib, entry):
    for p in _pointers(entry):
        assert _call(lib, entry, **{p: None}) == 1, p
    for p in ALIGNED + (["context_frag"] if entry in CONTEXT_ENTRIES else []):
        assert _call(lib, entry, **{p: OFF4}) == 1, p


@pytest.mark.parametrize("entry", RQ_ENTRIES)
def test_affine_and_rational_quadratic_forms(lib, entry):
    assert _call(lib, entry, params_per_dim=3) == 1                       # affine: scale and shift
    assert _call(lib, entry, params_per_dim=1) == 1
    assert _call(lib, entry, kind=2) == 1
    assert _call(lib, entry, kind=-1) == 1
    assert _call(lib, entry, kind=2, cfg=_rq(), params_per_dim=23) == 1
    assert _call(lib, entry, cfg=None, **RQ23) == 1                       # a spline without its configuration
    assert _call(lib, entry, cfg=_rq(8, 1), kind=1, params_per_dim=24) == 1      # 3K - 1 with tails, 3K + 1 without
    assert _call(lib, entry, cfg=_rq(8, 1), kind=1, params_per_dim=25) == 1
    assert _call(lib, entry, cfg=_rq(8, 0), kind=1, params_per_dim=23) == 1
    assert _call(lib, entry, cfg=_rq(8, 0), kind=1, params_per_dim=24) == 1
    assert _call(lib, entry, cfg=_rq(17, 1), kind=1, params_per_dim=50) == 1     # K <= 16, at most 48 parameters per dim
    assert _call(lib, entry, cfg=_rq(17, 1), kind=1, params_per_dim=48) == 1
    assert _call(lib, entry, cfg=_rq(16, 0), kind=1, params_per_dim=49) == 1
    assert _call(lib, entry, cfg=_rq(0, 0), kind=1, params_per_dim=1) == 1       # 3K + 1 holds, K >= 1 does not
    assert _call(lib, entry, cfg=_rq(0, 1), kind=1, params_per_dim=-1) == 1
    # the empty batch: kind, the affine form's two parameters, the limit of 48 and a missing configuration come before it,
    # what the configuration says after it
    assert _call(lib, entry, n=0, pointers=None, cfg=_rq(8, 1), **RQ23) == 0
    assert _call(lib, entry, n=0, pointers=None, cfg=_rq(8, 1), kind=1, params_per_dim=24) == 0
    assert _call(lib, entry, n=0, pointers=None, cfg=_rq(17, 1), kind=1, params_per_dim=48) == 0
    assert _call(lib, entry, n=0, pointers=None, params_per_dim=3) == 1
    assert _call(lib, entry, n=0, pointers=None, kind=2) == 1
    assert _call(lib, entry, n=0, pointers=None, cfg=None, **RQ23) == 1
    assert _call(lib, entry, n=0, pointers=None, cfg=_rq(17, 1), kind=1, params_per_dim=50) == 1
    assert _call(lib, entry, n=0, pointers=None, cfg=_rq(0, 0), kind=1, params_per_dim=0) == 1
    # every other refusal holds for the spline as for the affine form
    for change in (dict(d=65), dict(num_blocks=4), dict(n=17), dict(z=None), dict(final_unscale=None), dict(final_bias=OFF4)):
        assert _call(lib, entry, cfg=_rq(8, 1), **dict(RQ23, **change)) == 1, change


def test_sum_of_sigmoids_form(lib):
    entry = "fc_made_inverse_sos"
    for s in (0, 32, -1):
        assert _call(lib, entry, n_sigmoids=s) == 1, s
        assert _call(lib, entry, n=0, pointers=None, n_sigmoids=s) == 1, s
    assert _call(lib, entry, n=0, pointers=None, n_sigmoids=31) == 0              # 94 of at most 96 parameters per dim
    assert _call(lib, entry, n=0, pointers=None, n_sigmoids=31, d=64, num_blocks=3) == 0


def test_sibling_spline_forms(lib):
    entry = "fc_made_inverse_spline"
    assert _call(lib, entry, cfg=None) == 1
    assert _call(lib, entry, n=0, pointers=None, cfg=None) == 1
    for kind in (LINEAR, QUADRATIC, CUBIC):
        for bins in (0, 49, -1):
            assert _call(lib, entry, cfg=_spline(kind, bins)) == 1, (kind, bins)
            assert _call(lib, entry, n=0, pointers=None, cfg=_spline(kind, bins)) == 1, (kind, bins)
    for kind in (3, -1):
        assert _call(lib, entry, cfg=_spline(kind, 8)) == 1, kind
        assert _call(lib, entry, n=0, pointers=None, cfg=_spline(kind, 8)) == 1, kind
    # at most 48 parameters per dim: K (linear), 2K - 1 with tails / 2K + 1 without (quadratic), 2K + 2 (cubic)
    for kind, tails, last in ((LINEAR, 0, 48), (QUADRATIC, 1, 24), (QUADRATIC, 0, 23), (CUBIC, 0, 23)):
        assert _call(lib, entry, n=0, pointers=None, cfg=_spline(kind, last, tails)) == 0, (kind, tails)
        assert _call(lib, entry, n=0, pointers=None, cfg=_spline(kind, last + 1, tails)) == 1, (kind, tails)
        assert _call(lib, entry, cfg=_spline(kind, last + 1, tails)) == 1, (kind, tails)
    for change in (dict(d=65), dict(num_blocks=4), dict(n=17), dict(y=None), dict(hidden_frag=OFF4)):
        assert _call(lib, entry, cfg=_spline(QUADRATIC, 24, 1), **change) == 1, change


@pytest.mark.parametrize("entry", MOG_ENTRIES)
def test_mixture_components(lib, entry):
    for c in (0, 17, -1):
        assert _call(lib, entry, c=c) == 1, c
        assert _call(lib, entry, n=0, pointers=None, c=c) == 1, c
    assert _call(lib, entry, n=0, pointers=None, c=16) == 0
    assert _call(lib, entry, n=0, pointers=None, c=1, d=64, num_blocks=3) == 0


@pytest.mark.parametrize("entry", CONTEXT_ENTRIES)
def test_context_arguments(lib, entry):
    for c in (0, 33, -1):
        assert _call(lib, entry, context_features=c) == 1, c
        assert _call(lib, entry, n=0, pointers=None, context_features=c) == 1, c      # a size: before the empty batch
    assert _call(lib, entry, n=0, pointers=None, context_features=32) == 0
    for p in CONTEXT:
        assert _call(lib, entry, **{p: None}) == 1, p
        assert _call(lib, entry, n=0, **{p: None}) == 0, p
    assert _call(lib, entry, context_frag=OFF4) == 1
