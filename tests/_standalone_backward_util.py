"""Cases, launch-route predictors, float64 / float32 references and the per-slice comparison of the four stand-alone
backward entries (tests/test_standalone_backward_host.py, tests/test_gpu_standalone_backward.py):

    rq      fc_rq_spline_backward          csrc/fc_rq_backward.hip
    spline  fc_piecewise_spline_backward   csrc/fc_splines_backward.hip
    sos     fc_sum_of_sigmoids_backward    csrc/fc_sos_backward.hip
    affine  fc_affine_backward             csrc/fc_affine.hip

Importing it needs no GPU.

Cases.  ``SPECS`` names every case of the GPU file; ``case(id)`` builds its CPU tensors from a seed derived from the id.  A
case holds its DISTINCT rows only; a large case repeats them through ``idx = arange(n) % distinct`` (the trick of
tests/_tile_util.py): the GPU file gathers on the device, asserts that every row equals the first appearance of its source
row bit for bit and compares the distinct rows with float64.

Routes.  ``rq_route``, ``sos_route``, ``splines_trips`` and ``affine_trips`` restate the launchers' decisions in Python;
``branches`` names the branches a case reaches and the host file asserts that ``REQUIRED_BRANCHES`` are all reached.

References.  Autograd on oracle/torch_oracle.py in float64 and float32, loss L = sum gy y + sum gl logabsdet.

Exclusions, from float64 quantities only (``excluded``): transformed elements within 2^-18 (right - left) of an interior
knot of their own spline (d logabsdet / d params jumps there), and elements whose float64 output lies within that window of
a clamp edge whose slope enters the gradient (``clamp(., 0, 1)`` of the linear and quadratic splines where gy != 0,
``clamp(., 0, 3)`` of FC_AFFINE_SOFTPLUS_CLAMP3).  A case of n <= 1024 rows leaves out none and a larger one at most
``MAX_SHARE`` of its elements: the builder bumps the seed by 1000 until that holds (``Case.bump``), the host file asserts it.

The comparison.  The gradient is cut into slices: gx on the transformed columns per row, gp per row, gp per transformed dim.
Per slice

    scale = max |float64|,  floor = max |float32 reference - float64|,  err = max |kernel - float64|
    scale < 1e-30:  the kernel's slice is exactly zero
    otherwise:      err <= MARGIN * floor + (C[entry] + ULP) * scale + cond

so that an error in one row or one dim fails even where it is small next to the largest entry of the whole tensor.
MARGIN = 4 is the project's figure.  C covers the slices at which the float32 reference happens to be (nearly) exact; it is
measured from the float32 reference alone, never from a kernel: the median of floor / scale over all slices of the entry's
grid, rounded up to one significant digit (``PYTHONPATH=. python tests/_standalone_backward_util.py`` prints them):

    rq 2e-06 (median 1.06e-06)   spline 3e-07 (2.1e-07)   sos 2e-07 (1.52e-07)   affine 4e-08 (3.11e-08)

ULP = 2^-23 is no part of C: it is one float32 ulp of the slice's largest entry, the representability of the result.  The
measured C of the affine family, 4e-8, is below HALF an ulp (6e-8): where the float32 reference happens to be exact (d_t = 1:
floor / scale 1e-10 at some rows) a correctly rounded result that takes one more float32 operation misses C * scale.

cond (``conditioning``, ``moved``, ``rq_adjoint``) is the derived part of the bound, from float64 quantities only: the response
of the float64 gradient to a move of the inputs by two float32 ulps, the documented error of the kernels' primitives, and for
the RQ entry a running error bound of the kernel's own adjoint formulas (``Rounded``: cancellation on the way).  It is small
wherever the element is well conditioned: the median of cond / scale over an entry's grid is recorded in ``COND_MEDIAN`` the
way C is (printed by the same command, asserted by the host file):

    rq 3e-05 (median 2.62e-05)   spline 2e-06 (1.63e-06)   sos 4e-06 (3.24e-06)   affine 4e-07 (3.99e-07)

The identity columns of gx equal gy bit for bit."""
import collections
import functools
import math
import zlib

import torch
import torch.nn.functional as F

from flowconductor_amd import ops
from oracle import torch_oracle as O

MARGIN = 4.0
C = {"rq": 2e-06, "spline": 3e-07, "sos": 2e-07, "affine": 4e-08}
COND_MEDIAN = {"rq": 3e-05, "spline": 2e-06, "sos": 4e-06, "affine": 4e-07}      # of cond / scale, rounded up to one digit
ZERO_SCALE = 1e-30
ULP = 2.0 ** -23
KNOT_WINDOW = 2.0 ** -18
MAX_SHARE = 0.005            # tests/_tile_util.MAX_SHARE
SMALL_ROWS = 1024
CUS_MI355X = 256
DISTINCT = 256
RQ_BOUND, RQ_WH = 3.0, 8.0
SPLINE_BOUND = 2.0
ENTRIES = ("rq", "spline", "sos", "affine")

Spec = collections.namedtuple("Spec", "entry id cfg d d_t n distinct variant named")
Case = collections.namedtuple("Case", "spec entry id cfg n d d_t x params cols gy gl idx distinct bump")


def _r4(v):
    return (v + 3) & ~3


def _ceil(a, b):
    return -(-a // b)


# ---- route predictors ----------------------------------------------------------------------------------------------------

def rq_param_count(k, tails):
    return 3 * k - 1 if tails else 3 * k + 1


def rq_route(n, d, d_t, k, tails, aligned_rows=True, aligned_params=True):
    """``launch_bwd`` (csrc/fc_rq_backward.hip:167-201) and the dispatch on K (:216-221):
    (rows of the wave kernel, rows of the generic kernel, the wave kernel's strip "vector" | "scalar" | None, K compiled in)."""
    static = k in (4, 8, 16)                                                      # :216-221
    if static:                                                                    # :172
        p = rq_param_count(k, tails)
        pow2 = (d_t & (d_t - 1)) == 0 and d_t <= 64                               # :173
        g = 64 // d_t if pow2 else 1                                              # :174
        groups = n // g if pow2 else 0                                            # :175
        rows_ok = (g * d) % 4 != 0 or aligned_rows                                # :176-177
        lds = 4 * (_r4(d_t) + 4 * (2 * _r4(g * d) + _r4(64 * p)))                 # :178
        if groups >= 64 and rows_ok and lds <= 64 * 1024 and aligned_params:      # :179
            done = groups * g                                                     # :185
            return done, n - done, "vector" if (g * d) % 4 == 0 else "scalar", True     # :132, :186-190
    return 0, n, None, static


def rq_trips(wave_rows, generic_rows, d_t):
    """Grid-stride trips of (wave kernel, generic kernel): 2048 workgroups of four waves, one group of 64 / d_t rows per wave
    (:180-182, :117-118); 8192 workgroups of 256 threads, one element per thread (:196-199, :72)."""
    wave = 0
    if wave_rows:
        groups = wave_rows // (64 // d_t)
        wave = _ceil(groups, min(256 * 8, _ceil(groups, 4)) * 4)
    generic = 0
    if generic_rows:
        total = generic_rows * d_t
        generic = _ceil(total, min(256 * 32, _ceil(total, 256)) * 256)
    return wave, generic


def sos_route(total, s, cus):
    """``fc_sum_of_sigmoids_backward`` (csrc/fc_sos_backward.hip:182-211): ("tile" | "direct", groups of work, grid)."""
    ts = 3 * s + 1 + s                                                            # :192
    ts += (ts & 1) == 0                                                           # :193
    per_cu = (160 * 1024) // (64 * ts * 4)                                        # :194-195
    if per_cu >= 1:                                                               # :196
        groups = _ceil(total, 64)                                                 # :200
        return "tile", groups, min(groups, cus * per_cu)                          # :201-202
    groups = _ceil(total, 256)                                                    # :206
    return "direct", groups, min(groups, cus * 16)                                # :207-208


def splines_trips(total_threads, cus):
    """``fc_piecewise_spline_backward`` (csrc/fc_splines_backward.hip:106-108, :50): trips of the grid-stride loop."""
    grid = min(_ceil(total_threads, 256), cus * 8)
    return _ceil(total_threads, grid * 256)


def affine_trips(total):
    """``fc_affine_backward`` (csrc/fc_affine.hip:175-177, :108): trips of the grid-stride loop."""
    grid = min(_ceil(total, 256), 256 * 32)
    return _ceil(total, grid * 256)


# ---- the grid --------------------------------------------------------------------------------------------------------------

KIND_CODE = {"linear": ops.SPLINE_LINEAR, "quadratic": ops.SPLINE_QUADRATIC, "cubic": ops.SPLINE_CUBIC}
SPLINE_MID = {("linear", False): 7, ("linear", True): 7, ("quadratic", False): 6, ("quadratic", True): 9,
              ("cubic", False): 8, ("cubic", True): 5}
AFFINE_ACTS = {"sigmoid_plus2": ops.AFFINE_SIGMOID_PLUS2, "softplus_clamp3": ops.AFFINE_SOFTPLUS_CLAMP3,
               "scale_given": ops.AFFINE_SCALE_GIVEN, "additive": ops.AFFINE_ADDITIVE, "maf_softplus": ops.AFFINE_MAF_SOFTPLUS,
               "shift_tanh2": ops.AFFINE_SHIFT_TANH2, "scale_softplus": ops.AFFINE_SCALE_SOFTPLUS}
AFFINE_ONE = ("additive", "shift_tanh2", "scale_softplus")       # one raw value per transformed dim

# rows of the edge cases (n = 64)
ROW_HI, ROW_LO, ROW_ABOVE, ROW_BELOW, ROW_BIG_DERIVATIVE, ROW_WIDE_BIN, ROW_EQUAL = 0, 1, 2, 3, 4, 5, 6
SOS_ROWS = {"a+": 0, "a-": 1, "b+": 2, "b-": 3, "c+": 4, "e+": 5, "e-": 6, "x+": 7, "x-": 8}
AFFINE_ROW_ABOVE20, AFFINE_ROW_CLAMPED, AFFINE_ROW_MINUS40 = 0, 1, 2


def largest_k(kind, tails):
    """The largest bin count ``ops.piecewise_spline_backward_supported`` admits."""
    k = 1
    while ops.piecewise_spline_backward_supported(KIND_CODE[kind], k + 1, "linear" if tails else None):
        k += 1
    return k


def _tn(tails):
    return "tails" if tails else "box"


def grid(cus=CUS_MI355X):
    """Every case of the GPU file, {id: Spec}.  Only the row count of the three second trips that are capped by the number
    of compute units depends on ``cus``."""
    out = collections.OrderedDict()

    def add(entry, name, cfg, d, d_t, n, distinct=None, variant="plain", named=()):
        """``named``: the branches the case is in the grid for; the GPU file asserts them with the predictors, on the very
        pointers of its launch, before it launches."""
        cid = "%s-%s" % (entry, name)
        assert cid not in out, cid
        out[cid] = Spec(entry, cid, cfg, d, d_t, n, n if distinct is None else distinct, variant, tuple(named))

    # rq: every instantiation, on the wave kernel (512 rows: 64 groups of 8) and below its threshold (511)
    for k in (4, 8, 16, 5, 10, 32):
        for tails in (True, False):
            cfg, tag = dict(k=k, tails=tails), "K%d-%s-d12-dt8-n" % (k, _tn(tails))
            static = k in (4, 8, 16)
            add("rq", tag + "512", cfg, 12, 8, 512, named=["wave-K%d" % k if static else "runtime-K%d" % k])
            add("rq", tag + "511", cfg, 12, 8, 511, named=["below-64-groups" if static else "runtime-K%d" % k])
    # rq: routes
    for k, tails in ((8, True), (4, False)):
        cfg, tag = dict(k=k, tails=tails), "K%d-%s" % (k, _tn(tails))
        add("rq", tag + "-leftover", cfg, 12, 8, 517, named=["wave+leftover"])
        add("rq", tag + "-scalar-g2", cfg, 33, 32, 131, named=["strip-scalar", "G=2", "wave+leftover"])
        add("rq", tag + "-scalar-g1", cfg, 65, 64, 70, named=["strip-scalar", "G=1"])
        add("rq", tag + "-g64", cfg, 3, 1, 4103, named=["G=64", "wave+leftover", "strip-vector"])
        add("rq", tag + "-g1-nocols", cfg, 64, 64, 70, named=["G=1", "cols-none", "strip-vector"])
        add("rq", tag + "-misaligned-rows", cfg, 12, 8, 512, variant="mis_x", named=["misaligned-rows-fallback"])
        add("rq", tag + "-misaligned-params", cfg, 12, 8, 512, variant="mis_p", named=["misaligned-params-fallback"])
        add("rq", tag + "-gl-none", cfg, 12, 8, 517, variant="gl_none", named=["wave+leftover"])
        add("rq", tag + "-gy-zero", cfg, 12, 8, 517, variant="gy_zero", named=["wave+leftover"])
    add("rq", "K16-box-lds-fallback", dict(k=16, tails=False), 64, 1, 4096, named=["lds-fallback"])
    add("rq", "K4-tails-wave-trip2", dict(k=4, tails=True), 64, 64, 8192 + 130, DISTINCT, named=["wave-trip2"])
    add("rq", "K5-tails-generic-trip2", dict(k=5, tails=True), 48, 48, 43800, DISTINCT, named=["generic-trip2"])
    add("rq", "K8-tails-autograd", dict(k=8, tails=True), 12, 8, 512, variant="autograd", named=["wave-K8"])
    for k, tails in ((8, True), (9, False)):
        for ident in (False, True):
            add("rq", "K%d-%s-edges%s" % (k, _tn(tails), "-identity-init" if ident else ""),
                dict(k=k, tails=tails, ident=ident), 12, 8, 64, variant="edges")

    # piecewise splines: every K at (5, 3, 400); the other two shapes and the edge rows at the middle K
    for (kind, tails), mid in SPLINE_MID.items():
        for k in (3, mid, largest_k(kind, tails)):
            p = ops.spline_multiplier(KIND_CODE[kind], k, "linear" if tails else None)
            add("spline", "%s-K%d-%s-d5-dt3-n400" % (kind, k, _tn(tails)), dict(kind=kind, k=k, tails=tails), 5, 3, 400,
                named=["lds-64KB"] if p == 32 else [])
        cfg, tag = dict(kind=kind, k=mid, tails=tails), "%s-K%d-%s" % (kind, mid, _tn(tails))
        add("spline", tag + "-d4-dt4-n257", cfg, 4, 4, 257, named=["cols-none"])
        add("spline", tag + "-d3-dt1-n130", cfg, 3, 1, 130, named=["d_t=1"])
        add("spline", tag + "-edges", cfg, 5, 3, 64, variant="edges")
    add("spline", "linear-K8-box-trip2", dict(kind="linear", k=8, tails=False), 16, 16, (cus * 8 * 256) // (16 * 9) + 2, DISTINCT,
        named=["trip2"])

    # sum of sigmoids (every column is transformed)
    for s in (1, 6, 30):
        add("sos", "S%d-n515-d5" % s, dict(s=s), 5, 5, 515, named=["tile", "tile-partial-group"])
        add("sos", "S%d-n64-d4" % s, dict(s=s), 4, 4, 64, named=["tile", "tile-whole-groups"])        # 256 elements
    add("sos", "S159-n70-d3", dict(s=159), 3, 3, 70, named=["tile", "tile-lds-160KB"])
    for s in (160, 200):
        add("sos", "S%d-n70-d3" % s, dict(s=s), 3, 3, 70, named=["direct"])
    add("sos", "S30-tile-trip2", dict(s=30), 8, 8, (cus * 5 * 64) // 8 + 1, DISTINCT, named=["tile", "tile-trip2"])
    for s, kernel in ((6, "tile"), (160, "direct")):
        add("sos", "S%d-gl-none" % s, dict(s=s), 5, 5, 130, variant="gl_none", named=[kernel])
        add("sos", "S%d-postact" % s, dict(s=s, log_post=0.7), 5, 5, 130, variant="postact", named=[kernel])
        add("sos", "S%d-saturated" % s, dict(s=s), 3, 3, 64, variant="edges", named=[kernel])

    # affine family
    for act in AFFINE_ACTS:
        add("affine", act + "-d10-dt6-n300", dict(act=act), 10, 6, 300, named=[act + "-cols-subset"])
        add("affine", act + "-d6-dt6-n300", dict(act=act), 6, 6, 300, named=[act + "-cols-none"])
        add("affine", act + "-d4-dt1-n300", dict(act=act), 4, 1, 300, named=[act + "-d_t=1"])
        add("affine", act + "-edges", dict(act=act), 10, 6, 64, variant="edges", named=[act + "-edges"])
    for act in ("softplus_clamp3", "maf_softplus"):
        add("affine", act + "-trip2", dict(act=act), 8, 8, 262200, DISTINCT, named=["trip2"])
    return out


SPECS = grid()


def ids(entry, variant=None, contains=None):
    return [i for i, s in SPECS.items() if s.entry == entry and (variant is None or s.variant == variant)
            and (contains is None or contains in i)]


def params_per_dim(spec):
    cfg = spec.cfg
    if spec.entry == "rq":
        return rq_param_count(cfg["k"], cfg["tails"])
    if spec.entry == "spline":
        return ops.spline_multiplier(KIND_CODE[cfg["kind"]], cfg["k"], "linear" if cfg["tails"] else None)
    if spec.entry == "sos":
        return 3 * cfg["s"] + 1
    return 1 if cfg["act"] in AFFINE_ONE else 2


def interval(spec):
    """(left, right) of a spline's interval, the same on both axes."""
    if not spec.cfg["tails"]:
        return 0.0, 1.0
    b = RQ_BOUND if spec.entry == "rq" else SPLINE_BOUND
    return -b, b


def rq_kwargs(spec):
    """Keyword arguments of ``ops.rq_spline_backward`` / ``ops.rq_spline_autograd``."""
    cfg = spec.cfg
    if cfg["tails"]:
        return dict(num_bins=cfg["k"], tails="linear", tail_bound=RQ_BOUND, wh_divisor=RQ_WH,
                    enable_identity_init=cfg.get("ident", False))
    return dict(num_bins=cfg["k"], tails=None, enable_identity_init=cfg.get("ident", False))


def spline_kwargs(spec):
    cfg = spec.cfg
    return dict(kind=KIND_CODE[cfg["kind"]], num_bins=cfg["k"], tails="linear" if cfg["tails"] else None,
                tail_bound=SPLINE_BOUND)


# ---- case builders ---------------------------------------------------------------------------------------------------------

def _draw(spec, seed):
    """(x [R, d], params [R, d_t P], cols or None, gy [R, d], gl [R] or None) of the distinct rows."""
    gen = torch.Generator().manual_seed(seed)
    r, d, d_t, cfg, p = spec.distinct, spec.d, spec.d_t, spec.cfg, params_per_dim(spec)
    cols = None if d_t == d else torch.randperm(d, generator=gen)[:d_t].to(torch.int32)       # unsorted subset
    tc = slice(None) if cols is None else cols.long()
    gy, gl = torch.randn(r, d, generator=gen), torch.randn(r, generator=gen)
    params = torch.randn(r, d_t * p, generator=gen)
    edges = spec.variant == "edges"
    if spec.entry in ("rq", "spline"):
        lo, hi = interval(spec)
        spread = 1.8 if spec.entry == "rq" else 1.2
        x = torch.randn(r, d, generator=gen) * spread if cfg["tails"] else torch.rand(r, d, generator=gen) * 0.96 + 0.02
        if edges:
            rows = params.view(r, d_t, p)
            x[ROW_HI, tc], x[ROW_LO, tc] = hi, lo
            if cfg["tails"]:
                x[ROW_ABOVE], x[ROW_BELOW] = hi + 1.0, lo - 0.5
            if spec.entry == "rq":
                k = cfg["k"]
                gl[[ROW_HI, ROW_LO]] = 0.0      # y is the pinned end whatever the parameters are: gp = 0, gx = gy d_end
                rows[ROW_BIG_DERIVATIVE, :, 2 * k:] = 35.0       # every knot: above 20 / beta for both values of beta
                rows[ROW_WIDE_BIN, :, 2] = 60.0 * (RQ_WH if cfg["tails"] else 1.0)     # the softmax sees +60
                rows[ROW_EQUAL] = 0.3
            elif cfg["kind"] != "cubic":
                # the clamped splines: whether out = 1 - ulp or 1 + ulp at the right end decides the clamp's slope, in any
                # precision; with gy = 0 only logabsdet, which is not clamped, carries a gradient
                gy[[ROW_HI, ROW_LO]] = 0.0
    elif spec.entry == "sos":
        s = cfg["s"]
        x = torch.randn(r, d, generator=gen) * 3
        if edges:
            rows = params.view(r, d_t, p)
            rows[SOS_ROWS["a+"], :, 0], rows[SOS_ROWS["a-"], :, 0] = 8.0, -8.0
            rows[SOS_ROWS["b+"], :, s], rows[SOS_ROWS["b-"], :, s] = 12.0, -12.0
            rows[SOS_ROWS["c+"], :, 2 * s + min(1, s - 1)] = 40.0
            rows[SOS_ROWS["e+"], :, 3 * s], rows[SOS_ROWS["e-"], :, 3 * s] = 15.0, -15.0
            x[SOS_ROWS["x+"]], x[SOS_ROWS["x-"]] = 30.0, -30.0
    else:
        x = torch.randn(r, d, generator=gen)
        params = params * 1.5
        act = cfg["act"]
        if edges:
            if act == "maf_softplus":
                scale = params.view(r, d_t, 2)[..., 0]
            else:
                scale = params[:, d_t:] if p == 2 else params
            scale[AFFINE_ROW_ABOVE20], scale[AFFINE_ROW_CLAMPED], scale[AFFINE_ROW_MINUS40] = 25.0, 3.5, -40.0
        if act == "scale_given":
            params[:, d_t:] = params[:, d_t:].abs() + 0.2
    if spec.variant == "gl_none":
        gl = None
    elif spec.variant == "gy_zero":
        gy.zero_()
    return x, params, cols, gy, gl


def seed_of(spec, bump=0):
    return zlib.crc32(spec.id.encode()) % (2 ** 31 - 1) + 1000 * bump


def allowed_excluded(spec):
    """How many transformed elements a case may leave out."""
    return 0 if spec.n <= SMALL_ROWS else int(MAX_SHARE * spec.distinct * spec.d_t)


def build(spec, max_bumps=50):
    for bump in range(max_bumps):
        x, params, cols, gy, gl = _draw(spec, seed_of(spec, bump))
        idx = None if spec.distinct == spec.n else torch.arange(spec.n) % spec.distinct
        cs = Case(spec, spec.entry, spec.id, spec.cfg, spec.n, spec.d, spec.d_t, x, params, cols, gy, gl, idx, spec.distinct,
                  bump)
        if int(excluded(cs).sum()) <= allowed_excluded(spec):
            return cs
    raise RuntimeError("no seed of %s keeps away from the knots" % spec.id)


@functools.lru_cache(maxsize=None)
def case(cid):
    """The case ``cid`` of ``SPECS`` (built once; nobody writes to its tensors)."""
    return build(SPECS[cid])


def tcols(cs):
    return torch.arange(cs.d) if cs.cols is None else cs.cols.long()


def identity_columns(cs):
    taken = set(tcols(cs).tolist())
    return [c for c in range(cs.d) if c not in taken]


def take_rows(cs, rows):
    """The sub-batch of ``rows`` of the distinct rows."""
    x = cs.x[rows]
    return cs._replace(n=x.shape[0], distinct=x.shape[0], x=x, params=cs.params[rows], gy=cs.gy[rows],
                       gl=None if cs.gl is None else cs.gl[rows], idx=None)


# ---- references ------------------------------------------------------------------------------------------------------------

def _spline_parts(kind, k, rows):
    if kind == "linear":
        return [rows]
    if kind == "quadratic":
        return [rows[..., :k], rows[..., k:]]
    return [rows[..., :k], rows[..., k:2 * k], rows[..., 2 * k:2 * k + 1], rows[..., 2 * k + 1:]]


_SPLINE_FN = {"linear": O.linear_spline, "quadratic": O.quadratic_spline, "cubic": O.cubic_spline}


def affine_scale_shift(act, p, d_t):
    """(shift, scale) [R, d_t] of raw rows ``p`` -- the formulas of test_affine_backward_matches_torch_autograd."""
    if act == "sigmoid_plus2":
        return p[:, :d_t], torch.sigmoid(p[:, d_t:] + 2) + 1e-3
    if act == "softplus_clamp3":
        return p[:, :d_t], torch.clamp(F.softplus(p[:, d_t:]) + 1e-3, 0, 3)
    if act == "scale_given":
        return p[:, :d_t], p[:, d_t:]
    if act == "maf_softplus":
        v = p.view(p.shape[0], d_t, 2)
        return v[..., 1], F.softplus(v[..., 0]) + 1e-3
    if act == "scale_softplus":
        return torch.zeros_like(p), F.softplus(p) + 1e-5
    if act == "shift_tanh2":
        return 2 * torch.tanh(p), torch.ones_like(p)
    return p, torch.ones_like(p)


def forward(cs, xt, params):
    """(outputs on the transformed columns [R, d_t], logabsdet [R]) of the oracle in the dtype of its arguments."""
    r, d_t, cfg = xt.shape[0], cs.d_t, cs.cfg
    if cs.entry == "affine":
        shift, s = affine_scale_shift(cfg["act"], params, d_t)
        return xt * s + shift, torch.log(s).sum(dim=1)
    rows = params.view(r, d_t, -1) * 1.0            # (rq_from_rows divides slices of its argument in place)
    if cs.entry == "rq":
        y, lad = O.rq_from_rows(xt, rows, cfg["k"], "linear" if cfg["tails"] else None, RQ_BOUND, False,
                                wh_divisor=RQ_WH if cfg["tails"] else None, enable_identity_init=cfg.get("ident", False))
        return y, lad.sum(dim=1)
    if cs.entry == "sos":
        s = cfg["s"]
        return O.sos_forward(xt, rows[..., :s], rows[..., s:2 * s], rows[..., 2 * s:3 * s], rows[..., 3 * s],
                             log_scale_postact=cfg.get("log_post", 0.0))
    fn, parts = _SPLINE_FN[cfg["kind"]], _spline_parts(cfg["kind"], cfg["k"], rows)
    if cfg["tails"]:
        y, lad = O._unconstrained(fn, xt, SPLINE_BOUND, "linear", parts)
    else:
        y, lad = fn(xt, *parts)
    return y, lad.sum(dim=1)


def loss(cs, xt, params):
    y, lad = forward(cs, xt, params)
    total = (y * cs.gy[:, tcols(cs)].to(xt.dtype)).sum()
    if cs.gl is not None:
        total = total + (lad * cs.gl.to(xt.dtype)).sum()
    return total


def gradients(cs, dtype):
    """(gx on the transformed columns [R, d_t], gp [R, d_t P]) by torch autograd on the CPU in ``dtype``."""
    xt = cs.x[:, tcols(cs)].to(dtype).requires_grad_(True)
    p = cs.params.to(dtype).clone().requires_grad_(True)
    total = loss(cs, xt, p)
    if not total.requires_grad:                   # (a batch wholly outside the tails with no upstream gradient)
        return torch.zeros_like(xt), torch.zeros_like(p)
    got = torch.autograd.grad(total, (xt, p), allow_unused=True)
    return tuple(torch.zeros_like(t) if g is None else g for t, g in zip((xt, p), got))


@functools.lru_cache(maxsize=None)
def reference(cid):
    """((gx, gp) float64, (gx, gp) float32) of case ``cid``: computed once, shared, never written to."""
    cs = case(cid)
    return gradients(cs, torch.float64), gradients(cs, torch.float32)


# ---- exclusions ------------------------------------------------------------------------------------------------------------

def inner_knots(cs):
    """float64 interior knots on the x axis [R, d_t, K - 1] of a spline case."""
    cfg, k = cs.cfg, cs.cfg["k"]
    lo, hi = interval(cs.spec)
    r = cs.x.shape[0]
    rows = cs.params.double().view(r, cs.d_t, -1)
    if cs.entry == "rq":
        knots, _ = O._knots(rows[..., :k] / (RQ_WH if cfg["tails"] else 1.0), lo, hi, 1e-3, k)
        return knots[..., 1:-1]
    if cfg["kind"] == "linear":
        return (lo + (hi - lo) * torch.arange(1, k, dtype=torch.float64) / k).expand(r, cs.d_t, k - 1)
    widths = 1e-3 + (1 - 1e-3 * k) * torch.softmax(rows[..., :k], dim=-1)
    return lo + (hi - lo) * torch.cumsum(widths, dim=-1)[..., :-1]


def excluded(cs):
    """bool [R, d_t]: the transformed elements the comparison leaves out (module docstring)."""
    r = cs.x.shape[0]
    out = torch.zeros(r, cs.d_t, dtype=torch.bool)
    xt = cs.x[:, tcols(cs)].double()
    if cs.entry in ("rq", "spline"):
        lo, hi = interval(cs.spec)
        out |= ((xt.unsqueeze(-1) - inner_knots(cs)).abs() <= KNOT_WINDOW * (hi - lo)).any(dim=-1)
        if cs.entry == "spline" and cs.cfg["kind"] != "cubic":
            with torch.no_grad():
                y, _ = forward(cs, xt, cs.params.double())
            inside = (xt >= lo) & (xt <= hi)
            at_edge = ((y - lo).abs() <= KNOT_WINDOW * (hi - lo)) | ((y - hi).abs() <= KNOT_WINDOW * (hi - lo))
            out |= inside & at_edge & (cs.gy[:, tcols(cs)] != 0)
    elif cs.entry == "affine" and cs.cfg["act"] == "softplus_clamp3":
        v = F.softplus(cs.params.double()[:, cs.d_t:]) + 1e-3
        out |= ((v - 3.0).abs() <= KNOT_WINDOW * 3.0) | (v.abs() <= KNOT_WINDOW * 3.0)
    return out


# ---- slices and the comparison ---------------------------------------------------------------------------------------------

def param_view(cs, gp):
    """``gp`` [R, d_t P] as [R, d_t, P] whatever the row layout (the affine rows [shift block | scale block] included)."""
    r = gp.shape[0]
    gp = gp.reshape(r, -1)
    if cs.entry == "affine" and cs.cfg["act"] in ("sigmoid_plus2", "softplus_clamp3", "scale_given"):
        return gp.view(r, 2, cs.d_t).permute(0, 2, 1)
    return gp.view(r, cs.d_t, -1)


SLICE_KINDS = ("gx_row", "gp_row", "gp_dim")


def slices(kind, cs, gx_t, gp, keep):
    """[slices, entries] float64 with the entries of the left-out elements (``keep`` [R, d_t] False) set to zero."""
    keep = keep.double()
    if kind == "gx_row":
        return gx_t.detach().double().cpu() * keep
    v = param_view(cs, gp.detach().double().cpu()) * keep.unsqueeze(-1)
    if kind == "gp_row":
        return v.reshape(v.shape[0], -1)
    return v.permute(1, 0, 2).reshape(cs.d_t, -1)


Result = collections.namedtuple("Result", "ok worst worst_floor detail")


def compare(got, ref64, ref32, c, cond, margin=MARGIN):
    """Per-slice comparison of [slices, entries] tensors: ``ok``, the worst err / bound, the worst err / floor (over the
    slices with a floor above 1e-3 c scale) and a line that names the worst slice."""
    scale = ref64.abs().amax(dim=1)
    floor = (ref32 - ref64).abs().amax(dim=1)
    err = (got - ref64).abs().amax(dim=1)
    finite = bool(torch.isfinite(got).all())
    bound = margin * floor + (c + ULP) * scale + cond
    zero = scale < ZERO_SCALE
    bad = torch.where(zero, got.abs().amax(dim=1) != 0, ~(err <= bound))
    ratio = torch.where(zero, torch.zeros_like(err), err / bound.clamp_min(1e-300))
    rfloor = torch.where(zero | (floor <= 1e-3 * c * scale), torch.zeros_like(err), err / floor.clamp_min(1e-300))
    i = int(ratio.nan_to_num(nan=float("inf")).argmax()) if not bool(bad.any()) else int(bad.float().argmax())
    detail = "slice %d: err %.3g, floor %.3g, scale %.3g, cond %.3g, bound %.3g; %d of %d slices fail" % (
        i, err[i], floor[i], scale[i], cond[i], bound[i], int(bad.sum()), bad.numel())
    return Result(finite and not bool(bad.any()), float(ratio.max()), float(rfloor.max()), detail)


MOVES = ("params", "x", "upstream")


def moved(cs, gen, what):
    """``cs`` with one group of its float64 inputs moved by what float32 arithmetic on the kernels' primitives does to it:

        params    every raw parameter by +-2^-22 max(1, |u|).  Every raw value first meets an exponential, a sigmoid, a tanh
                  or a softplus; csrc/fc_math.h documents exp_lean, log_lean and div_lean at <= 1 ulp each and sigmoid_lean /
                  tanh_lean at 1 - 2 ulp, and a result that is 2 ulp off, f(u) (1 +- 2^-22), is the exact function of an
                  argument moved by that much: exp(u) (1 +- e) = exp(u +- e); the |u| part is the rounding of the argument
                  itself (u / wh_divisor, beta u, u + 2).
        x         splines: every transformed entry inside the interval by +-sqrt(K) 2^-24 (right - left), clamped to the
                  interval (x - knot in float32: a knot is a cumulative sum of up to K widths with one rounding of the
                  interval's size each, adding up like a random walk -- the figure of tests/_fused_backward_util.py);
                  the other entries: by +-2^-22 |x| (alpha (x - s), x s: products with 2-ulp quantities).
        upstream  gy and gl by +-2^-22 |entry|: each multiplies a derivative that comes out of those primitives 2 ulp off,
                  d (1 +- 2^-22) gy = d gy (1 +- 2^-22), and the two products may be far larger than their sum.

    Random signs from ``gen``."""
    def sign(t):
        return torch.randint(0, 2, t.shape, generator=gen).double() * 2 - 1

    if what == "params":
        params = cs.params.double()
        return cs._replace(params=params + sign(params) * 2.0 ** -22 * params.abs().clamp_min(1.0))
    if what == "x":
        x = cs.x.double()
        if cs.entry in ("rq", "spline"):
            lo, hi = interval(cs.spec)
            step = cs.cfg["k"] ** 0.5 * 2.0 ** -24 * (hi - lo)
            return cs._replace(x=torch.where((x >= lo) & (x <= hi), (x + sign(x) * step).clamp(lo, hi), x))
        return cs._replace(x=x * (1 + sign(x) * 2.0 ** -22))
    gy = cs.gy.double() * (1 + sign(cs.gy) * 2.0 ** -22)
    return cs._replace(gy=gy, gl=None if cs.gl is None else cs.gl.double() * (1 + sign(cs.gl) * 2.0 ** -22))


@functools.lru_cache(maxsize=None)
def conditioning(cid, trials=3):
    """{kind: [slices]}: how far the FLOAT64 gradient of case ``cid`` moves, per slice, when its inputs move as ``moved``
    describes: per group of inputs the largest change over ``trials`` draws of the signs, summed over the three groups
    (two groups' responses may cancel under one draw of the signs and add up under the next); for the RQ entry plus
    ``rq_adjoint``'s running error bound.

    This is the derived part of the bound.  MARGIN * floor + (C + ULP) * scale alone fails on the GPU at single rows (err /
    floor 5 .. 1000): a per-row slice of one to eight elements is too small a sample for ONE float32 run to measure float32
    arithmetic.  At an element in a narrow bin or on a steep sigmoid (|alpha (x - s)| up to 100) the gradient amplifies the
    2-ulp error of the kernels' lean primitives by the very factor by which it amplifies a move of the inputs, and
    gx = gy dy/dx + gl dlogabsdet/dx may be a hundredth of either product.  cond states those factors in float64 quantities
    alone; nothing in it comes from a kernel or from the float32 reference."""
    cs = case(cid)
    r64, _ = reference(cid)
    keep = ~excluded(cs)
    gen = torch.Generator().manual_seed(seed_of(cs.spec) + 7)
    base = {kind: slices(kind, cs, r64[0], r64[1], keep) for kind in SLICE_KINDS}
    total = {kind: torch.zeros(base[kind].shape[0], dtype=torch.float64) for kind in SLICE_KINDS}
    for what in MOVES:
        worst = {kind: torch.zeros_like(total[kind]) for kind in SLICE_KINDS}
        for _ in range(trials):
            m64 = gradients(moved(cs, gen, what), torch.float64)
            for kind in SLICE_KINDS:
                worst[kind] = torch.maximum(worst[kind], (slices(kind, cs, m64[0], m64[1], keep) - base[kind]).abs().amax(dim=1))
        for kind in SLICE_KINDS:
            total[kind] = total[kind] + worst[kind]
    if cs.entry == "rq":
        _, _, e_gx, e_gp = rq_adjoint(cs)
        for kind in SLICE_KINDS:
            total[kind] = total[kind] + slices(kind, cs, e_gx, e_gp, keep).amax(dim=1)
    return total


class Rounded:
    """A float64 value ``v`` with a first-order bound ``e`` on the error of its float32 evaluation (running error analysis):
    every sum, difference and product adds half an ulp of its result, 2^-24 |v|, every quotient one ulp (div_lean,
    csrc/fc_math.h), on top of the operands' errors carried through the operation.  A plain tensor or number is exact."""
    HALF_ULP = 2.0 ** -24

    def __init__(self, v, e=None):
        self.v, self.e = v, torch.zeros_like(v) if e is None else e

    @staticmethod
    def of(t):
        return t if isinstance(t, Rounded) else Rounded(torch.as_tensor(t, dtype=torch.float64))

    def _out(self, v, e, ulps=1.0):
        return Rounded(v, e + ulps * Rounded.HALF_ULP * v.abs())

    def __add__(self, o):
        o = Rounded.of(o)
        return self._out(self.v + o.v, self.e + o.e)

    def __sub__(self, o):
        o = Rounded.of(o)
        return self._out(self.v - o.v, self.e + o.e)

    def __rsub__(self, o):
        return Rounded.of(o) - self

    def __mul__(self, o):
        o = Rounded.of(o)
        return self._out(self.v * o.v, self.e * o.v.abs() + o.e * self.v.abs())

    __radd__, __rmul__ = __add__, __mul__

    def __truediv__(self, o):
        o = Rounded.of(o)
        q = self.v / o.v
        return self._out(q, (self.e + q.abs() * o.e) / o.v.abs(), 2.0)

    def __rtruediv__(self, o):
        return Rounded.of(o) / self

    def __neg__(self):
        return Rounded(-self.v, self.e)

    def unsqueeze(self, dim):
        return Rounded(self.v.unsqueeze(dim), self.e.unsqueeze(dim))


def rq_adjoint(cs):
    """``rq_backward_element`` (csrc/fc_rq_backward_op.h:104-163) restated in float64 on ``Rounded`` numbers: (gx [R, d_t],
    gp [R, d_t P]) and a first-order bound on what float32 arithmetic loses in these very formulas, (E_gx, E_gp).

    The element's inputs here -- x, gy, gl, the knots, the knot derivatives, the softmax probabilities -- are taken as exact:
    what their own float32 evaluation loses is what ``moved`` covers.  What no move of the inputs shows is cancellation on
    the way: sd = d_k + d_k+1 - 2 delta, g_t1 = 2 delta g_b1 + sd g_den + d_k g_a1, g_theta = 2 theta g_th2 +
    (1 - theta) g_t1 - g_omt, g_delta, and the chain to the knots all add terms of both signs.  At element 440 of
    ``rq-K8-tails-g64``, in a wide bin and far from a knot, g_t1 keeps 15 ulps and gx 70 in float32 arithmetic of these
    formulas on the CPU (the float32 reference, another operation order, is 20 floors off after a one-ulp change of a
    knot).  The host file asserts that (gx, gp) here equal the autograd reference."""
    cfg, k = cs.cfg, cs.cfg["k"]
    tails = cfg["tails"]
    lo, hi = interval(cs.spec)
    r, d_t = cs.x.shape[0], cs.d_t
    tc = tcols(cs)
    x, gy = cs.x[:, tc].double(), cs.gy[:, tc].double()
    gl = (torch.zeros(r) if cs.gl is None else cs.gl).double().unsqueeze(1).expand(r, d_t)
    u = cs.params.double().view(r, d_t, -1)
    p_count = u.shape[-1]
    inv = 1.0 / (RQ_WH if tails else 1.0)
    beta = math.log(2.0) / (1 - 1e-3) if cfg.get("ident") else 1.0
    cw = 1 - 1e-3 * k
    pw, ph = torch.softmax(u[..., :k] * inv, -1), torch.softmax(u[..., k:2 * k] * inv, -1)

    def knots(p):
        kn = F.pad(torch.cumsum(1e-3 + cw * p, -1), (1, 0)) * (hi - lo) + lo
        kn[..., 0], kn[..., -1] = lo, hi
        return kn, F.pad(torch.cumsum(p, -1), (1, 0))

    kx, cpw = knots(pw)
    ky, cph = knots(ph)
    inside = (x >= lo) & (x <= hi)
    idx = ((x.unsqueeze(-1) >= kx[..., :-1]).sum(-1) - 1).clamp(0, k - 1).unsqueeze(-1)

    def at(t, off=0):
        return t.gather(-1, idx + off)[..., 0]

    ud = u[..., 2 * k:]
    if tails:
        ud = F.pad(ud, (1, 1), value=math.log(math.exp(1 - 1e-3) - 1))
    dv = 1e-3 + F.softplus(ud, beta=beta)
    sl = torch.where(ud * beta > 20, torch.ones_like(ud), torch.sigmoid(ud * beta))
    xk, xk1, yk, yk1 = at(kx), at(kx, 1), at(ky), at(ky, 1)
    pwk, pwk1, phk, phk1 = at(cpw), at(cpw, 1), at(cph), at(cph, 1)
    d0, d1, s0, s1 = at(dv), at(dv, 1), at(sl), at(sl, 1)
    R = Rounded
    wk, hk = R(xk1) - xk, R(yk1) - yk
    rwk = 1.0 / wk
    delta, theta = hk * rwk, (R(x) - xk) * rwk
    omt = 1.0 - theta
    t1, th2 = theta * omt, theta * theta
    a1 = delta * th2 + t1 * d0
    num = hk * a1
    sd = (R(d0) + d1) - delta * 2.0
    den = delta + sd * t1
    b1 = th2 * d1 + delta * t1 * 2.0 + omt * omt * d0
    dnum = delta * delta * b1
    rden = 1.0 / den
    g_num = rden * gy
    g_den = -((num * rden * gy + 2.0 * gl) * rden)
    g_dnum = gl / dnum
    g_b1, g_a1 = g_dnum * delta * delta, g_num * hk
    g_sd = g_den * t1
    g_delta = g_dnum * 2.0 * delta * b1 + g_b1 * 2.0 * t1 + g_den - g_sd * 2.0 + g_a1 * th2
    g_d1 = g_b1 * th2 + g_sd
    g_d0 = g_b1 * (omt * omt) + g_sd + g_a1 * t1
    g_th2 = g_b1 * d1 + g_a1 * delta
    g_t1 = g_b1 * 2.0 * delta + g_den * sd + g_a1 * d0
    g_omt = g_b1 * d0 * 2.0 * omt + g_t1 * theta
    g_theta = g_th2 * 2.0 * theta + g_t1 * omt - g_omt
    g_hk = g_num * a1 + g_delta * rwk
    g_dx = g_theta * rwk
    g_wk = -((g_theta * theta + g_delta * delta) * rwk)
    first, last = (idx[..., 0] > 0).double(), (idx[..., 0] + 1 < k).double()
    g_xk, g_xk1 = (-g_dx - g_wk) * first, g_wk * last
    g_yk, g_yk1 = (gy - g_hk) * first, g_hk * last
    m = torch.arange(k).expand(r, d_t, k)
    below_lo, below_hi = (m < idx).double(), (m < idx + 1).double()

    def chain(p, g_lo, g_hi, pre_lo, pre_hi):
        w_lo, w_hi = below_lo - pre_lo.unsqueeze(-1), below_hi - pre_hi.unsqueeze(-1)
        return (g_lo.unsqueeze(-1) * w_lo + g_hi.unsqueeze(-1) * w_hi) * ((hi - lo) * cw * inv * p)

    gw, gh = chain(pw, g_xk, g_xk1, pwk, pwk1), chain(ph, g_yk, g_yk1, phk, phk1)
    knot = torch.arange(k + 1).expand(r, d_t, k + 1)
    gd = (g_d0 * s0).unsqueeze(-1) * (knot == idx).double() + (g_d1 * s1).unsqueeze(-1) * (knot == idx + 1).double()
    mask = inside.unsqueeze(-1)
    out = []
    for part in (0, 1):         # values, error bounds
        pick = (lambda t: t.v) if part == 0 else (lambda t: t.e)
        d = pick(gd)[..., 1:-1] if tails else pick(gd)
        gp = torch.cat([pick(gw), pick(gh), d], -1)
        out.append(torch.where(inside, pick(g_dx), gy if part == 0 else torch.zeros_like(gy)))
        out.append(torch.where(mask, gp, torch.zeros_like(gp)).reshape(r, d_t * p_count))
    return out[0], out[1], out[2], out[3]


def check(cs, gx_t, gp):
    """The three per-slice comparisons of a kernel's (gx on the transformed columns, gp) on the distinct rows of ``cs``:
    [(kind, Result)]."""
    r64, r32 = reference(cs.id)
    cond = conditioning(cs.id)
    keep = ~excluded(cs)
    out = []
    for kind in SLICE_KINDS:
        out.append((kind, compare(slices(kind, cs, gx_t, gp, keep), slices(kind, cs, r64[0], r64[1], keep),
                                  slices(kind, cs, r32[0], r32[1], keep), C[cs.entry], cond[kind])))
    return out


# ---- gradients at the knots ------------------------------------------------------------------------------------------------
# The elements every case above leaves out: x on an interior knot of its own spline and within a few float32 ulps of it.  On
# which side of the knot the kernel puts such an element is its own business (the spline is C1, the gradient of logabsdet
# with respect to the parameters is not), so an element passes if it agrees with the float64 gradient taken a little to the
# left of the knot OR a little to the right.  These cases are not part of SPECS: C and COND_MEDIAN are measured without them.

KNOT_SHIFT = 2.0 ** -16          # delta, as a share of the interval: far outside the few-ulp disagreement, well inside a bin
KNOT_NEIGHBOURS = 4              # float32 neighbours of the rounded knot on either side
KNOT_K = 8
KNOT_CASES = collections.OrderedDict([("quadratic-box", ("quadratic", False)), ("cubic-box", ("cubic", False)),
                                      ("quadratic-tails", ("quadratic", True))])


@functools.lru_cache(maxsize=None)
def knot_case(name):
    """d = d_t = 2, one parameter row ~ N(0, 1) shared by all rows; row 9 k + o holds, per dim, the float32 rounding of that
    dim's interior knot k stepped by o - 4 float32 neighbours (``torch.nextafter``): 7 knots x 9 values = 63 rows."""
    kind, tails = KNOT_CASES[name]
    cfg = dict(kind=kind, k=KNOT_K, tails=tails)
    rows = (KNOT_K - 1) * (2 * KNOT_NEIGHBOURS + 1)
    spec = Spec("spline", "spline-knots-" + name, cfg, 2, 2, rows, rows, "knots", ())
    gen = torch.Generator().manual_seed(seed_of(spec))
    p = params_per_dim(spec)
    params = torch.randn(1, 2 * p, generator=gen).expand(rows, 2 * p).contiguous()
    gy, gl = torch.randn(rows, 2, generator=gen), torch.randn(rows, generator=gen)
    cs = Case(spec, "spline", spec.id, cfg, rows, 2, 2, torch.zeros(rows, 2), params, None, gy, gl, None, rows, 0)
    knots = inner_knots(cs)[0].float()                                  # [d_t, K - 1]
    up, down = torch.tensor(float("inf")), torch.tensor(float("-inf"))
    steps = {0: knots}
    for o in range(1, KNOT_NEIGHBOURS + 1):
        steps[o], steps[-o] = torch.nextafter(steps[o - 1], up), torch.nextafter(steps[1 - o], down)
    x = torch.stack([steps[o] for o in range(-KNOT_NEIGHBOURS, KNOT_NEIGHBOURS + 1)], dim=-1)      # [d_t, K - 1, 9]
    return cs._replace(x=x.reshape(2, rows).t().contiguous())


def narrowest_bin(cs):
    """The narrowest bin of a spline case on the x axis, as a share of the interval (float64)."""
    lo, hi = interval(cs.spec)
    r = cs.x.shape[0]
    edges = torch.cat([torch.full((r, cs.d_t, 1), lo, dtype=torch.float64), inner_knots(cs),
                       torch.full((r, cs.d_t, 1), hi, dtype=torch.float64)], dim=-1)
    return float((edges[..., 1:] - edges[..., :-1]).min()) / (hi - lo)


def element_slices(cs, gx_t, gp):
    """[R d_t, 1 + P] float64: per transformed element its gx and its own parameters' gp."""
    gx_t, gp = gx_t.detach().double().cpu(), param_view(cs, gp.detach().double().cpu())
    return torch.cat([gx_t.unsqueeze(-1), gp], dim=-1).reshape(gx_t.numel(), -1)


@functools.lru_cache(maxsize=None)
def knot_reference(name):
    """Per side ("left", "right") of the knots: (float64 gradient slices at x -+ delta, the bound of every element).  The bound
    is the per-slice form of ``compare`` with, in the place of cond, the drift of the one-sided float64 gradient over the
    distance the point was shifted: MARGIN floor + (C + ULP) scale + 2 max |g64(x -+ delta) - g64(x -+ 2 delta)|, the floor
    from the float32 oracle at x -+ delta.  Nothing in it comes from a kernel."""
    cs = knot_case(name)
    lo, hi = interval(cs.spec)
    delta = KNOT_SHIFT * (hi - lo)
    out = {}
    for side, sign in (("left", -1.0), ("right", 1.0)):
        near, far = cs._replace(x=cs.x.double() + sign * delta), cs._replace(x=cs.x.double() + 2 * sign * delta)
        g64 = element_slices(cs, *gradients(near, torch.float64))
        g32 = element_slices(cs, *gradients(near, torch.float32))
        g64_far = element_slices(cs, *gradients(far, torch.float64))
        scale = g64.abs().amax(dim=1)
        floor = (g32 - g64).abs().amax(dim=1)
        drift = 2 * (g64 - g64_far).abs().amax(dim=1)
        out[side] = (g64, MARGIN * floor + (C["spline"] + ULP) * scale + drift)
    return out


def check_knots(name, gx_t, gp):
    """(ok, worst err / bound over the elements -- each on its better side --, a line on the worst element)."""
    cs = knot_case(name)
    got = element_slices(cs, gx_t, gp)
    ratios = []
    for side in ("left", "right"):
        g64, bound = knot_reference(name)[side]
        ratios.append((got - g64).abs().amax(dim=1) / bound.clamp_min(1e-300))
    ratio = torch.minimum(*ratios).nan_to_num(nan=float("inf"))
    finite = bool(torch.isfinite(got).all())
    i = int(ratio.argmax())
    detail = "element %d (row %d, dim %d): err / bound %.3g on the left, %.3g on the right; %d of %d elements fail" % (
        i, i // cs.d_t, i % cs.d_t, ratios[0][i], ratios[1][i], int((ratio > 1).sum()), ratio.numel())
    return finite and bool((ratio <= 1).all()), float(ratio.max()), detail


def round_up_one_digit(v):
    e = math.floor(math.log10(v))
    return float("%.0e" % (math.ceil(v / 10 ** e - 1e-9) * 10 ** e))


def measure_c(entry):
    """(C, median, 90 %, max, slices): floor / scale of the float32 reference over every slice of every case of ``entry``."""
    ratios = []
    for cid in ids(entry):
        cs = case(cid)
        r64, r32 = reference(cid)
        keep = ~excluded(cs)
        for kind in SLICE_KINDS:
            a, b = slices(kind, cs, r64[0], r64[1], keep), slices(kind, cs, r32[0], r32[1], keep)
            scale = a.abs().amax(dim=1)
            ratios.append(((b - a).abs().amax(dim=1) / scale)[scale >= ZERO_SCALE])
    r = torch.cat(ratios)
    med = float(r.median())
    return round_up_one_digit(med), med, float(r.quantile(0.9)), float(r.max()), r.numel()


# ---- the branches a case reaches -------------------------------------------------------------------------------------------

REQUIRED_BRANCHES = {
    "rq": ["wave-K4", "wave-K8", "wave-K16", "generic-K4", "generic-K8", "generic-K16", "runtime-K5", "runtime-K10",
           "runtime-K32", "tails", "box", "below-64-groups", "wave+leftover", "strip-vector", "strip-scalar", "G=1", "G=2",
           "G=8", "G=64", "cols-none", "cols-subset", "misaligned-rows-fallback", "misaligned-params-fallback",
           "lds-fallback", "gl-none", "gy-zero", "wave-trip2", "generic-trip2", "edges", "identity-init", "autograd"],
    "spline": ["%s-%s-K%s" % (kind, _tn(tails), k) for (kind, tails) in SPLINE_MID for k in ("3", "mid", "max")]
              + ["cols-none", "cols-subset", "d_t=1", "lds-64KB", "trip2", "edges"],
    "sos": ["tile", "direct", "tile-partial-group", "tile-whole-groups", "tile-lds-160KB", "tile-trip2", "gl-none", "postact",
            "edges", "direct-edges", "direct-gl-none", "direct-postact", "S=1", "S=6", "S=30", "S=159", "S=160", "S=200"],
    "affine": [a + suffix for a in AFFINE_ACTS for suffix in ("", "-cols-none", "-cols-subset", "-d_t=1", "-edges")] + ["trip2"],
}


def with_cus(cs, cus):
    """``cs`` with the row count its spec has on a device of ``cus`` compute units (the distinct rows do not change)."""
    spec = grid(cus)[cs.id]
    if spec.n == cs.n:
        return cs
    return cs._replace(spec=spec, n=spec.n, idx=torch.arange(spec.n) % spec.distinct)


def branches(spec, cus=CUS_MI355X, aligned_rows=None, aligned_params=None):
    """The names of the launcher branches (and the variants) the case reaches, from the predictors; ``aligned_*``: of the
    launch's own pointers (default: what the variant is meant to have)."""
    cfg, out = spec.cfg, set()
    aligned_rows = spec.variant != "mis_x" if aligned_rows is None else aligned_rows
    aligned_params = spec.variant != "mis_p" if aligned_params is None else aligned_params
    out.add("cols-none" if spec.d_t == spec.d else "cols-subset")
    if spec.variant in ("edges", "gl_none", "gy_zero", "postact", "autograd"):
        out.add(spec.variant.replace("_", "-"))
    if spec.entry == "rq":
        k, tails = cfg["k"], cfg["tails"]
        wave, generic, strip, static = rq_route(spec.n, spec.d, spec.d_t, k, tails, aligned_rows, aligned_params)
        out.add("tails" if tails else "box")
        if cfg.get("ident"):
            out.add("identity-init")
        if not static:
            out.add("runtime-K%d" % k)
        if wave:
            out |= {"wave-K%d" % k, "strip-" + strip, "G=%d" % (64 // spec.d_t)}
            if generic:
                out.add("wave+leftover")
        elif static:
            out.add("generic-K%d" % k)
            aligned = rq_route(spec.n, spec.d, spec.d_t, k, tails)[0] > 0
            if not aligned_rows and aligned and rq_route(spec.n, spec.d, spec.d_t, k, tails, True, aligned_params)[0]:
                out.add("misaligned-rows-fallback")
            elif not aligned_params and aligned and rq_route(spec.n, spec.d, spec.d_t, k, tails, aligned_rows, True)[0]:
                out.add("misaligned-params-fallback")
            elif (spec.d_t & (spec.d_t - 1)) == 0 and spec.n // (64 // spec.d_t) < 64:
                out.add("below-64-groups")
            elif not aligned:
                out.add("lds-fallback")
        trips = rq_trips(wave, generic, spec.d_t)
        if trips[0] > 1:
            out.add("wave-trip2")
        if trips[1] > 1:
            out.add("generic-trip2")
    elif spec.entry == "spline":
        p, k = params_per_dim(spec), cfg["k"]
        which = "3" if k == 3 else ("max" if k == largest_k(cfg["kind"], cfg["tails"]) else "mid")
        out.add("%s-%s-K%s" % (cfg["kind"], _tn(cfg["tails"]), which))
        if 256 * p * 8 == 64 * 1024:
            out.add("lds-64KB")
        if spec.d_t == 1:
            out.add("d_t=1")
        if splines_trips(spec.n * spec.d_t * (p + 1), cus) > 1:
            out.add("trip2")
    elif spec.entry == "sos":
        s, total = cfg["s"], spec.n * spec.d
        kernel, groups, launched = sos_route(total, s, cus)
        out |= {kernel, "S=%d" % s}
        if kernel == "tile":
            out.add("tile-whole-groups" if total % 64 == 0 else "tile-partial-group")
            if 64 * (4 * s + 1) * 4 > 64 * 1024:
                out.add("tile-lds-160KB")
            if groups > launched:
                out.add("tile-trip2")
        elif spec.variant != "plain":
            out.add("direct-" + spec.variant.replace("_", "-"))
    else:
        act = cfg["act"]
        out = {act, "%s-%s" % (act, "cols-none" if spec.d_t == spec.d else "cols-subset")}
        if spec.d_t == 1:
            out.add(act + "-d_t=1")
        if spec.variant == "edges":
            out.add(act + "-edges")
        if affine_trips(spec.n * spec.d_t) > 1:
            out.add("trip2")
    return out


def measure_cond(entry):
    """(median, 90 %) of cond / scale over every slice of every case of ``entry``."""
    ratios = []
    for cid in ids(entry):
        cs = case(cid)
        r64, _ = reference(cid)
        keep = ~excluded(cs)
        for kind in SLICE_KINDS:
            scale = slices(kind, cs, r64[0], r64[1], keep).abs().amax(dim=1)
            ratios.append((conditioning(cid)[kind] / scale)[scale >= ZERO_SCALE])
    r = torch.cat(ratios)
    return float(r.median()), float(r.quantile(0.9))


if __name__ == "__main__":      # (from the repository root: PYTHONPATH=. python tests/_standalone_backward_util.py)
    for name in ENTRIES:
        print("%-6s C = %g   (floor / scale: median %.3g, 90 %% %.3g, max %.3g over %d slices)" % ((name,) + measure_c(name)))
        med, p90 = measure_cond(name)
        print("       cond / scale: median %.3g (recorded as %g), 90 %% %.3g" % (med, round_up_one_digit(med), p90))
    bumped = {cid: case(cid).bump for cid in SPECS if case(cid).bump}
    print("seed bumps:", bumped)
