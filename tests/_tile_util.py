"""Shared by tests/test_tile_route_host.py and tests/test_gpu_tile_routes.py: the launch route of csrc/fc_tile.h as
``fc_tile_route`` reports it, the op configurations and shapes that reach each route, their inputs, the float64 oracle of
each op and the decision points of that oracle.

Everything that decides what a test may leave out is computed from float64 quantities of the oracle alone, and every
noise floor is oracle float32 against oracle float64 on the batch under test: nothing here looks at a kernel's output."""
import collections
import ctypes

import torch

from flowconductor_amd import _hip, ops, options
from oracle import torch_oracle as O

# ---- the route -------------------------------------------------------------------------------------------------------

Route = collections.namedtuple("Route", "pf pf_s pf_tiles left_rows kernel s grid block")
NO_PF, PF61, PF82 = 0, 1, 2            # Route.pf: tile_kernel_pf<Op, 6, 1> / <Op, 8, 2>
NO_KERNEL, VECTOR, SCALAR = 0, 1, 2    # Route.kernel: tile_kernel<Op, true> / <Op, false>


def route(n, d, d_t, rowlen, shared=False, aligned=True):
    """``(return code, Route)`` of fc_tile_route: what launch_tile does for this shape."""
    out = (ctypes.c_int64 * 8)()
    code = _hip.load().fc_tile_route(n, d, d_t, rowlen, int(shared), int(aligned), out)
    return code, Route(*out)


# ---- op configurations -----------------------------------------------------------------------------------------------
# m: parameter floats per transformed dim, what each entry multiplies d_t with for its TileArgs.rowlen.

Config = collections.namedtuple("Config", "family m k tails bound")
CONFIGS = {
    "affine": Config("affine", 2, None, None, None),
    "rq8_tails": Config("rq", 23, 8, "linear", 3.0),
    "rq10_box": Config("rq", 31, 10, None, None),
    "linear8_box": Config("linear", 8, 8, None, None),
    "quadratic8_tails": Config("quadratic", 15, 8, "linear", 2.0),
    "quadratic8_box": Config("quadratic", 17, 8, None, None),
    "cubic8_tails": Config("cubic", 18, 8, "linear", 2.0),
    "cubic15_box": Config("cubic", 32, 15, None, None),
    "sos6": Config("sos", 19, 6, None, None),
    "sos8": Config("sos", 25, 8, None, None),
}
SPLINES = ("rq", "linear", "quadratic", "cubic")
_KIND = {"linear": ops.SPLINE_LINEAR, "quadratic": ops.SPLINE_QUADRATIC, "cubic": ops.SPLINE_CUBIC}


def facade_multiplier(cfg):
    """``m`` as the Python facade computes it for the same entry (a cross-check of the table above)."""
    if cfg.family == "affine":
        return 2
    if cfg.family == "rq":
        return ops.rq_param_count(cfg.k, cfg.tails)
    if cfg.family == "sos":
        return 3 * cfg.k + 1
    return ops.spline_multiplier(_KIND[cfg.family], cfg.k, cfg.tails)


# (N, D, d_t) and the number R of distinct rows: a batch is base[arange(N) % R] with R < 64 S, so the same row lands in
# several persistent tiles and in the leftover tile.  The sum of sigmoids transforms every column: D = d_t there.
SHAPES = {"A": (517, 64, 32), "B": (1031, 96, 16), "C": (100, 130, 65), "D": (259, 60, 60), "G": (3, 6, 3), "H": (257, 8, 4)}
DISTINCT = {"A": 257, "B": 257, "C": 100, "D": 129, "G": 3, "H": 257}


SOS_WIDTH = {"A": 32, "B": 16, "C": 130, "D": 60, "G": 3, "H": 4}       # C: one 130-wide row per tile


def dims(cfg, shape):
    n, d, d_t = SHAPES[shape]
    return (n, SOS_WIDTH[shape], SOS_WIDTH[shape]) if cfg.family == "sos" else (n, d, d_t)


def expected_route(cfg, shape):
    """The route each (configuration, shape) is in the suite for, aligned pointers (tests/test_tile_route_host.py asserts the
    same table against the export on a machine without a GPU)."""
    sos = cfg.family == "sos"
    if shape == "A":        # 8 rows x 32 dims: 64 m parameter float4 per tile, over 6 x 256 from m = 25
        return Route(PF82 if cfg.m >= 25 else PF61, 8, 64, 5, VECTOR, 5, 1, 192)
    if shape == "B":        # 16 rows x 96 floats: 384 input float4 per tile; D = 16: 64, and 64 m parameter float4
        return Route(PF82 if (not sos or cfg.m >= 25) else PF61, 16, 64, 7, VECTOR, 7, 1, 128)
    if shape == "C":        # 3 x 130 is no multiple of 4; D = d_t = 130: one row per tile
        return Route(NO_PF, 0, 0, 0, SCALAR, 1, 100, 192) if sos else Route(NO_PF, 0, 0, 0, SCALAR, 3, 34, 256)
    if shape == "D":        # 4 rows x 60 dims: 60 m parameter float4 per tile, over 6 x 256 from m = 26
        return Route(PF82 if cfg.m >= 26 else PF61, 4, 64, 3, VECTOR, 3, 1, 192)
    if shape == "G":
        return Route(NO_PF, 0, 0, 0, SCALAR, 3, 1, 64)
    return Route(NO_PF, 0, 0, 0, VECTOR, 64, 5, 256)


def columns(cfg, shape):
    """Transformed columns: a non-trivial, unsorted subset (a permutation where every column is transformed)."""
    n, d, d_t = dims(cfg, shape)
    if cfg.family == "sos":
        return None
    if shape == "A":
        return torch.arange(63, 0, -2)                                     # the odd columns, reversed
    if shape == "G":
        return torch.tensor([4, 0, 3])
    if shape == "H":
        return torch.tensor([6, 1, 7, 2])
    gen = torch.Generator().manual_seed(1000 + d)
    return torch.randperm(d, generator=gen)[:d_t]                          # B: 16 of 96, C: 65 of 130, D: all 60, shuffled


def domain(cfg):
    """(left, right) of the spline's interval on both axes; None for the ops defined on the whole line."""
    if cfg.family not in SPLINES:
        return None
    return (-cfg.bound, cfg.bound) if cfg.tails else (0.0, 1.0)


Case = collections.namedtuple("Case", "cfg shape n d d_t x params cols idx distinct")


def make_case(name, shape, seed):
    """float32 CPU tensors of one batch: randn parameters of scale 1; inputs randn * 1.2 where the op has tails or the whole
    line (so some elements of a tailed spline fall in its identity tails), rand * 0.96 + 0.02 on the box; for splines the
    last two distinct rows sit exactly on ``left`` and exactly on ``right``."""
    cfg = CONFIGS[name]
    n, d, d_t = dims(cfg, shape)
    r = DISTINCT[shape]
    gen = torch.Generator().manual_seed(seed)
    dom = domain(cfg)
    if dom is None or cfg.tails:
        x = torch.randn(r, d, generator=gen) * 1.2
    else:
        x = torch.rand(r, d, generator=gen) * 0.96 + 0.02
    if dom is not None:
        x[r - 2] = dom[0]
        x[r - 1] = dom[1]
    params = torch.randn(r, d_t * cfg.m, generator=gen)
    idx = torch.arange(n) % r
    return Case(cfg, shape, n, d, d_t, x[idx].contiguous(), params[idx].contiguous(), columns(cfg, shape), idx, r)


def misaligned(t, device):
    """``t`` on the device in a buffer that starts 4 bytes past a 16-byte boundary."""
    flat = torch.empty(t.numel() + 1, dtype=torch.float32, device=device)
    shifted = flat[1:].reshape(t.shape)
    shifted.copy_(t)
    assert shifted.data_ptr() % 16 == 4
    return shifted


def route_of(cfg, x, params, cols, shared=False):
    """The route of the call ``gpu_apply(cfg, x, params, cols, ...)`` with these very tensors (the outputs are fresh
    allocations, 16-byte aligned)."""
    n, d = x.shape
    d_t = d if cols is None else cols.numel()
    aligned = x.data_ptr() % 16 == 0 and params.data_ptr() % 16 == 0
    code, r = route(n, d, d_t, d_t * cfg.m, shared, aligned)
    assert code == 0
    return r


def gpu_apply(cfg, x, params, cols, inverse, shared=False, **kw):
    """The stand-alone entry of ``cfg`` on device tensors: (y [N, D], logabsdet [N])."""
    with torch.no_grad():
        if cfg.family == "affine":
            return ops.affine_coupling(x, params, cols, activation=ops.AFFINE_SIGMOID_PLUS2, inverse=inverse,
                                       shared_params=shared, **kw)
        if cfg.family == "rq":
            # fc_rq_spline has a register kernel of its own for power-of-two d_t; these tests are about its LDS-tile path
            with options.override(rq_force_tile=True):
                return ops.rq_spline(x, params, cols, num_bins=cfg.k, tails=cfg.tails, tail_bound=cfg.bound or 1.0,
                                     inverse=inverse, shared_params=shared)
        if cfg.family == "sos":
            return ops.sum_of_sigmoids(x, params, cfg.k, inverse=inverse, shared_params=shared)
        return ops.piecewise_spline(x, params, cols, kind=_KIND[cfg.family], num_bins=cfg.k, tails=cfg.tails,
                                    tail_bound=cfg.bound or 1.0, inverse=inverse, shared_params=shared)


# ---- the oracle ------------------------------------------------------------------------------------------------------

def _spline_parts(cfg, rows):
    k = cfg.k
    if cfg.family == "linear":
        return [rows]
    if cfg.family == "quadratic":
        return [rows[..., :k], rows[..., k:]]
    return [rows[..., :k], rows[..., k:2 * k], rows[..., 2 * k:2 * k + 1], rows[..., 2 * k + 1:]]


def oracle(cfg, xt, params, inverse, dtype, **kw):
    """oracle/torch_oracle.py on the transformed columns ``xt`` [N, d_t] and the raw rows ``params`` [N, d_t * m], evaluated
    in ``dtype``: (outputs [N, d_t], logabsdet [N])."""
    n, d_t = xt.shape
    xt = xt.to(dtype)
    with torch.no_grad():
        if cfg.family == "affine":
            scale, shift = O.affine_coupling_scale_shift(params.to(dtype), d_t, "sigmoid")
            return O.affine_elementwise(xt, scale, shift, inverse)
        rows = params.to(dtype).reshape(n, d_t, cfg.m).clone()
        if cfg.family == "rq":
            y, lad = O.rq_from_rows(xt, rows, cfg.k, cfg.tails, cfg.bound, inverse)
            return y, lad.sum(-1)
        if cfg.family == "sos":
            sp, ls, rs, es = torch.split(rows, [cfg.k, cfg.k, cfg.k, 1], dim=-1)

            def forward(v):
                return O.sos_forward(v, sp, ls, rs, es[..., 0])

            if inverse:
                return O.monotonic_inverse(forward, xt, 120, 50)
            return forward(xt)
        fn = {"linear": O.linear_spline, "quadratic": O.quadratic_spline, "cubic": O.cubic_spline}[cfg.family]
        parts = _spline_parts(cfg, rows)
        if cfg.tails:
            y, lad = O._unconstrained(fn, xt, cfg.bound, cfg.tails, parts, inverse=inverse, **kw)
        else:
            y, lad = fn(xt, *parts, inverse=inverse, **kw)
        return y, lad.sum(-1)


def clamp_to_domain(cfg, v, inputs):
    """An un-clamped inverse (the cubic's) may land an ulp outside the interval its input lay in: the oracle's forward
    refuses such a value on a box and takes it for a point of the identity tails otherwise (tests/test_gpu_golden.py
    clamps for the same reason).  Elements whose input lay in the tails stay as they are."""
    dom = domain(cfg)
    if dom is None:
        return v
    inside = (inputs >= dom[0]) & (inputs <= dom[1])
    return torch.where(inside, v.clamp(*dom), v)


def near_inner_knot(xt, raw, k, interval, inverse):
    """Elements [N, d_t] of a linear spline with K bins on ``interval`` whose float64 position on the searched axis (x:
    the knots i / K; the inverse: the cdf knots) lies within 1e-5 of an inner knot.  ``raw``: [N, d_t * K]."""
    n, d_t = xt.shape
    lo, hi = interval
    pos = (xt.double() - lo) / (hi - lo)
    inside = (pos >= 0) & (pos <= 1)
    if inverse:
        knots = torch.cumsum(torch.softmax(raw.double().reshape(n, d_t, k), dim=-1), dim=-1)[..., :-1]
    else:
        knots = (torch.arange(1, k, dtype=torch.float64) / k).expand(n, d_t, k - 1)
    return inside & ((pos[..., None] - knots).abs().min(-1).values < 1e-5)


def decision_points(cfg, xt, params, inverse):
    """Elements [N, d_t] at a decision point of the reference itself, from float64 quantities only:
    * linear spline: the normalised position on the searched axis lies within 1e-5 of an inner knot (logabsdet is
      piecewise constant and jumps there; the outer knots are the ends of the domain, nothing is searched beyond them;
      the other splines have a continuous derivative, a bin chosen differently at a knot moves nothing);
    * cubic inverse: |a| of the element's bin lies within 1e-4 of the 1e-3 threshold below which the reference replaces
      Blinn's root by the root of the bin's quadratic part: exactly the elements whose float64 result depends on whether
      the threshold is 0.9e-3 or 1.1e-3."""
    n, d_t = xt.shape
    none = torch.zeros(n, d_t, dtype=torch.bool)
    if cfg.family == "linear":
        return near_inner_knot(xt, params, cfg.k, domain(cfg), inverse)
    if cfg.family == "cubic" and inverse:
        low, _ = oracle(cfg, xt, params, True, torch.float64, quadratic_threshold=0.9e-3)
        high, _ = oracle(cfg, xt, params, True, torch.float64, quadratic_threshold=1.1e-3)
        return low != high
    return none


MAX_SHARE = 0.005     # of a case's elements at a decision point


def bound_of(ref, floor):
    """tests/test_gpu_golden.py: 1e-5 of the tensor's magnitude plus 4 x the reference's own float32 noise floor."""
    return 1e-5 * max(1.0, float(ref.abs().max())) + 4.0 * floor


def maxabs(t):
    return float(t.abs().max()) if t.numel() else 0.0


def needed_multiple(err, ref, floor):
    """The multiple of the floor that ``err`` needs in ``bound_of`` (0: the 1e-5 term alone covers it)."""
    over = err - 1e-5 * max(1.0, float(ref.abs().max()))
    if over <= 0:
        return 0.0
    return over / floor if floor > 0 else float("inf")
