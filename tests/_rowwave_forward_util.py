"""The forward kernels of the row-per-wavefront family (``fc_householder``, ``fc_planar``, ``fc_sylvester``) and the
matrix-core Sylvester kernel (``fc_sylvester_mm``) against float64: what tests/test_rowwave_forward_host.py and
tests/test_gpu_rowwave_forward.py share.  Nothing here needs a GPU.

Four parts.

1. The three maps written out in torch for any dtype, from the formulas of include/flowcon_hip.h, each with shared and
   with per-sample parameters.  Run in float64 they are the truth; run in float32 on the same inputs they are the
   reference's own arithmetic, whose error is the noise floor.
2. The bound: the row-wise rule of tests/_ar_sampler_util.py, its numbers imported from there.  With e[r] and f[r] the
   kernel's and the float32 reference's error of row r relative to max(1, max_j |ref64[r, j]|):
       max(e) <= 4 max(f) + 1e-5
       Q_p(e) <= 4 Q_p(f) + 2^-23   for p in {0.5, 0.9, 0.99}, for cases of at least 1000 rows
       got is finite wherever float64 is
   applied to y and to logabsdet separately.
3. A mirror of the kernels' launch arithmetic as plain functions of the shape (which instantiation, how many rows a wave
   carries, how many rows one sweep of the persistent loop covers).  Its three constants are compared with the sources
   by the host test.
4. The case tables.  Every row names the instantiation it is meant to reach and, where it matters, the number of sweeps;
   the host test runs the tables through the mirror and counts.
"""
import math

import torch
from torch.nn import functional as F

from _ar_sampler_util import MAX_SLACK, MULTIPLE, ULP, row_error, summary      # summary: p50, p90, p99, max

F32, F64 = torch.float32, torch.float64
QUANTILE_ROWS = 1000      # the quantile lines need a population: cases with at least this many rows

HOUSEHOLDER, PLANAR, SYLVESTER, SYLVESTER_MM, DENSE_MM = ("fc_householder", "fc_planar", "fc_sylvester", "fc_sylvester_mm",
                                                          "fc_dense_mm")
ENTRIES = (HOUSEHOLDER, PLANAR, SYLVESTER, SYLVESTER_MM, DENSE_MM)


# ---- 1. the maps, written out ---------------------------------------------------------------------------------------

def householder_ref(x, q, reverse=False):
    """``out -= (out . q_k) (2 / |q_k|^2) q_k`` for k = 0 .. K-1 (``reverse``: K-1 .. 0); q [K, D] or [N, K, D], K >= 0."""
    k = q.shape[-2]
    out = x
    for i in (range(k - 1, -1, -1) if reverse else range(k)):
        qi = q[..., i, :]
        out = out - (out * qi).sum(-1, keepdim=True) * ((2.0 / (qi * qi).sum(-1, keepdim=True)) * qi)
    return out


def planar_ref(x, w, u_hat, b):
    """``y = x + u_hat tanh(x . w + b)``, ``logabsdet = log(1e-7 + |1 + sum_j u_hat_j (1 - tanh^2) w_j|)``; w, u_hat [D] or
    [1, D] with b [1], or per sample [N, D] with b [N]."""
    d = x.shape[1]
    w, u_hat = w.reshape(-1, d), u_hat.reshape(-1, d)
    t = torch.tanh((x * w).sum(-1) + b.reshape(-1))
    s = (u_hat * ((1 - t * t).unsqueeze(-1) * w)).sum(-1)
    return x + u_hat * t.unsqueeze(-1), torch.log(1e-7 + (1 + s).abs())


def constrained_u(w, u):
    """``u + (softplus(w . u) - 1 - w . u) w / |w|^2`` for w, u [1, D] (planar.py:60-69)."""
    wtu = torch.mm(u, w.T)
    return u + ((-1 + F.softplus(wtu)) - wtu) * (w / (torch.norm(w, p=2, dim=1) ** 2))


def planar_module_ref(x, w, u, b):
    """PlanarTransform.forward (planar.py:30-69): the constraint on u, then the map."""
    return planar_ref(x, w, constrained_u(w, u), b)


def sylvester_ref(x, q, r1, r2, bias, with_args=False):
    """``y = z + Q R2 tanh(R1 Q^T z + bias)`` with Q the reflections q, ``logabsdet = sum_j log(1 + (1 - tanh^2)_j
    diag(R1)_j diag(R2)_j)``.  Shared: q [M, D], R [D, D] multiplied as given (every entry), bias [D].  Per sample:
    q [N, M, D], R [N, D, D] row-major of which the upper triangle only is read, bias [N, D].  ``with_args``: the
    arguments of the logarithm as a third result."""
    if r1.dim() == 3:
        r1, r2 = torch.triu(r1), torch.triu(r2)
        apply = lambda r, v: torch.einsum("nij,nj->ni", r, v)      # noqa: E731
    else:
        apply = lambda r, v: torch.einsum("ij,nj->ni", r, v)       # noqa: E731
    act = torch.tanh(apply(r1, householder_ref(x, q, reverse=True)) + bias)
    y = x + householder_ref(apply(r2, act), q, reverse=False)
    args = 1 + (1 - act * act) * (torch.diagonal(r1, dim1=-2, dim2=-1) * torch.diagonal(r2, dim1=-2, dim2=-1))
    lad = torch.log(args).sum(-1)
    return (y, lad, args) if with_args else (y, lad)


def both(fn, *tensors, **kw):
    """``(fn in float32, fn in float64)`` on the same float32 values."""
    return fn(*[t.to(F32) for t in tensors], **kw), fn(*[t.to(F64) for t in tensors], **kw)


# ---- 2. the bound ----------------------------------------------------------------------------------------------------

RATIOS = {}      # C entry -> (largest max(e) / (4 max(f) + 1e-5) seen in this process, its label)


def _host64(t):
    return t.detach().cpu().to(F64)


def finite_violation(got, ref64):
    """None, or a message when ``got`` is not finite somewhere float64 is."""
    got, ref64 = _host64(got), _host64(ref64)
    fin = torch.isfinite(ref64)
    if bool(torch.isfinite(got[fin]).all()):
        return None
    return "non-finite output at %d places where float64 is finite" % int((~torch.isfinite(got[fin])).sum())


def check(entry, label, got, ref32, ref64, quantiles=None, poisoned=False):
    """The bound on ONE quantity, ``[N, D]`` or ``[N]``.  Prints the case's ``max(e) / (4 max(f) + 1e-5)`` before it
    asserts and returns it.  ``quantiles``: None = by the row count.  ``poisoned``: the case holds rows made non-finite on
    purpose; those only have to be finite where float64 is, every other row enters the error populations.  Without it
    a non-finite float64 value is a broken fixture."""
    got, ref32, ref64 = _host64(got), _host64(ref32), _host64(ref64)
    assert got.shape == ref64.shape, (label, tuple(got.shape), tuple(ref64.shape))
    fin = torch.isfinite(ref64)
    assert poisoned or bool(fin.all()), (label, "fixture: non-finite float64 reference")
    rows = fin if ref64.dim() == 1 else fin.all(dim=1)
    assert bool(rows.any()), (label, "fixture: no finite row")
    assert bool(torch.isfinite(ref32[rows]).all()), (label, "fixture: non-finite float32 reference")
    se, sf = summary(row_error(got[rows], ref64[rows])), summary(row_error(ref32[rows], ref64[rows]))
    ratio = se[3] / (MULTIPLE * sf[3] + MAX_SLACK)
    print("%s %s: max(e) / (4 max(f) + 1e-5) = %.4f   e p50 %.2e p90 %.2e p99 %.2e max %.2e   f %.2e %.2e %.2e %.2e"
          % ((entry, label, ratio) + se + sf))
    if not ratio <= RATIOS.get(entry, (-1.0, ""))[0]:
        RATIOS[entry] = (ratio, label)
    bad = []
    message = finite_violation(got, ref64)
    if message:
        bad.append(message)
    if not se[3] <= MULTIPLE * sf[3] + MAX_SLACK:
        bad.append("max: %.3g > 4 x %.3g + 1e-5" % (se[3], sf[3]))
    if (int(rows.sum()) >= QUANTILE_ROWS) if quantiles is None else quantiles:
        for name, e, f in zip(("p50", "p90", "p99"), se, sf):
            if not e <= MULTIPLE * f + ULP:
                bad.append("%s: %.3g > 4 x %.3g + 2^-23" % (name, e, f))
    assert not bad, "%s %s: %s" % (entry, label, "; ".join(bad))
    return ratio


def check_pair(entry, label, got, ref32, ref64, rows=None, quantiles=None, poisoned=False):
    """``check`` on y and on logabsdet separately; ``got`` / ``ref32`` / ``ref64`` are ``(y, logabsdet)``, ``rows`` an
    optional slice or index of the rows to judge as a group of their own."""
    pick = (lambda t: t) if rows is None else (lambda t: t[rows])
    return max(check(entry, "%s %s" % (label, what), pick(got[i]), pick(ref32[i]), pick(ref64[i]), quantiles, poisoned)
               for i, what in enumerate(("y", "logabsdet")))


# ---- 3. the mirror of the dispatch ----------------------------------------------------------------------------------

K_WAVES_PER_BLOCK = 4             # fc_row.h kWavesPerBlock
K_STREAM_GRID_CAP = 256 * 8       # fc_row.h kStreamGridCap
K_SYL_THREADS = 512               # fc_sylvester_mm.hip kSylThreads
NARROW_FEATURES = 16              # d <= 16: four samples per wave
PLANAR_ROWS4_MAX = 256            # the float4 planar kernel's widest row
CUS = 256                         # compute units of the part the sweep counts are stated for


def elems_for(d):
    return 1 if d <= 64 else 2 if d <= 128 else 4 if d <= 256 else 8


def lanes_for(pieces):
    lanes = 1
    while lanes < pieces:
        lanes <<= 1
    return lanes


def planar_instantiation(d, aligned16=True):
    if d % 4 == 0 and d <= PLANAR_ROWS4_MAX and aligned16:
        return "planar_rows4_kernel<%d>" % lanes_for(d // 4)
    return "planar_kernel<%d>" % elems_for(d)


def householder_instantiation(d):
    return "householder_narrow_kernel" if d <= NARROW_FEATURES else "householder_kernel<%d>" % elems_for(d)


def sylvester_instantiation(d, per_sample):
    return "sylvester_kernel<%d, %s>" % (elems_for(d), "true" if per_sample else "false")


def sylvester_mm_instantiation(d):
    return "sylvester_mm_kernel<%d, false, 1>" % (d // 32)


def rows_per_unit(instantiation):
    """Rows one wave carries per iteration of its loop."""
    if instantiation.startswith("planar_rows4_kernel<"):
        return 64 // int(instantiation[len("planar_rows4_kernel<"):-1])
    return 4 if instantiation == "householder_narrow_kernel" else 1


def sweep_units():
    """Wave-units one sweep of a row kernel's grid covers, once the grid is at its cap."""
    return K_STREAM_GRID_CAP * K_WAVES_PER_BLOCK


def row_sweeps(instantiation, n):
    """``(sweeps, first row of the last sweep, whether the last sweep is partial)`` of a row kernel on n rows."""
    per = rows_per_unit(instantiation)
    units = -(-n // per)
    sweeps = max(1, -(-units // sweep_units()))
    return sweeps, (sweeps - 1) * sweep_units() * per, units % sweep_units() != 0


def sylvester_mm_plan(n, d, cus=CUS):
    """``(workgroups, rows of one sweep, sweeps, whether the last sweep is partial)`` of fc_sylvester_mm on n rows."""
    blocks16 = n // 16
    waves = K_SYL_THREADS // 64
    grid = min(cus * (2 if d <= 64 else 1), -(-blocks16 // waves))
    sweep = grid * waves * 16
    return grid, sweep, -(-n // sweep), n % sweep != 0


def sylvester_mm_full_sweep_rows(d, cus=CUS):
    """Rows that fill every wave of the largest grid exactly once."""
    return cus * (2 if d <= 64 else 1) * (K_SYL_THREADS // 64) * 16


# ---- 4. the case tables ----------------------------------------------------------------------------------------------

WIDTH_ROWS = (1, 5, 67)
WIDE_PER_SAMPLE_ROWS = (1, 5, 9)      # per-sample Sylvester at d >= 257: the matrices are n * d * d

# fc_planar: (d, instantiation).  d / 4 = 3, 5, 9, 25, 33 are the pieces counts that are no power of two.
PLANAR_WIDTHS = [
    (4, "planar_rows4_kernel<1>"), (8, "planar_rows4_kernel<2>"), (12, "planar_rows4_kernel<4>"),
    (16, "planar_rows4_kernel<4>"), (20, "planar_rows4_kernel<8>"), (32, "planar_rows4_kernel<8>"),
    (36, "planar_rows4_kernel<16>"), (64, "planar_rows4_kernel<16>"), (100, "planar_rows4_kernel<32>"),
    (128, "planar_rows4_kernel<32>"), (132, "planar_rows4_kernel<64>"), (256, "planar_rows4_kernel<64>"),
    (1, "planar_kernel<1>"), (2, "planar_kernel<1>"), (3, "planar_kernel<1>"), (63, "planar_kernel<1>"),
    (65, "planar_kernel<2>"), (127, "planar_kernel<2>"), (129, "planar_kernel<4>"), (255, "planar_kernel<4>"),
    (257, "planar_kernel<8>"), (260, "planar_kernel<8>"), (511, "planar_kernel<8>"), (512, "planar_kernel<8>"),
]

# fc_householder, wide kernel: (d, K, instantiation).  Every d, and every K once per register count E.
HOUSEHOLDER_REFLECTIONS = (0, 1, 7, 8, 9, 16, 17, 33)
HOUSEHOLDER_WIDTHS = [(ds[i % len(ds)], k, "householder_kernel<%d>" % e)
                      for e, ds in ((1, (17, 63, 64)), (2, (65, 128)), (4, (129, 256)), (8, (257, 512)))
                      for i, k in enumerate(HOUSEHOLDER_REFLECTIONS)]

# fc_sylvester: (d, M, instantiation)
SYLVESTER_SHARED_WIDTHS = [(d, m, "sylvester_kernel<%d, false>" % e)
                           for d, e in ((1, 1), (2, 1), (33, 1), (64, 1), (65, 2), (128, 2), (129, 4), (200, 4), (256, 4),
                                        (257, 8), (512, 8))
                           for m in (1, 5, 32)]
SYLVESTER_PER_SAMPLE_WIDTHS = [(d, m, "sylvester_kernel<%d, true>" % e)
                               for d, e in ((1, 1), (15, 1), (16, 1), (17, 1), (64, 1), (65, 2), (129, 4), (257, 8))
                               for m in (1, 8, 9, 17)]

# more units than one sweep, the last sweep partial: (name, C entry, instantiation, sweeps, shape)
SWEEP_CASES = [
    ("householder", HOUSEHOLDER, "householder_kernel<2>", 3, dict(d=70, k=3, n=2 * 8192 + 3)),
    ("householder-narrow", HOUSEHOLDER, "householder_narrow_kernel", 3, dict(d=5, k=2, n=2 * 32768 + 3)),
    ("planar", PLANAR, "planar_kernel<1>", 3, dict(d=30, n=2 * 8192 + 3)),
    ("planar-rows4-d64", PLANAR, "planar_rows4_kernel<16>", 3, dict(d=64, n=2 * 32768 + 3)),
    ("planar-rows4-d4", PLANAR, "planar_rows4_kernel<1>", 3, dict(d=4, n=2 * 524288 + 3)),
    ("sylvester-shared", SYLVESTER, "sylvester_kernel<1, false>", 3, dict(d=12, m=5, n=2 * 8192 + 3, per_sample=False)),
    ("sylvester-per-sample", SYLVESTER, "sylvester_kernel<1, true>", 3, dict(d=12, m=5, n=2 * 8192 + 3, per_sample=True)),
]

# fc_sylvester_mm: (d, M, instantiation); the sweep case of each is one full sweep of the device plus 16 rows
SYLVESTER_MM_WIDTHS = [(32, 8, "sylvester_mm_kernel<1, false, 1>"), (64, 16, "sylvester_mm_kernel<2, false, 1>"),
                       (96, 32, "sylvester_mm_kernel<3, false, 1>"), (128, 32, "sylvester_mm_kernel<4, false, 1>")]
SYLVESTER_MM_EDGE_ROWS = (16, 16 * 9, 16 * 23)      # seven idle waves; a second workgroup with one live wave; 23 blocks
SEAM_ROWS = 1024 + 5                                 # a matrix-core body and a row-kernel tail

ALL_INSTANTIATIONS = sorted(
    ["planar_rows4_kernel<%d>" % l for l in (1, 2, 4, 8, 16, 32, 64)]
    + ["%s<%d%s>" % (kernel, e, tail) for kernel, tail in (("planar_kernel", ""), ("householder_kernel", ""),
                                                          ("sylvester_kernel", ", false"), ("sylvester_kernel", ", true"))
       for e in (1, 2, 4, 8)]
    + ["householder_narrow_kernel"] + ["sylvester_mm_kernel<%d, false, 1>" % ks for ks in (1, 2, 3, 4)])


# ---- inputs of the cases (all float32, on the host, from a seeded generator) ------------------------------------------

def _gen(*key):
    return torch.Generator().manual_seed(sum(int(v) * 1000003 ** i for i, v in enumerate(key)) % (2 ** 31))


def householder_inputs(n, d, k, per_sample):
    """x ~ N(0, 1) [n, d] and q ~ N(0, 1), [k, d] or [n, k, d]."""
    g = _gen(1, n, d, k, per_sample)
    x = torch.randn(n, d, generator=g)
    return x, torch.randn(*((n, k, d) if per_sample else (k, d)), generator=g)


def planar_inputs(n, d, per_sample):
    """x ~ N(0, 1); w ~ N(0, 1.5^2 / d), b ~ N(0, 1); u_hat the constrained form of u ~ N(0, 1) (so w . u_hat > -1 and the
    log-determinant's argument stays away from 0), formed in float64 and rounded once."""
    g = _gen(2, n, d, per_sample)
    rows = n if per_sample else 1
    x = torch.randn(n, d, generator=g)
    w = torch.randn(rows, d, generator=g) * (1.5 / math.sqrt(d))
    u = torch.randn(rows, d, generator=g)
    b = torch.randn(rows, generator=g)
    u_hat = torch.cat([constrained_u(w[i:i + 1].double(), u[i:i + 1].double()) for i in range(rows)]).float()
    return x, w, u_hat, b


def sylvester_inputs(n, d, m, per_sample):
    """x, q ~ N(0, 1); R1, R2 upper triangular with off-diagonals ~ N(0, 1 / d) and tanh-squashed N(0, 1) diagonals;
    bias ~ N(0, 0.5^2).  Per sample the strict lower triangles hold junk ~ N(0, 100^2), which must never be read."""
    g = _gen(3, n, d, m, per_sample)
    lead = (n,) if per_sample else ()
    x = torch.randn(n, d, generator=g)
    q = torch.randn(*lead, m, d, generator=g)
    rs = []
    for _ in range(2):
        r = torch.triu(torch.randn(*lead, d, d, generator=g) / math.sqrt(d))
        r.diagonal(dim1=-2, dim2=-1).tanh_()
        if per_sample:
            r = r + torch.tril(torch.randn(n, d, d, generator=g) * 100, -1)
        rs.append(r)
    return x, q, rs[0], rs[1], torch.randn(*lead, d, generator=g) * 0.5


def sylvester_module(d, m, seed, near_singular=False):
    """A SylvesterTransform on the host, its parameters well away from their initial values: q ~ N(0, 1), off-diagonals
    twice their U(-1/sqrt d, 1/sqrt d) initialisation, log-diagonals ~ N(0, 1), bias ~ N(0, 0.3^2).  ``near_singular``:
    log_upper_diag1 = +4 and log_upper_diag2 = -4 on the first half of the features, diag(R1) diag(R2) ~ -0.9987 there."""
    from flowconductor_amd.transforms import SylvesterTransform

    torch.manual_seed(seed)
    t = SylvesterTransform(features=d, num_householder=m, device=None).eval()
    g = _gen(4, d, m, seed)
    with torch.no_grad():
        t.Q_orth.q_vectors.copy_(torch.randn(m, d, generator=g))
        t.upper_entries1.mul_(2.0)
        t.upper_entries2.mul_(2.0)
        t.log_upper_diag1.copy_(torch.randn(d, generator=g))
        t.log_upper_diag2.copy_(torch.randn(d, generator=g))
        t.bias.copy_(torch.randn(d, generator=g) * 0.3)
        if near_singular:
            t.log_upper_diag1[:d // 2] = 4.0
            t.log_upper_diag2[:d // 2] = -4.0
    return t


def module_parameters(t, dtype):
    """``(q, R1, R2, bias)`` of a SylvesterTransform in ``dtype`` on the host, built from its float32 parameters as the
    module builds them (the diagonal's tanh taken in ``dtype``)."""
    d = t.features
    iu = torch.triu_indices(d, d, 1)
    rs = []
    for entries, log_diag in ((t.upper_entries1, t.log_upper_diag1), (t.upper_entries2, t.log_upper_diag2)):
        r = torch.zeros(d, d, dtype=dtype)
        r[iu[0], iu[1]] = entries.detach().cpu().to(dtype)
        r.diagonal().copy_(torch.tanh(log_diag.detach().cpu().to(dtype)))
        rs.append(r)
    return t.Q_orth.q_vectors.detach().cpu().to(dtype), rs[0], rs[1], t.bias.detach().cpu().to(dtype)


def module_refs(t, x, with_args=False):
    """``(float32, float64)`` results of ``sylvester_ref`` for module ``t`` on the float32 rows ``x``."""
    x = x.detach().cpu()
    return tuple(sylvester_ref(x.to(dtype), *module_parameters(t, dtype), with_args=with_args) for dtype in (F32, F64))


def mm_rows(n, d, seed, scale=1.0):
    return torch.randn(n, d, generator=_gen(5, n, d, seed)) * scale


# the strain rows of test_gpu_linear.py::test_split_f16_route_inputs, and one group more: ordinary rows that share their
# 16-row tile with rows holding 7e4 (the odd rows of 48:64; the even ones hold the large entry)
STRAIN_ROWS = 2048
STRAIN_GROUPS = {"1e4": slice(0, 8), "7e4": slice(8, 16), "zero": slice(16, 32), "1e-30": slice(32, 48),
                 "7e4 beside": slice(48, 64, 2), "ordinary beside 7e4": slice(49, 64, 2), "normal": slice(64, STRAIN_ROWS)}


def strain_rows(d, seed):
    x = mm_rows(STRAIN_ROWS, d, seed)
    x[0:8, 5] = 1e4
    x[8:16, 40 % d] = 7e4
    x[16:32] = 0.0
    x[32:48] = x[32:48] * 1e-30
    x[48:64:2, 7] = 7e4
    return x


def poison(x, nan_row, inf_row):
    """``(x with one row of NaN and one row holding an Inf, x with those two rows zeroed)``."""
    bad, zeroed = x.clone(), x.clone()
    bad[nan_row] = float("nan")
    bad[inf_row, 1 % x.shape[1]] = float("inf")
    zeroed[nan_row] = 0.0
    zeroed[inf_row] = 0.0
    return bad, zeroed


def planar_module_inputs(d, n):
    """w, u [1, d] with w . u = -3 (so ``get_constrained_u`` changes u), b [1], x [n, d]."""
    g = _gen(6, d, n)
    w = torch.randn(1, d, generator=g) * (1.5 / math.sqrt(d))
    u = torch.randn(1, d, generator=g)
    u = u - ((u * w).sum() + 3.0) * w / (w * w).sum()
    return torch.randn(n, d, generator=g), w, u, torch.randn(1, generator=g)
