"""Cases, oracle and bound for the one-kernel affine layer (fc_affine_coupling_resnet) and its sibling hidden-stack kernels,
shared by tests/test_affine_tail_host.py, tests/test_gpu_affine_tail.py and tests/test_gpu_hidden_passes.py.

The layer is one conditioner pass, so the oracle (oracle/torch_oracle.py in float32 and in float64) runs on EVERY row of a
launch, and the rows are held to the row-wise population bound of tests/_ar_sampler_util.py, unchanged: the transformed
columns and the log-determinant separately, each against the float32 oracle's error on the very same rows; identity and
ride-along columns bit-equal to the input.

Which launch a shape takes is asked from ``fc_hidden_route`` (the host functions the launches themselves call), never
worked out by hand: ``route`` below.  The pair route (two 16-row blocks per wave) starts at 256 rows per CU, so ``n_big`` is
the smallest batch at which it can go wrong; it has an odd number of blocks, so its last group repeats a block."""
import collections
import copy
import ctypes

import torch

import _ar_sampler_util as A
from flowconductor_amd import _hip
from oracle import torch_oracle as O

STACK, GLU, ADDITIVE, TAIL, WIDE = range(5)            # FC_ROUTE_* of include/flowcon_hip.h
Route = collections.namedtuple("Route", "bpw xvt grid waves lds passes repeats code")
LDS_PER_CU = 160 * 1024


def route(kind, n, d, in_features, context_features=0, blocks=2, hidden=64):
    """``(return code, Route)`` of fc_hidden_route: what the entry behind ``kind`` launches for this shape."""
    out = (ctypes.c_int64 * 8)()
    code = _hip.load().fc_hidden_route(kind, n, d, in_features, context_features, blocks, hidden, out)
    return code, Route(*out)


def cus():
    """CUs of the current device as the launches count them (256 without a device): a batch large enough fills them."""
    return route(TAIL, 1 << 26, 8, 4, 0, 0)[1].grid


def n_big(leftover=5):
    """256 rows per CU, three more blocks (an odd block count) and ``leftover`` rows for the stand-alone path."""
    return 256 * cus() + 3 * 16 + leftover


def n_mid():
    """Between the thresholds: more than one pass of single blocks (128 rows per CU), not yet pairs (256 per CU)."""
    return 192 * cus() + 3 * 16


# ---- the cases ----------------------------------------------------------------------------------------------------------
# kind: affine (sigmoid(u + 2) + 1e-3), general (softplus + 1e-3 clamped at 3), additive, maf (density direction of a
# masked-autoregressive affine layer: every column read AND transformed).
# mask: "alt" alternating, ("split", k) the first k columns identity, ("random", k, seed) k random identity columns.
# ride > 0: the layer lives on ``d`` randomly chosen columns of rows ``d + ride`` wide; the others are neither read nor
# transformed (only reachable through ops.affine_coupling_resnet).
Case = collections.namedtuple("Case", "kind d mask hidden blocks seed ride", defaults=(0,))

CASES = [
    # D <= 32: the pair route keeps 2 row pieces per lane
    Case("affine", 32, "alt", 64, 2, 11),
    Case("general", 31, ("random", 15, 3), 64, 0, 12),          # D % 4 == 3, a non-alternating mask
    Case("affine", 29, ("split", 28), 48, 1, 13),               # D % 4 == 1, d_t = 1
    Case("additive", 18, ("split", 1), 64, 3, 14),              # D % 4 == 2, one identity feature
    Case("maf", 32, None, 64, 3, 15),                           # d_t = 32
    Case("maf", 7, None, 32, 2, 16),
    Case("maf", 2, None, 4, 1, 17),                             # the README flow's layer
    # 32 < D <= 64: 4 row pieces per lane
    Case("affine", 64, "alt", 64, 2, 21),                       # d_t = 32
    Case("general", 33, ("random", 8, 5), 64, 3, 22),           # D % 4 == 1; (D | 1) <= 37: the pair form of 3 blocks exists
    Case("additive", 40, "alt", 64, 0, 23),
    Case("affine", 35, ("split", 20), 50, 1, 24),               # D % 4 == 3
    Case("general", 50, ("split", 34), 64, 0, 25),              # two k-steps of the initial layer from here on
    Case("affine", 64, ("split", 33), 64, 1, 26),               # 33 identity features
    Case("general", 60, ("random", 40, 7), 64, 2, 27),          # (D | 1) <= 61: the pair form of 2 blocks + 2 k-steps exists
    # the table drops the pair form (3 blocks: 126 KB of weights + two [16][65] tiles per wave > 160 KB)
    Case("general", 64, "alt", 64, 3, 31),
    # D > 64: one block per wave at any batch
    Case("affine", 65, ("split", 64), 64, 2, 41),               # 64 identity features, d_t = 1
    Case("general", 96, ("split", 64), 64, 2, 42),              # d_t = 32
    Case("affine", 64, ("random", 40, 9), 64, 1, 43, 64),       # D = 128: 64 columns ride along
    Case("additive", 48, "alt", 64, 2, 44),                     # D <= 64, for the batch between the thresholds
]
# every weight image of the one-block kernel: NB 0..3 x K0S 1, 2 (the activation is swept by the test)
IMAGES = [(nb, k0s) for nb in range(4) for k0s in (1, 2)]


def case_id(case):
    mask = "" if case.mask is None else "-alt" if case.mask == "alt" else "-%s%d" % (case.mask[0], case.mask[1])
    return "%s-D%d%s-H%d-b%d%s" % (case.kind, case.d + case.ride, mask, case.hidden, case.blocks,
                                   "-ride%d" % case.ride if case.ride else "")


def image_case(nb, k0s, kind):
    """The smallest-width case of a weight image: D 40 with 34 identity features for two k-steps, D 12 for one."""
    if kind == "maf":
        return Case("maf", 12, None, 64, nb, 60 + nb)
    return Case(kind, 40, ("split", 34), 64, nb, 70 + nb) if k0s == 2 else Case(kind, 12, "alt", 48, nb, 80 + nb)


def identity_mask(case):
    """Boolean [d]: True where the column is an identity column of the coupling layer."""
    if case.mask == "alt":
        return torch.arange(case.d) % 2 == 1       # create_alternating_binary_mask(even=True) transforms 0, 2, ...
    ident = torch.zeros(case.d, dtype=torch.bool)
    if case.mask[0] == "split":
        ident[:case.mask[1]] = True
    else:
        g = torch.Generator().manual_seed(case.mask[2])
        ident[torch.randperm(case.d, generator=g)[:case.mask[1]]] = True
    return ident


def dims(case):
    """``(row width, in_features, d_t, blocks)`` as the entry sees them."""
    if case.kind == "maf":
        return case.d, case.d, case.d, case.blocks
    k = int(identity_mask(case).sum())
    return case.d + case.ride, k, case.d - k, case.blocks


def tail_route(case, n):
    width, in_features, _, blocks = dims(case)
    return route(TAIL, n - n % 16, width, in_features, 0, blocks)


def build(case):
    """The case's layer on the CPU in eval mode: parameters times 1.7, a random bias on the final layer."""
    from flowconductor_amd import transforms as T
    from flowconductor_amd.nn import nets

    torch.manual_seed(case.seed)
    if case.kind == "maf":
        t = T.MaskedAffineAutoregressiveTransform(case.d, case.hidden, num_blocks=case.blocks)
        final = t.autoregressive_net.final_layer
    else:
        mask = torch.where(identity_mask(case), -1.0, 1.0)

        def net(i, o):
            return nets.ResidualNet(i, o, hidden_features=case.hidden, num_blocks=case.blocks)

        if case.kind == "additive":
            t = T.AdditiveCouplingTransform(mask, net)
        else:
            act = (T.AffineCouplingTransform.GENERAL_SCALE_ACTIVATION if case.kind == "general"
                   else T.AffineCouplingTransform.DEFAULT_SCALE_ACTIVATION)
            t = T.AffineCouplingTransform(mask, net, scale_activation=act)
        final = t.transform_net.final_layer
    t = t.eval()
    with torch.no_grad():
        for p in t.parameters():
            p.mul_(1.7)
        final.bias.add_(torch.randn_like(final.bias) * 0.3)
    return t


def used_columns(case):
    """Columns of the ``d + ride`` wide rows the layer lives on (all of them without ride-along columns)."""
    if not case.ride:
        return torch.arange(case.d)
    g = torch.Generator().manual_seed(case.seed)
    return torch.randperm(case.d + case.ride, generator=g)[:case.d].sort().values


def transformed_columns(case):
    used = used_columns(case)
    return used if case.kind == "maf" else used[~identity_mask(case)]


def inputs(case, n):
    g = torch.Generator().manual_seed(5)
    return torch.randn(n, case.d + case.ride, generator=g) * 1.3


def oracle(t, case, x, inverse):
    """The oracle on the rows of ``x`` in float32 and float64: ``(y32, lad32, y64, lad64)``, rows as wide as ``x``."""
    used = used_columns(case)
    out = []
    with torch.no_grad():
        for layer, rows in ((t, x), (copy.deepcopy(t).double(), x.double())):
            y, lad = O.transform_apply(layer, rows[:, used].contiguous(), None, inverse=inverse)
            full = rows.clone()
            full[:, used] = y
            out += [full, lad]
    return tuple(out)


_REFS = {}


def references(case, n, inverse, x=None):
    """``(layer on the CPU, x, (y32, lad32, y64, lad64))``; computed once per (case, n, direction) and never changed."""
    key = (case, n, inverse)
    if key not in _REFS:
        t = build(case)
        rows = inputs(case, n) if x is None else x
        _REFS[key] = (t, rows, oracle(t, case, rows, inverse))
    t, rows, refs = _REFS[key]
    return copy.deepcopy(t), rows.clone(), refs


def check_fixture(case, refs):
    """On the reference alone: float64 finite, at most 1 % of the rows beyond 1e3."""
    cols = transformed_columns(case)
    A.check_fixture(refs[2][:, cols], refs[3])
    assert bool(torch.isfinite(refs[0]).all()) and bool(torch.isfinite(refs[1]).all()), "fixture: non-finite float32 oracle"


def check(label, case, x, got, refs):
    """The row-wise bound on the transformed columns and on the log-determinant, each on its own; every other column
    bit-equal to the input.  Prints the population summary before it judges; returns it."""
    y, lad = got[0].detach().cpu(), got[1].detach().cpu()
    y32, lad32, y64, lad64 = refs
    check_fixture(case, refs)
    assert y.shape == x.shape and lad.shape == (x.shape[0],)
    cols = transformed_columns(case)
    rest = torch.ones(x.shape[1], dtype=torch.bool)
    rest[cols] = False
    bad_y, stats_y = A.quantity_violations("y", y[:, cols], y32[:, cols], y64[:, cols])
    bad_l, stats_l = A.quantity_violations("lad", lad, lad32, lad64)
    stats = {"y": stats_y, "lad": stats_l}
    print(A.format_stats(label, stats))
    assert torch.equal(y[:, rest], x[:, rest]), "%s: identity / ride-along columns are not the input's bits" % label
    assert not bad_y + bad_l, "%s: %s" % (label, "; ".join(bad_y + bad_l))
    return stats


def check_hidden(label, h, h32, h64):
    """The same bound on a bare ``[N, H]`` output."""
    assert bool(torch.isfinite(h64).all()) and bool(torch.isfinite(h32).all()), "fixture: non-finite reference"
    bad, stats = A.quantity_violations("h", h.detach().cpu(), h32, h64)
    print(A.format_stats(label, {"h": stats}))
    assert not bad, "%s: %s" % (label, "; ".join(bad))
    return stats


# ---- running the layer on the device --------------------------------------------------------------------------------------
def run(t, case, x, inverse, total=None):
    """The layer ``t`` (on the device) on the device rows ``x``: through the module where it reaches the shape, else
    through ops.affine_coupling_resnet with the module's own weight image.  ``total`` [n]: the running log-determinant
    the kernel adds onto (returned in the log-determinant's place)."""
    from flowconductor_amd import ops

    with torch.no_grad():
        if not case.ride:
            assert t._one_kernel_ok(x, None)
            if total is not None:
                return t._apply_accumulate(x, None, inverse, total), total
            return (t.inverse if inverse else t)(x)
        assert x.shape[0] % 16 == 0
        net = t.transform_net
        d_t = t.num_transform_features
        pack, image = ops.device_pack_affine_coupling(net, d_t, t._activation_code() == ops.AFFINE_ADDITIVE)
        pack.refresh()
        used = used_columns(case).to(x.device)
        return ops.affine_coupling_resnet(x, used[t.identity_features.to(x.device)], used[t.transform_features.to(x.device)],
                                          image, net.initial_layer.in_features, len(net.blocks), t._activation_code(),
                                          inverse=inverse, logabsdet_accum=total)


def directions(case):
    return (False,) if case.kind == "maf" else (False, True)


# ---- the table of the coupling tail, from fc_hidden_route ----------------------------------------------------------------
def reachable(n):
    """Every ``(NB, K0S, blocks per wave, XVT)`` the entry launches at ``n`` rows for some width: in_features <= 32 exists at
    every D, in_features > 32 from D 33 on."""
    found = set()
    for nb in range(4):
        for k0s in (1, 2):
            for d in range(1 if k0s == 1 else 33, 129):
                code, r = route(TAIL, n, d, min(d, 32) if k0s == 1 else 33, 0, nb)
                if code == 0:
                    found.add((nb, k0s, r.bpw, r.xvt))
    return found


def instantiation(case, n):
    """``(NB, K0S, blocks per wave, XVT)`` of ``case`` at ``n`` rows."""
    code, r = tail_route(case, n)
    assert code == 0, (case, n, code)
    return case.blocks, 1 if dims(case)[1] <= 32 else 2, r.bpw, r.xvt


def pair_cases(n):
    return [c for c in CASES if instantiation(c, n)[2] == 2]


def format_route(label, case, n, r):
    return "route %s: n %d, %d CUs, %d blocks of 16, %d per wave, XVT %d, grid %d, passes %d%s" % (
        label, n, cus(), n // 16, r.bpw, r.xvt, r.grid, r.passes, ", last group repeats a block" if r.repeats else "")
