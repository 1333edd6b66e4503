"""Later passes of the hidden-stack kernels' persistent loops (resnet_hidden_kernel without a tail, and
resnet_hidden_wide_kernel): one case per instantiation family that the other files run for a single pass only.  The batch is
the smallest whole number of row blocks for which fc_hidden_route reports two passes, so the last pass is partial; h is
held to the module in float64 on all rows by the row-wise bound of tests/_ar_sampler_util.py, is bit-equal to the same rows
sent in single-pass pieces, and its padding units are exactly 0."""
import collections
import copy

import pytest
import torch
from torch.nn import functional as F

import _affine_tail_util as U
from flowconductor_amd import ops

pytestmark = pytest.mark.gpu

# net: "resnet" (ResidualNet; GLU gate with a context) or "made" (MADE; additive context); width: the kernel's (64: the
# one-wave-per-block kernel, 128 / 256: the wide kernel); d: row width, in_f identity columns picked at random
Case = collections.namedtuple("Case", "name net kind entry width d in_f ctx hidden blocks act")
CASES = [
    Case("glu-context", "resnet", U.GLU, "fc_resnet_hidden_context", 64, 32, 16, 8, 64, 2, F.relu),
    Case("additive-context", "made", U.ADDITIVE, "fc_resnet_hidden_context", 64, 12, 12, 5, 50, 3, F.relu),
    Case("tanh", "resnet", U.STACK, "fc_resnet_hidden", 64, 33, 16, None, 48, 2, torch.tanh),
    Case("two-k-steps", "resnet", U.STACK, "fc_resnet_hidden", 64, 96, 48, None, 56, 2, F.relu),
    Case("four-blocks", "resnet", U.STACK, "fc_resnet_hidden", 64, 48, 24, None, 40, 4, F.relu),
    Case("wide-256-relu", "resnet", U.WIDE, "fc_resnet_hidden_wide", 256, 64, 32, None, 200, 2, F.relu),
    Case("wide-128-silu", "resnet", U.WIDE, "fc_resnet_hidden_wide", 128, 41, 20, None, 100, 2, F.silu),
]


def _route(case, n):
    code, r = U.route(case.kind, n, case.d, case.in_f, case.ctx or 0, case.blocks, case.width)
    assert code == 0, (case.name, n, code)
    return r


def _two_pass_rows(case):
    """Smallest multiple of the kernel's row block that takes two passes: one block more than one pass holds."""
    rows = 64 if case.kind == U.WIDE else 16
    hi = rows
    while _route(case, hi).passes < 2:
        hi *= 2
    lo = hi // 2                      # passes(lo) == 1 (or lo < rows: a single block never takes two)
    while hi - lo > rows:
        mid = (lo + hi) // 2 // rows * rows
        lo, hi = (lo, mid) if _route(case, mid).passes >= 2 else (mid, hi)
    return hi


def _build(case):
    from flowconductor_amd.nn import nets
    from flowconductor_amd.transforms import made

    torch.manual_seed(len(case.name) + case.hidden)
    if case.net == "made":
        net = made.MADE(case.d, case.hidden, context_features=case.ctx, num_blocks=case.blocks, output_multiplier=2,
                        activation=case.act)
    else:
        net = nets.ResidualNet(case.in_f, 8, hidden_features=case.hidden, context_features=case.ctx, num_blocks=case.blocks,
                               activation=case.act)
    net = net.eval()
    with torch.no_grad():
        for p in net.parameters():
            p.mul_(2.0)      # residual blocks / gates far from their near-zero initialisation
    return net


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_later_passes_against_float64_and_single_pass_pieces(case, device):
    n = _two_pass_rows(case)
    rows = 64 if case.kind == U.WIDE else 16
    r, one = _route(case, n), _route(case, n - rows)
    print("route %s: n %d, %d CUs, %d blocks of %d rows, grid %d, passes %d (one pass up to %d rows)"
          % (case.name, n, U.cus(), n // rows, rows, r.grid, r.passes, n - rows))
    assert r.passes == 2 and one.passes == 1 and r.grid == one.grid and n > rows
    net = _build(case)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(n, case.d, generator=g) * 1.3
    c = None if case.ctx is None else torch.randn(n, case.ctx, generator=g) * 1.5
    ids = (torch.arange(case.d) if case.net == "made"
           else torch.randperm(case.d, generator=g)[:case.in_f].sort().values)
    with torch.no_grad():
        args = (x[:, ids],) if c is None else (x[:, ids], c)
        h32 = net.hidden(*args)
        h64 = copy.deepcopy(net).double().hidden(*(a.double() for a in args))
    net = net.to(device)
    xd, idd = x.to(device), ids.to(device)
    cd = None if c is None else c.to(device)

    def run(lo, hi):
        rows_x, rows_c = xd[lo:hi], None if cd is None else cd[lo:hi]
        with torch.no_grad(), ops.KernelTimer(case.entry) as timer:
            if case.kind == U.WIDE:
                assert net.hip_hidden_wide_supported(case.d)
                h = net.hidden_hip_wide(rows_x, idd)
            elif case.net == "made":
                assert net.hip_hidden_supported(rows_c)
                h = net.hidden_hip(rows_x, rows_c)
            else:
                assert net.hip_hidden_supported(case.d, rows_c)
                h = net.hidden_hip(rows_x, idd, rows_c)
        assert len(timer.pairs) == 1, "%s did not run as one launch" % case.entry
        return h

    h = run(0, n)
    assert h.shape == (n, case.width)
    U.check_hidden(case.name, h[:, :case.hidden], h32, h64)
    if case.hidden < case.width:
        assert float(h[:, case.hidden:].abs().max()) == 0.0, "padding units are not exactly 0"
    pieces = torch.cat((run(0, n - rows), run(n - rows, n)))
    assert torch.equal(pieces, h), "rows differ between the two-pass launch and single-pass launches"
