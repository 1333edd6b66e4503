"""The one-launch autoregressive samplers (fc_made_inverse, fc_made_inverse_context, fc_made_inverse_sos,
fc_made_inverse_spline, fc_made_mog_sample: the device loop of fc_made_inverse.h) held to the row-wise bound of
tests/_ar_sampler_util.py against the float64 oracle, on the one-block-per-wave route at 2053 rows and on the
two-blocks-per-wave route at 256 rows per CU and more.  The host loop (options ar_device_loop = False) meets the same bound
against float64; the two paths are not bounded against each other."""
import copy

import pytest
import torch

import _ar_sampler_util as U
import _mog_util as M
from flowconductor_amd import ops, options
from flowconductor_amd.transforms.made import pad_rows

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", U.CASES, ids=U.case_id)
def test_rows_of_the_device_loop_against_float64(case, device):
    """2053 rows (not a whole 16-row block), one launch of the case's entry."""
    t, x, context, refs = U.references(case)
    t = t.to(device)
    xd = x.to(device)
    cd = None if context is None else context.to(device)
    entry = U.ENTRY[case[0]]
    with torch.no_grad():
        assert t._device_loop_ok(xd, cd)
        with ops.KernelTimer(entry) as timer:
            out = t.inverse(xd, cd)
        assert len(timer.pairs) == 1, "%s did not run as one launch" % entry
        with options.override(ar_device_loop=False), ops.KernelTimer(entry) as timer:
            assert not t._device_loop_ok(xd, cd)
            host = t.inverse(xd, cd)
        assert not timer.pairs
    assert out[0].shape == (U.ROWS, case[3]) and out[1].shape == (U.ROWS,)
    U.check_routes(U.case_id(case), {"device loop": out, "host loop": host}, *refs)


# ---- the two-blocks-per-wave route -------------------------------------------------------------------------------------
def _n_big(device):
    """``launch_made_inverse`` hands a pair of 16-row blocks to every wave from 256 rows per CU on; 53 more rows end the batch
    on a ragged block."""
    return 256 * torch.cuda.get_device_properties(device).multi_processor_count + 16 * 3 + 5


def _subset(n):
    """The rows the oracle is run on: the first 32, the last 64 and 1024 random ones in between (rows are independent)."""
    g = torch.Generator().manual_seed(n)
    middle = torch.randperm(n - 96, generator=g)[:1024].sort().values + 32
    return torch.cat((torch.arange(32), middle, torch.arange(n - 64, n)))


def _report(label, n, device, launches):
    cus = torch.cuda.get_device_properties(device).multi_processor_count
    print("pair route %s: n_big %d >= 256 x %d CUs = %d rows, %d blocks of 16, launches %d"
          % (label, n, cus, 256 * cus, -(-n // 16), launches))
    assert n >= 256 * cus and launches == 1


@pytest.mark.parametrize("case", U.PAIR_CASES + [U.NO_PAIR_CASE], ids=U.case_id)
def test_rows_of_the_two_block_route_against_float64(case, device):
    """Every entry on a shape whose pair instantiation exists (and one whose table entry drops it: the large batch still
    runs as one launch): the row-wise bound on a subset of the rows; the same rows sent as one small batch through the
    one-block route come out bit for bit the same; so does a batch one block shorter, which has an odd number of blocks (the
    last wave repeats a block and must not store it twice); a running log-determinant total gets the stored values added."""
    n = _n_big(device)
    t = U.build(case)
    x, context = U.inputs(case, n)
    rows = _subset(n)
    xs = x[rows].contiguous()
    cs = None if context is None else context[rows].contiguous()
    refs = U.oracle(t, xs, cs)
    t = t.to(device)
    xd, xsd = x.to(device), xs.to(device)
    cd, csd = (None, None) if context is None else (context.to(device), cs.to(device))
    entry = U.ENTRY[case[0]]
    form, per_dim, kw = t._device_loop_form()
    net = t.autoregressive_net

    def through_ops(z, c, total=None):
        """The ``ops`` entry underneath ``t.inverse``: for a running total, and where the layer's own routing rule caps
        its batch below ``n_big`` (the sum-of-sigmoids row limit)."""
        pack, context_pack = net.inverse_packs(per_dim, c is not None)
        y, lad = ops.made_inverse(pad_rows(z), pack, len(net.blocks), per_dim, form, kw, logabsdet_accum=total,
                                  context=None if c is None else pad_rows(c), context_pack=context_pack)
        return y[:z.shape[0]], lad[:z.shape[0]]

    with torch.no_grad():
        assert t._device_loop_ok(xsd, csd)
        run = t.inverse if t._device_loop_ok(xd, cd) else through_ops
        with ops.KernelTimer(entry) as timer:
            y, lad = run(xd, cd)
        _report(U.case_id(case) + ("" if run is not through_ops else " (ops.made_inverse directly)"), n, device, len(timer.pairs))
        with ops.KernelTimer(entry) as timer:
            y_small, lad_small = t.inverse(xsd, csd)
        assert len(timer.pairs) == 1
        odd = n - 16
        assert -(-odd // 16) % 2 == 1 and odd % 16 != 0
        with ops.KernelTimer(entry) as timer:
            y_odd, lad_odd = run(xd[:odd].contiguous(), None if cd is None else cd[:odd].contiguous())
        _report(U.case_id(case) + " one block less", odd, device, len(timer.pairs))
        padded = n + -n % 16
        prior = torch.randn(padded, generator=torch.Generator().manual_seed(3)).mul_(5.0).to(device)
        total = prior.clone()
        with ops.KernelTimer(entry) as timer:
            through_ops(xd, cd, total)
        assert len(timer.pairs) == 1
    assert y.shape == (n, case[3]) and lad.shape == (n,)
    picked = rows.to(device)
    U.check_routes(U.case_id(case), {"pair route": (y[picked], lad[picked]),
                                     "same rows, one block per wave": (y_small, lad_small)}, *refs)
    assert torch.equal(y[picked], y_small) and torch.equal(lad[picked], lad_small), \
        "the one- and two-blocks-per-wave forms differ on the same rows"
    assert torch.equal(y_odd, y[:odd]) and torch.equal(lad_odd, lad[:odd]), "an odd number of blocks changes the rows"
    expect = prior[:n].double() + lad.double()
    assert float(((total[:n].double() - expect).abs() / expect.abs().clamp(min=1.0)).max()) <= 1e-6


def test_mixture_sampler_on_the_two_block_route(device):
    """fc_made_mog_sample (D 8, 10 components, hidden 50, two blocks): the draws and their log-density in the place of the
    outputs and the log-determinant, on the rows whose float64 run is not within 1e-5 of a boundary between two components
    (another component moves a draw by the distance between two components, not by a rounding error).  The float32 yardstick
    is the selection rule's PyTorch composition on the CPU.  The entry has no running-total form."""
    n = _n_big(device)
    dist = M.build(8, 50, 10, None, 2)
    normal, uniform, _ = M.noise(n, 8, None, seed=68)
    rows = _subset(n)
    ns, us = normal[rows].contiguous(), uniform[rows].contiguous()
    x64, keep, logp64 = M.sample64(dist, ns, us, None)
    assert float(keep.float().mean()) >= 0.95
    with torch.no_grad():
        x32, logp32 = copy.deepcopy(dist)._made._sample_host_loop(ns, us, None)
    refs = (x32[keep], logp32[keep], x64[keep], logp64[keep])
    made = copy.deepcopy(dist).to(device)._made
    nd, ud = normal.to(device), uniform.to(device)
    with ops.KernelTimer("fc_made_mog_sample") as timer:
        x, logp = made._sample_from_noise(nd, ud, with_log_prob=True)
    _report("mixture D8 C10 H50 b2", n, device, len(timer.pairs))
    with ops.KernelTimer("fc_made_mog_sample") as timer:
        x_small, logp_small = made._sample_from_noise(ns.to(device), us.to(device), with_log_prob=True)
    assert len(timer.pairs) == 1
    odd = n - 16
    with ops.KernelTimer("fc_made_mog_sample") as timer:
        x_odd, logp_odd = made._sample_from_noise(nd[:odd].contiguous(), ud[:odd].contiguous(), with_log_prob=True)
    _report("mixture one block less", odd, device, len(timer.pairs))
    with options.override(ar_device_loop=False), ops.KernelTimer("fc_made_mog_sample") as timer:
        x_host, logp_host = made._sample_from_noise(ns.to(device), us.to(device), with_log_prob=True)
    assert not timer.pairs
    kept, picked = keep.to(device), rows.to(device)
    U.check_routes("mixture D8 C10 H50 b2", {"pair route": (x[picked][kept], logp[picked][kept]),
                                             "host loop": (x_host[kept], logp_host[kept])}, *refs)
    assert torch.equal(x[picked], x_small) and torch.equal(logp[picked], logp_small), \
        "the one- and two-blocks-per-wave forms differ on the same rows"
    assert torch.equal(x_odd, x[:odd]) and torch.equal(logp_odd, logp[:odd]), "an odd number of blocks changes the rows"
