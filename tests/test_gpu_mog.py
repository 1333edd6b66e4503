"""MADEMoG on the GPU: the density kernels (fc_mog_log_prob / _backward) against the reference's fixtures and float64, the
one-kernel sampler (fc_made_mog_sample / _context) against the float64 restatement of the selection rule, routing."""
import copy

import pytest
import torch

import _mog_util as M
from flowconductor_amd import flows, ops, options, transforms

pytestmark = pytest.mark.gpu

KERNEL_SHAPES = [(1, 1, 1), (7, 3, 3), (333, 33, 10), (64, 64, 16)]
EPS = 1e-2


def kernel_inputs(n, d, c, seed=0):
    """x and params with logits spread over +-30, unconstrained stds down to -40 and up past softplus' threshold."""
    g = torch.Generator().manual_seed(100 * d + c + seed)
    x = 2.0 * torch.randn(n, d, generator=g)
    params = torch.randn(n, d, c, 3, generator=g)
    params[..., 0] *= 3.0
    params[..., 1] *= 2.0
    params[0, :, :, 0] = (torch.arange(c) % 2 * 60.0 - 30.0)            # logits at -30 / +30
    params[n // 2, :, 0, 2] = -40.0                                       # std = epsilon
    params[n - 1, :, c - 1, 2] = 25.0                                     # beyond softplus' threshold
    x[n - 1] = 50.0
    return x, params.reshape(n, d * c * 3)


@pytest.mark.parametrize("name", M.FIXTURES)
@pytest.mark.parametrize("rows", [257, 1, 7])
def test_log_prob_matches_reference_fixture(name, rows, device):
    """Bound: 1e-5 of the values' scale + 4 x the fixture's own float32 noise floor -- the bound of test_gpu_golden.py's
    ``_check`` for the maf_affine log-determinants (the same split-f16 hidden stack sits upstream), which is never below
    4 x the floor -- separately on the ordinary rows and on the rows at +-50."""
    g, dims = M.fixture(name)
    dist = M.build(*dims, state=g).to(device)
    x = torch.from_numpy(g["x"][:rows]).to(device)
    context = torch.from_numpy(g["context"][:rows]).to(device) if dims[3] else None
    with torch.no_grad(), ops.KernelTimer("fc_mog_log_prob") as timer:
        lp = dist.log_prob(x, context)
    assert len(timer.pairs) == 1, "the density kernel did not run"
    assert lp.shape == (rows,) and torch.isfinite(lp).all()
    ref = torch.from_numpy(g["log_prob64"][:rows])
    err = (lp.cpu().double() - ref).abs()
    for part, floor in ((slice(0, M.FAR_ROWS), g["floor_far"]), (slice(M.FAR_ROWS, None), g["floor_body"])):
        if err[part].numel():
            bound = 1e-5 * max(1.0, float(ref[part].abs().max())) + 4 * float(floor)
            print(name, rows, "err %.3g bound %.3g floor %.3g" % (err[part].max(), bound, floor))
            assert float(err[part].max()) <= bound


@pytest.mark.parametrize("n,d,c", KERNEL_SHAPES)
def test_log_prob_kernel_alone_against_float64(n, d, c, device):
    """No net upstream: the kernel on given parameters.  Bound: 4 x the error of the float32 torch composition of the
    reference's expression on the same inputs (its own noise floor) + 1e-5 of the scale; everything finite."""
    x, params = kernel_inputs(n, d, c)
    ref = M.density64(params, x, c, EPS).sum(dim=1)
    from flowconductor_amd.nn.nde.made import _mixture_log_density
    ref32 = _mixture_log_density(params.reshape(n, d, c, 3), x, EPS)
    got = ops.mog_log_prob(x.to(device), params.to(device), c, EPS)
    assert torch.isfinite(got).all() and torch.isfinite(ref).all()
    # the last row sits 50 units out and has its own (much larger) scale
    for part in (slice(0, n - 1), slice(n - 1, n)):
        if ref[part].numel():
            err = float((got.cpu().double() - ref)[part].abs().max())
            bound = 1e-5 * max(1.0, float(ref[part].abs().max())) + 4 * float((ref32.double() - ref)[part].abs().max())
            print((n, d, c), "err %.3g bound %.3g" % (err, bound))
            assert err <= bound
    # the accumulate flag adds onto the output
    base = torch.randn(n, generator=torch.Generator().manual_seed(1)).to(device)
    total = ops.mog_log_prob(x.to(device), params.to(device), c, EPS, logp_accum=base.clone())
    assert float((total - (base + got)).abs().max()) <= 1e-6 * max(1.0, float(got.abs().max()))


def test_log_prob_kernel_wide_rows_and_empty_batch(device):
    """d > 256 takes one sample per workgroup in chunks of 256 dims; n = 0 is a no-op."""
    x, params = kernel_inputs(5, 300, 2)
    ref = M.density64(params, x, 2, EPS).sum(dim=1)
    got = ops.mog_log_prob(x.to(device), params.to(device), 2, EPS)
    assert float((got.cpu().double() - ref).abs().max()) <= 2e-5 * float(ref.abs().max())
    assert ops.mog_log_prob(torch.zeros(0, 4, device=device), torch.zeros(0, 4 * 9, device=device), 3, EPS).shape == (0,)


@pytest.mark.parametrize("n,d,c", KERNEL_SHAPES)
def test_backward_kernel_against_float64_autograd(n, d, c, device):
    """grad_x and grad_params against float64 autograd of the reference expression; the bound of
    test_gpu_backward.py::test_affine_backward_matches_torch_autograd: 2e-5 max(1, max |gradient|)."""
    x, params = kernel_inputs(n, d, c, seed=1)
    x[n - 1] = 0.5 * x[0]            # (no row 50 units out: its gradients of 1e7 would set the scale for all the others)
    gl = torch.randn(n, generator=torch.Generator().manual_seed(2))
    x64, p64 = x.double().requires_grad_(True), params.double().requires_grad_(True)
    (M.density64(p64, x64, c, EPS).sum(dim=1) * gl.double()).sum().backward()
    xd, pd = x.to(device).requires_grad_(True), params.to(device).requires_grad_(True)
    with ops.KernelTimer("fc_mog_log_prob_backward") as timer:
        (ops.mog_log_prob(xd, pd, c, EPS) * gl.to(device)).sum().backward()
    assert len(timer.pairs) == 1
    ex = float((xd.grad.cpu().double() - x64.grad).abs().max())
    ep = float((pd.grad.cpu().double() - p64.grad).abs().max())
    sx, sp = max(1.0, float(x64.grad.abs().max())), max(1.0, float(p64.grad.abs().max()))
    print((n, d, c), "grad_x %.3g / %.3g grad_params %.3g / %.3g" % (ex, 2e-5 * sx, ep, 2e-5 * sp))
    assert ex <= 2e-5 * sx and ep <= 2e-5 * sp


@pytest.mark.parametrize("name", ["d5_h32_c5_ctx3_b2", "d33_h24_c10_ctx5_b2"])
def test_parameter_gradients_match_fixture(name, device):
    """Conditioner under torch autograd + fc_mog_log_prob_backward against the reference's float64 gradients; the bound of
    test_gpu_backward.py::test_coupling_layer_trains_through_hip_path (the same composition): 2e-4 of each gradient's scale."""
    g, dims = M.fixture(name)
    dist = M.build(*dims, state=g).to(device)
    x = torch.from_numpy(g["x"]).to(device).requires_grad_(True)
    context = torch.from_numpy(g["context"]).to(device)
    with ops.KernelTimer("fc_mog_log_prob_backward") as timer:
        dist.log_prob(x, context).sum().backward()
    assert len(timer.pairs) == 1
    ref = torch.from_numpy(g["grad_x64"])
    assert float((x.grad.cpu().double() - ref).abs().max()) <= 2e-4 * float(ref.abs().max())
    for pname, p in dist.named_parameters():
        ref = torch.from_numpy(g["grad64::" + pname])
        err, scale = float((p.grad.cpu().double() - ref).abs().max()), max(1e-6, float(ref.abs().max()))
        assert err <= 2e-4 * scale, (pname, err, scale)


# (D, hidden, C, context, blocks, N)
SAMPLER_CASES = [(2, 4, 1, None, 2, 16), (6, 64, 5, None, 2, 1000), (33, 24, 10, 5, 2, 200), (64, 64, 16, 8, 1, 96),
                 (5, 50, 10, 32, 3, 77)]
_sampler_reference = {}


def sampler_case(case):
    """The case's model, noise and float64 restatement, computed once."""
    if case not in _sampler_reference:
        dist = M.build(*case[:5])
        normal, uniform, context = M.noise(case[5], case[0], case[3], seed=sum(case[:3]))
        _sampler_reference[case] = (dist, normal, uniform, context) + M.sample64(dist, normal, uniform, context)
    return _sampler_reference[case]


@pytest.mark.parametrize("case", SAMPLER_CASES)
def test_one_kernel_sampler_against_float64_restatement(case, device):
    dist, normal, uniform, context, x64, keep, logp64 = sampler_case(case)
    assert float(keep.float().mean()) >= 0.95
    dist = copy.deepcopy(dist).to(device)
    dev = [None if t is None else t.to(device) for t in (normal, uniform, context)]
    entry = "fc_made_mog_sample" if context is None else "fc_made_mog_sample_context"
    with ops.KernelTimer(entry) as timer:
        x, logp = dist._made._sample_from_noise(*dev, with_log_prob=True)
    assert len(timer.pairs) == 1, "%s did not run" % entry
    with options.override(ar_device_loop=False), ops.KernelTimer(entry) as timer:
        x_host = dist._sample_from_noise(*dev)
    assert len(timer.pairs) == 0
    scale = max(1.0, float(x64.abs().max()))
    err_host = float((x_host.cpu().double() - x64)[keep].abs().max())
    err = float((x.cpu().double() - x64)[keep].abs().max())
    print(case, "kept %d / %d kernel %.3g host loop %.3g" % (int(keep.sum()), case[5], err, err_host))
    # the yardstick itself picked the float64 run's components on every kept row (another component moves a draw by the
    # distance between two components, not by rounding errors)
    assert err_host <= 1e-3 * scale
    assert err <= 4 * err_host
    # the returned log-density is the density of the draws: the log_prob bound, with the float32 composition's error on
    # these draws as the floor
    with torch.no_grad():
        after = dist.log_prob(x, dev[2])
        cpu = copy.deepcopy(dist).cpu()
        after32 = cpu._made.log_prob_composition(x.cpu(), context)
        after64 = cpu.double()._made.log_prob_composition(x.cpu().double(), None if context is None else context.double())
    floor = float((after32.double() - after64).abs().max())
    bound = 1e-5 * max(1.0, float(after64.abs().max())) + 4 * floor
    assert float((logp.cpu().double() - after.cpu().double()).abs().max()) <= bound
    assert float((logp.cpu().double() - after64)[keep].abs().max()) <= bound


def _spy(monkeypatch):
    names = []
    real = ops.mog._call

    def call(name, *args):
        names.append(name)
        return real(name, *args)

    monkeypatch.setattr(ops.mog, "_call", call)
    return names


def test_routing(device, monkeypatch):
    names = _spy(monkeypatch)
    dist = M.build(6, 64, 5, None, 2).to(device)
    normal, uniform, _ = M.noise(40, 6, None, 3)
    x = dist._sample_from_noise(normal.to(device), uniform.to(device))
    assert "fc_made_mog_sample" in names
    del names[:]
    with options.override(ar_device_loop=False):
        x_host = dist._sample_from_noise(normal.to(device), uniform.to(device))
    assert not any(n.startswith("fc_made_mog_sample") for n in names)
    x64, keep, _ = M.sample64(dist, normal, uniform, None)
    assert float((x.cpu().double() - x64)[keep].abs().max()) <= 1e-4 * max(1.0, float(x64.abs().max()))
    assert float((x_host.cpu().double() - x64)[keep].abs().max()) <= 1e-4 * max(1.0, float(x64.abs().max()))
    # P = 48 at three blocks with a context: no LDS instantiation, the host loop serves
    del names[:]
    wide = M.build(5, 50, 16, 8, 3).to(device)
    normal, uniform, context = M.noise(40, 5, 8, 4)
    assert not ops.made_inverse_context_fits(5, 3, 48)
    x = wide._sample_from_noise(normal.to(device), uniform.to(device), context.to(device))
    assert not any(n.startswith("fc_made_mog_sample") for n in names)
    x64, keep, _ = M.sample64(wide, normal, uniform, context)
    assert float((x.cpu().double() - x64)[keep].abs().max()) <= 1e-4 * max(1.0, float(x64.abs().max()))
    # a shape inside the limits with a context
    del names[:]
    cond = M.build(5, 32, 5, 3, 2).to(device)
    normal, uniform, context = M.noise(40, 5, 3, 5)
    cond._sample_from_noise(normal.to(device), uniform.to(device), context.to(device))
    assert "fc_made_mog_sample_context" in names


def test_shapes_and_flow_composition(device):
    dist = M.build(5, 32, 5, 3, 2).to(device)
    context = torch.randn(3, 3, device=device)
    assert dist.sample(7, context).shape == (3, 7, 5)
    draws, logp = dist.sample_and_log_prob(7, context)
    assert draws.shape == (3, 7, 5) and logp.shape == (3, 7) and draws.is_cuda
    free = M.build(6, 16, 3, None, 1).to(device)
    assert free.sample(7).shape == (7, 6)
    draws, logp = free.sample_and_log_prob(7)
    assert draws.shape == (7, 6) and logp.shape == (7,)
    torch.manual_seed(0)
    flow = flows.Flow(transforms.CompositeTransform([transforms.MaskedAffineAutoregressiveTransform(5, 16, context_features=3)]),
                      M.build(5, 32, 5, 3, 2)).to(device).eval()
    x = torch.randn(33, 5, device=device)
    ctx = torch.randn(33, 3, device=device)
    with torch.no_grad():
        lp = flow.log_prob(x, ctx)
        samples = flow.sample(4, ctx[:3])
    assert lp.shape == (33,) and torch.isfinite(lp).all()
    assert samples.shape == (3, 4, 5) and torch.isfinite(samples).all()
