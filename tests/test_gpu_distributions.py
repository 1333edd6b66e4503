"""The discrete / uniform base kernels on the GPU (fc_bernoulli_log_prob and its backward, fc_bernoulli_sample,
fc_box_log_prob) and the classes over them, against the reference's float64 fixtures of
tests/golden/make_distributions_golden.py.

Margins.  Fixture comparisons use ``_distributions_util.bound``: 4 x the fixture's stored float32 noise floor, never below 4
float32 ulps of the largest magnitude compared.  The layout tests run on seeded inputs without a fixture; their bounds come
from the number format alone (EPS = 2^-23):
  log_prob        a summand is (x - step) l - log1p(exp(-|l|)): at most ~4 rounded operations at <= 2 EPS each, and a lane
                  sum plus a 6-level butterfly adds <= 8 roundings of a partial sum -> 16 EPS max_row sum_d |summand|
  grad_logits     g (x - sigmoid(l)), |x - sigmoid| <= 1, sigmoid good to 2 EPS -> 8 EPS |g|
  grad_inputs     g l, one rounding -> EPS |g l|
  samples         exact wherever |noise - sigmoid64(l)| >= 1e-6 (a float32 sigmoid is good to 2.4e-7)
  box             -inf rows exact; the finite value is a sum of d logarithms -> (d + 8) EPS sum_d |log(high - low)|
"""
import pytest
import torch

import _distributions_util as U
from flowconductor_amd import distributions, ops
from flowconductor_amd.distributions.uniform import BoxUniform, LotkaVolterraOscillating, MG1Uniform

pytestmark = pytest.mark.gpu


# ---- the Bernoulli likelihood against the fixtures ------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(U.BERNOULLI))
def test_log_prob_matches_the_float64_fixture(name, device):
    t = U.fixture("bernoulli_" + name)
    dist = U.build_bernoulli(name, device)
    x, context = t["x"].to(device), t["context"].to(device)
    with torch.no_grad(), ops.KernelTimer("fc_bernoulli_log_prob") as timer:
        logp = dist.log_prob(x, context=context)
        mean = dist.mean(context)
        logits = dist._compute_params(context)
        direct = ops.bernoulli_log_prob(x, logits)
    assert len(timer.pairs) == 2, "the HIP kernel did not run"
    assert logp.is_cuda and logp.dtype == torch.float32 and logp.shape == t["logp64"].shape and torch.equal(logp, direct)
    U.check(name + " log_prob", logp, t["logp64"], t["floor_logp"])
    U.check(name + " mean", mean, t["mean64"], t["floor_mean"])


@pytest.mark.parametrize("name", U.WITH_GRADIENTS)
def test_gradients_match_the_float64_fixture(name, device):
    t = U.fixture("bernoulli_" + name)
    dist = U.build_bernoulli(name, device)
    context, taps = U.tap_logits(dist, t["context"].to(device))
    x = t["x"].to(device).requires_grad_(True)
    with ops.KernelTimer("fc_bernoulli_log_prob_backward") as timer:
        logp = dist.log_prob(x, context=context)
        (logp * t["g"].to(device)).sum().backward()
    assert len(timer.pairs) == 1, "one backward launch"
    U.check(name + " log_prob (with a graph)", logp, t["logp64"], t["floor_logp"])
    U.check(name + " grad logits", taps[0].grad.reshape(x.shape), t["grad_logits64"], t["floor_grad_logits"])
    U.check(name + " grad inputs", x.grad, t["grad_x64"], t["floor_grad_x"])
    for key, p in dist.named_parameters():
        key = key[len("_context_encoder."):]
        U.check("%s grad %s" % (name, key), p.grad, t["grad64::" + key], t["floor_grad::" + key])


def _logits_of(name, device):
    t = U.fixture("bernoulli_" + name)
    with torch.no_grad():
        return t, U.build_bernoulli(name, device)._compute_params(t["context"].to(device)).contiguous()


def test_one_sided_gradients_add_and_fallbacks(device):
    t, logits = _logits_of("d130", device)
    x, g = t["x"].to(device), t["g"].to(device)
    with torch.no_grad():
        plain = ops.bernoulli_log_prob(x, logits)
    # only the inputs require a gradient
    xi = x.clone().requires_grad_(True)
    li = logits.clone()
    out = ops.bernoulli_log_prob(xi, li)
    (out * g).sum().backward()
    assert torch.equal(out.detach(), plain) and li.grad is None
    U.check("inputs only", xi.grad, t["grad_x64"], t["floor_grad_x"])
    # only the logits require one
    xl = x.clone()
    ll = logits.clone().requires_grad_(True)
    out = ops.bernoulli_log_prob(xl, ll)
    (out * g).sum().backward()
    assert torch.equal(out.detach(), plain) and xl.grad is None
    U.check("logits only", ll.grad, t["grad_logits64"], t["floor_grad_logits"])
    # the Function itself hands back None for the side that was not asked for
    gx, gl, ga = _apply_backward(x, logits, g, (True, False, False))
    assert gl is None and ga is None and torch.equal(gx, xi.grad)
    gx, gl, ga = _apply_backward(x, logits, g, (False, True, False))
    assert gx is None and ga is None and torch.equal(gl, ll.grad)
    # add= is the sum, in the same pass; its gradient is the row gradient
    add = torch.randn(x.shape[0], device=device, generator=torch.Generator(device).manual_seed(5))
    assert torch.equal(ops.bernoulli_log_prob(x, logits, add=add), plain + add)
    add_g = add.clone().requires_grad_(True)
    lg = logits.clone().requires_grad_(True)
    out = ops.bernoulli_log_prob(x, lg, add=add_g)
    (out * g).sum().backward()
    assert torch.equal(out.detach(), plain + add) and torch.equal(add_g.grad, g) and torch.equal(lg.grad, ll.grad)
    # the gradient of a plain sum arrives as an expanded scalar
    ls = logits.clone().requires_grad_(True)
    ops.bernoulli_log_prob(x, ls).sum().backward()
    U.check("sum", ls.grad, (t["x"].double() - torch.sigmoid(logits.cpu().double())), 0.0)
    # float64 and non-contiguous inputs take the composition and agree
    with torch.no_grad(), ops.KernelTimer("fc_bernoulli_log_prob") as timer:
        wide = ops.bernoulli_log_prob(x.double(), logits.double())
        strided = ops.bernoulli_log_prob(x.t().contiguous().t(), logits)
    assert len(timer.pairs) == 0 and wide.dtype == torch.float64
    assert float((wide.cpu() - t["logp64"]).abs().max()) <= 1e-6 * float(t["logp64"].abs().max())   # (float32 logits, widened)
    U.check("strided", strided, t["logp64"], t["floor_logp"])
    # a double backward goes through the torch expression
    l2 = logits[:8].clone().requires_grad_(True)
    (first,) = torch.autograd.grad(ops.bernoulli_log_prob(x[:8], l2).sum(), l2, create_graph=True)
    (second,) = torch.autograd.grad(first.sum(), l2)
    p = torch.sigmoid(l2.detach())
    assert float((second + p * (1 - p)).abs().max()) <= 8 * U.EPS


def _apply_backward(x, logits, g, needs):
    class Ctx:
        saved_tensors = (x, logits)
        needs_input_grad = needs
    with torch.no_grad():
        return ops._BernoulliLogProbFunction.backward(Ctx, g)


# ---- the sampler ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", U.SAMPLES)
def test_samples_equal_the_reference_exactly(name, device):
    t = U.fixture("bernoulli_sample_" + name)
    contexts, draws = t["samples32"].shape[:2]
    with ops.KernelTimer("fc_bernoulli_sample") as timer:
        got = ops.bernoulli_sample(t["logits"].to(device), t["noise"].to(device), draws)
    assert len(timer.pairs) == 1 and got.is_cuda and got.dtype == torch.float32 and got.shape == t["noise"].shape
    assert torch.equal(got.cpu().reshape(t["samples32"].shape), t["samples32"])


def test_class_sampler_draws_rand_on_the_device(device):
    torch.manual_seed(0)
    dist = distributions.ConditionalIndependentBernoulli([2, 3], torch.nn.Linear(4, 6)).to(device)
    context = torch.randn(5, 4, device=device)
    for seed in (1, 2):
        torch.manual_seed(seed)
        draws = dist.sample(7, context=context)
        torch.manual_seed(seed)
        noise = torch.rand(35, 2, 3, device=device)
        with torch.no_grad():
            expected = ops.bernoulli_sample(dist._compute_params(context), noise, 7)
        assert draws.device == context.device and draws.dtype == torch.float32 and draws.shape == (5, 7, 2, 3)
        assert torch.equal(draws, expected.reshape(5, 7, 2, 3))
    both, logp = dist.sample_and_log_prob(3, context=context)
    assert both.shape == (5, 3, 2, 3) and logp.shape == (5, 3) and logp.is_cuda


def test_empirical_frequencies(device):
    contexts, draws, d = 3, 20000, 10
    logits = torch.linspace(-3, 3, contexts * d).reshape(contexts, d)
    dist = distributions.ConditionalIndependentBernoulli([d])
    torch.manual_seed(123)
    samples = dist.sample(draws, context=logits.to(device))
    assert samples.shape == (contexts, draws, d) and samples.is_cuda and samples.dtype == torch.float32
    p = torch.sigmoid(logits.double())
    deviation = (samples.double().mean(1).cpu() - p).abs() / torch.sqrt(p * (1 - p) / draws)
    print("largest deviation %.2f standard deviations" % float(deviation.max()))
    assert float(deviation.max()) <= 5.0


# ---- the box --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", U.BOX)
def test_box_log_prob_matches_the_fixture(d, device):
    t = U.fixture("box_d%d" % d)
    low, high, x = t["low"].to(device), t["high"].to(device), t["x"].to(device)
    box = BoxUniform(low, high, validate_args=False)
    reference_outside = torch.isinf(t["logp64"])
    with ops.KernelTimer("fc_box_log_prob") as timer:
        results = (box.log_prob(x), ops.box_log_prob(x, low, high))
    assert len(timer.pairs) == 2
    for got in results:
        got = got.cpu()
        outside = torch.isinf(got)
        assert got.dtype == torch.float32 and not torch.isnan(got).any() and bool((got[outside] < 0).all())
        assert torch.equal(outside, reference_outside)                  # boundary rows and the NaN row included
        U.check("box_d%d" % d, got[~outside], t["logp64"][~outside], t["floor_logp"])
    checked = BoxUniform(low, high)
    if bool(t["default_validation_raises"]):
        with pytest.raises(ValueError, match="to be within the support"):
            checked.log_prob(x)
    inside = x[~reference_outside.to(device)]
    U.check("box_d%d validated" % d, checked.log_prob(inside), t["logp64"][~reference_outside], t["floor_logp"])
    assert checked.sample((4,)).is_cuda and isinstance(checked, torch.distributions.Independent)


def test_sbi_priors_on_device_tensors(device):
    t = U.fixture("sbi_priors")
    mg1 = MG1Uniform(t["mg1_low"].to(device), t["mg1_high"].to(device), validate_args=False)
    got = mg1.log_prob(t["mg1_x"].to(device)).cpu()
    outside = torch.isinf(got)
    assert got.shape == (64, 3) and torch.equal(outside, torch.isinf(t["mg1_logp64"]))
    U.check("mg1", got[~outside], t["mg1_logp64"][~outside], t["mg1_floor"])
    assert mg1.sample((9,)).is_cuda

    prior = LotkaVolterraOscillating(device=device)
    with ops.KernelTimer("fc_box_log_prob") as timer:
        got = prior.log_prob(t["lv_x"].to(device)).cpu()
    assert len(timer.pairs) == 1
    outside = torch.isinf(got)
    assert got.shape == (64,) and torch.equal(outside, torch.isinf(t["lv_logp64"]))
    U.check("lotka-volterra", got[~outside], t["lv_logp64"][~outside], t["lv_floor"])
    torch.manual_seed(4)
    draws = prior.sample((50,))
    assert draws.is_cuda and draws.shape == (50, 4) and bool(((draws >= -5) & (draws < 2)).all())


# ---- every layout branch at its smallest shape ----------------------------------------------------------------------
def _misaligned(t):
    """A contiguous copy of ``t`` that starts 4 bytes off a 16-byte boundary."""
    buffer = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    view = buffer[1:].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() % 16 == 4
    return view


# d = 64 aligned is the only 16-byte layout here; shifted by 4 bytes it must take the scalar one
@pytest.mark.parametrize("d,shift", [(1, False), (3, False), (64, False), (64, True), (65, False)],
                         ids=["d1", "d3", "d64", "d64-misaligned", "d65"])
@pytest.mark.parametrize("rows", [1, 3, 257])
def test_layouts(rows, d, shift, device):
    c = U.layout_inputs(d)
    place = (lambda v: _misaligned(v.to(device))) if shift else (lambda v: v.to(device))
    x, logits, g, noise, points = (place(c[k][:rows]) for k in ("x", "logits", "g", "noise", "points"))
    low, high = place(c["low"]), place(c["high"])

    xg, lg = x.requires_grad_(True), logits.requires_grad_(True)
    with ops.KernelTimer("fc_bernoulli_log_prob") as forward, ops.KernelTimer("fc_bernoulli_log_prob_backward") as backward:
        logp = ops.bernoulli_log_prob(xg, lg)
        (logp * g).sum().backward()
    assert len(forward.pairs) == 1 and len(backward.pairs) == 1
    err = float((logp.detach().cpu().double() - c["logp64"][:rows]).abs().max())
    limit = 16 * U.EPS * float(c["magnitude"][:rows].max())
    print("log_prob err %.3g bound %.3g" % (err, limit))
    assert err <= limit
    g64, l64, x64 = c["g"][:rows].double()[:, None], c["logits"][:rows].double(), c["x"][:rows].double()
    err_l = (lg.grad.cpu().double() - g64 * (x64 - c["probs64"][:rows])).abs() - 8 * U.EPS * g64.abs()
    err_x = (xg.grad.cpu().double() - g64 * l64).abs() - U.EPS * (g64 * l64).abs()
    assert float(err_l.max()) <= 0 and float(err_x.max()) <= 0

    # (contexts, draws per context): one draw per row, and at 257 rows also 51 contexts x 5 draws
    for groups, draws in ([(rows, 1), (51, 5)] if rows == 257 else [(rows, 1)]):
        used = groups * draws
        with ops.KernelTimer("fc_bernoulli_sample") as sampler:
            samples = ops.bernoulli_sample(logits.detach()[:groups], noise[:used], draws)
        assert len(sampler.pairs) == 1
        probs = c["probs64"][:groups].repeat_interleave(draws, 0)
        decided = (c["noise"][:used].double() - probs).abs() >= 1e-6
        assert torch.equal(samples.cpu()[decided], (c["noise"][:used].double() < probs).float()[decided])

    with ops.KernelTimer("fc_box_log_prob") as box:
        inside = ops.box_log_prob(points, low, high).cpu()
    assert len(box.pairs) == 1
    assert torch.equal(torch.isinf(inside), c["outside"][:rows]) and not torch.isnan(inside).any()
    finite = inside[~c["outside"][:rows]].double()
    widths = torch.log(c["high"].double() - c["low"].double()).abs().sum()
    assert finite.numel() == 0 or float((finite + c["volume64"]).abs().max()) <= (d + 8) * U.EPS * float(widths)
