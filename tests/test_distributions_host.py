"""ConditionalIndependentBernoulli, BoxUniform, MG1Uniform and LotkaVolterraOscillating off the GPU: on CPU tensors the
classes take the torch composition, which must reproduce the reference's fixtures; the reference's exceptions, state_dict
keys, exports and the C ABI of the new entries."""
import copy
import ctypes
import os
import pickle
import re

import pytest
import torch
from torch import nn

import _distributions_util as U
from flowconductor_amd import _hip, distributions, ops
from flowconductor_amd.distributions.uniform import BoxUniform, LotkaVolterraOscillating, MG1Uniform

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["fc_bernoulli_log_prob", "fc_bernoulli_log_prob_backward", "fc_bernoulli_sample", "fc_box_log_prob"]


def test_exports_carry_the_reference_names():
    for name in ("Distribution", "NoMeanException", "ConditionalIndependentBernoulli", "MADEMoG", "ConditionalDiagonalNormal",
                 "DiagonalNormal", "StandardNormal", "LotkaVolterraOscillating", "MG1Uniform"):
        assert name in dir(distributions) and name in getattr(distributions, "__all__", dir(distributions)), name
    assert issubclass(distributions.ConditionalIndependentBernoulli, distributions.Distribution)
    assert issubclass(BoxUniform, torch.distributions.Independent)
    assert issubclass(MG1Uniform, torch.distributions.Uniform)
    for name in ("bernoulli_log_prob", "bernoulli_sample", "box_log_prob", "_BernoulliLogProbFunction"):
        assert hasattr(ops, name), name


@pytest.mark.parametrize("name", ENTRIES)
def test_entries_are_declared_bound_and_exported(name):
    assert name in _hip.SIGNATURES
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "flowcon_hip.h")).read(), flags=re.S)
    decl = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, header)
    assert decl is not None, "%s is not declared in include/flowcon_hip.h" % name
    assert len(decl.group(1).split(",")) == len(_hip.SIGNATURES[name])
    assert hasattr(ctypes.CDLL(_hip.LIB_PATH), name), "libflowcon_hip.so does not export %s" % name


@pytest.mark.parametrize("name", sorted(U.BERNOULLI))
def test_bernoulli_reproduces_the_fixture_on_the_cpu(name):
    t = U.fixture("bernoulli_" + name)
    dist = U.build_bernoulli(name)
    assert os.path.getsize(os.path.join(U.GOLDEN, "bernoulli_%s.npz" % name)) <= 1 << 20
    assert t["x"].shape[1:] == tuple(U.BERNOULLI[name]) and t["x"].shape[0] == (33 if name == "d784" else 257)
    zero_one = bool(((t["x"] == 0) | (t["x"] == 1)).all())
    assert zero_one == (name != U.FRACTIONAL) and float(t["x"].min()) >= 0 and float(t["x"].max()) <= 1
    with torch.no_grad():
        logp = dist.log_prob(t["x"], context=t["context"])
        mean = dist.mean(t["context"])
    assert logp.dtype == torch.float32 and mean.shape == t["x"].shape
    U.check(name + " log_prob", logp, t["logp64"], t["floor_logp"])
    U.check(name + " log_prob vs float32", logp, t["logp32"].double(), t["floor_logp"])
    U.check(name + " mean", mean, t["mean64"], t["floor_mean"])
    # a float64 copy on the same inputs is the float64 fixture itself
    logp64 = copy.deepcopy(dist).double().log_prob(t["x"].double(), context=t["context"].double())
    assert logp64.dtype == torch.float64 and float((logp64.detach() - t["logp64"]).abs().max()) <= 1e-9 * float(t["logp64"].abs().max())


@pytest.mark.parametrize("name", U.WITH_GRADIENTS)
def test_bernoulli_gradients_on_the_cpu(name):
    t = U.fixture("bernoulli_" + name)
    dist = U.build_bernoulli(name)
    context, taps = U.tap_logits(dist, t["context"].clone())
    x = t["x"].clone().requires_grad_(True)
    (dist.log_prob(x, context=context) * t["g"]).sum().backward()
    U.check(name + " grad logits", taps[0].grad.reshape(x.shape), t["grad_logits64"], t["floor_grad_logits"])
    U.check(name + " grad inputs", x.grad, t["grad_x64"], t["floor_grad_x"])
    for key, p in dist.named_parameters():
        key = key[len("_context_encoder."):]
        U.check("%s grad %s" % (name, key), p.grad, t["grad64::" + key], t["floor_grad::" + key])


@pytest.mark.parametrize("name", U.SAMPLES)
def test_bernoulli_sample_reproduces_the_fixture_on_the_cpu(name):
    t = U.fixture("bernoulli_sample_" + name)
    contexts, draws = t["samples32"].shape[:2]
    shape = tuple(t["logits"].shape[1:])
    assert int(t["num_samples"]) == draws and torch.equal(t["samples32"], t["samples64"])
    assert float((t["noise"].double() - torch.sigmoid(t["logits"].double()).repeat_interleave(draws, 0)).abs().min()) >= 1e-6
    got = ops.bernoulli_sample(t["logits"], t["noise"], draws)
    assert got.dtype == torch.float32 and torch.equal(got.reshape(t["samples32"].shape), t["samples32"])
    # the class draws the reference's noise under the reference's seed (both on the CPU here)
    dist = distributions.ConditionalIndependentBernoulli(shape)
    torch.manual_seed(int(t["seed"]))
    drawn = dist.sample(draws, context=t["logits"])
    assert drawn.shape == (contexts, draws) + shape and torch.equal(drawn, t["samples32"])


@pytest.mark.parametrize("d", U.BOX)
def test_box_uniform_reproduces_the_fixture_on_the_cpu(d):
    t = U.fixture("box_d%d" % d)
    box = BoxUniform(t["low"], t["high"], validate_args=False)
    assert isinstance(box, torch.distributions.Independent) and box.event_shape == (d,) and box.batch_shape == ()
    for got in (box.log_prob(t["x"]), ops.box_log_prob(t["x"], t["low"], t["high"])):
        outside = torch.isinf(got)
        assert torch.equal(outside, torch.isinf(t["logp64"])) and bool((got[outside] < 0).all()) and not torch.isnan(got).any()
        assert not outside[0] and outside[1] and outside[int(t["nan_row"])]
        U.check("box_d%d" % d, got[~outside], t["logp64"][~outside], t["floor_logp"])
    # default validation: torch's own, exactly as the parent runs it
    checked = BoxUniform(t["low"], t["high"])
    if bool(t["default_validation_raises"]):
        with pytest.raises(ValueError, match="to be within the support"):
            checked.log_prob(t["x"])
    else:
        assert torch.equal(torch.isinf(checked.log_prob(t["x"])), outside)
    inside = t["x"][~outside]
    U.check("box_d%d validated" % d, checked.log_prob(inside), t["logp64"][~outside], t["floor_logp"])
    # the rest of Independent keeps working
    assert checked.sample((5,)).shape == (5, d) and checked.rsample((2, 3)).shape == (2, 3, d)
    assert bool(checked.support.check(inside).all()) and checked.mean.shape == (d,)
    assert float((checked.entropy() + t["logp64"][0]).abs()) <= U.bound(t["logp64"][0], t["floor_logp"])


def test_box_uniform_other_forms_fall_through_to_independent():
    scalar = BoxUniform(0.0, 2.0, reinterpreted_batch_ndims=0)
    assert float(scalar.log_prob(torch.tensor(1.0))) == pytest.approx(-0.6931471805599453)
    nested = BoxUniform(torch.zeros(2, 3), 2 * torch.ones(2, 3), reinterpreted_batch_ndims=2)
    assert nested.log_prob(torch.ones(5, 2, 3)).shape == (5,)
    batched = BoxUniform(torch.zeros(2, 3), 2 * torch.ones(2, 3))
    assert batched.log_prob(torch.ones(5, 2, 3)).shape == (5, 2)
    with pytest.raises(ValueError):
        ops.box_log_prob(torch.zeros(4, 3), torch.zeros(2), torch.ones(2))


def test_sbi_priors_reproduce_the_fixture_on_the_cpu():
    t = U.fixture("sbi_priors")
    mg1 = MG1Uniform(t["mg1_low"], t["mg1_high"], validate_args=False)
    got = mg1.log_prob(t["mg1_x"])
    assert got.shape == (64, 3)                     # element-wise, not summed
    outside = torch.isinf(got)
    assert torch.equal(outside, torch.isinf(t["mg1_logp64"])) and 0 < int(outside.sum()) < outside.numel()
    U.check("mg1", got[~outside], t["mg1_logp64"][~outside], t["mg1_floor"])
    draws = mg1.sample((200,))
    assert draws.shape == (200, 3) and bool((~torch.isinf(mg1.log_prob(draws))).all())
    # the matrices follow the value's dtype (the reference raises a dtype mismatch here)
    assert torch.equal(torch.isinf(mg1.log_prob(t["mg1_x"].double())), outside)

    prior = LotkaVolterraOscillating()
    got = prior.log_prob(t["lv_x"])
    outside = torch.isinf(got)
    assert got.shape == (64,) and torch.equal(outside, torch.isinf(t["lv_logp64"])) and 0 < int(outside.sum()) < 64
    U.check("lotka-volterra", got[~outside], t["lv_logp64"][~outside], t["lv_floor"])


def test_lotka_volterra_samples_lie_in_the_box():
    torch.manual_seed(3)
    prior = LotkaVolterraOscillating()
    draws = prior.sample((50,))
    assert draws.shape == (50, 4) and draws.dtype == torch.float32
    assert bool(((draws >= -5) & (draws < 2)).all()) and bool(torch.isfinite(prior.log_prob(draws)).all())
    assert LotkaVolterraOscillating(device="cpu").sample((3,)).device.type == "cpu"


def test_reference_exceptions_and_messages():
    dist = distributions.ConditionalIndependentBernoulli([3], nn.Linear(4, 3))
    x, context = torch.zeros(5, 3), torch.zeros(5, 4)
    with pytest.raises(ValueError, match="Context can't be None."):
        dist.log_prob(x)
    with pytest.raises(ValueError, match="Context can't be None."):
        dist.sample(2)
    with pytest.raises(ValueError, match="Context can't be None."):
        dist.mean()
    with pytest.raises(ValueError, match=re.escape("Expected input of shape torch.Size([3]), got torch.Size([4])")):
        dist.log_prob(torch.zeros(5, 4), context=context)
    with pytest.raises(ValueError, match="Number of input items must be equal to number of context items."):
        dist.log_prob(x, context=context[:4])
    halving = distributions.ConditionalIndependentBernoulli([3], lambda c: c[::2, :3])
    with pytest.raises(RuntimeError, match="The batch dimension of the parameters is inconsistent with the input."):
        halving.log_prob(torch.zeros(4, 3), context=torch.zeros(4, 4))
    with pytest.raises(RuntimeError, match="Forward method cannot be called"):
        dist(x)
    with pytest.raises(ValueError):
        ops.bernoulli_log_prob(torch.zeros(2, 3), torch.zeros(2, 4))
    with pytest.raises(ValueError):
        ops.bernoulli_log_prob(torch.zeros(2, 3), torch.zeros(2, 3), add=torch.zeros(3))
    with pytest.raises(ValueError):
        ops.bernoulli_sample(torch.zeros(2, 3), torch.zeros(5, 3), 2)


def test_state_dict_keys_follow_the_encoder():
    encoder = nn.Sequential(nn.Linear(4, 8), nn.ReLU(), nn.Linear(8, 6))
    dist = distributions.ConditionalIndependentBernoulli([2, 3], encoder)
    assert list(dist.state_dict()) == ["_context_encoder." + key for key in encoder.state_dict()]
    assert list(U.build_bernoulli("d3").state_dict()) == ["_context_encoder.weight", "_context_encoder.bias"]
    assert list(distributions.ConditionalIndependentBernoulli([3]).state_dict()) == []
    assert list(distributions.ConditionalIndependentBernoulli([3], lambda c: c).state_dict()) == []


def test_sample_shapes():
    torch.manual_seed(0)
    dist = distributions.ConditionalIndependentBernoulli([2, 3], nn.Linear(4, 6))
    context = torch.randn(5, 4)
    draws = dist.sample(7, context=context)
    assert draws.shape == (5, 7, 2, 3) and draws.dtype == torch.float32 and bool(((draws == 0) | (draws == 1)).all())
    # the base class draws in pieces of batch_size and joins them along the leading dimension, as the reference does
    assert dist.sample(6, context=context, batch_size=3).shape == (10, 3, 2, 3)
    assert dist.sample(3, context=context, batch_size=5).shape == (5, 3, 2, 3)
    both, logp = dist.sample_and_log_prob(4, context=context)
    assert both.shape == (5, 4, 2, 3) and logp.shape == (5, 4) and bool((logp <= 0).all())
    assert dist.mean(context).shape == (5, 2, 3)


def test_copies_and_pickles_after_use():
    dist = U.build_bernoulli("d3")
    t = U.fixture("bernoulli_d3")
    with torch.no_grad():
        before = dist.log_prob(t["x"], context=t["context"])
        dist.sample(2, context=t["context"])
    plain = distributions.ConditionalIndependentBernoulli([3])
    plain.log_prob(torch.zeros(2, 3), context=torch.zeros(2, 3))
    for clone in (copy.deepcopy(dist), pickle.loads(pickle.dumps(dist))):
        assert list(clone.state_dict()) == list(dist.state_dict())
        with torch.no_grad():
            assert torch.equal(clone.log_prob(t["x"], context=t["context"]), before)
    for clone in (copy.deepcopy(plain), pickle.loads(pickle.dumps(plain))):
        assert float(clone.log_prob(torch.zeros(1, 3), context=torch.zeros(1, 3))) == pytest.approx(-3 * 0.6931471805599453)
    box = pickle.loads(pickle.dumps(BoxUniform(torch.zeros(3), torch.ones(3))))
    assert float(box.log_prob(torch.full((3,), 0.5))) == 0.0


def test_double_backward_goes_through_the_composition():
    t = U.fixture("bernoulli_d3")
    x = t["x"].double()
    logits = (t["grad_logits64"] * 0 + torch.linspace(-2, 2, x.numel()).reshape(x.shape)).double().requires_grad_(True)
    logp = ops.bernoulli_log_prob(x, logits)
    (grad,) = torch.autograd.grad(logp.sum(), logits, create_graph=True)
    (second,) = torch.autograd.grad(grad.sum(), logits)
    p = torch.sigmoid(logits.detach())
    assert float((second + p * (1 - p)).abs().max()) <= 1e-12
