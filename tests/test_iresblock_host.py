"""Invertible residual blocks over Lipschitz DenseNets: host side (no GPU).

The torch composition of ``transforms.iResBlock`` is pinned to fixtures recorded from the reference
(tests/golden/make_iresblock_golden.py).  Tolerances:

* eval-mode forward / inverse / logabsdet against the reference's float32 results: both sides are torch float32 on a
  CPU; where the port orders an operation differently the two are two float32 realisations of the same float64 value,
  so the bound is the fixture's own noise floor ``max|ref32 - ref64|`` times the factor 4 that tests/test_gpu_golden.py
  uses (the floor is one realisation of a heavy-tailed error).  The inverse is compared the same way with the floor of
  the inverse outputs.
* training-mode results under fixed seeds: the port runs the reference's op sequence with the same random draws, so
  results and gradients differ by float32 rounding of re-ordered sums only; the bound is 64 eps32 relative to the largest
  magnitude of the compared tensor (a sum over at most a few hundred terms of that magnitude).
"""
import copy
import ctypes
import io
import os
import pickle
import re

import numpy as np
import pytest
import torch

import flowconductor_amd  # noqa: F401
from flowconductor_amd import _hip, distributions, flows, ops, transforms
from flowconductor_amd.nn import nets
from flowconductor_amd.nn.nets import activations, invertible_densenet
from flowconductor_amd.transforms import lipschitz
from flowconductor_amd.transforms.lipschitz import util as lip_util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
EPS32 = float(np.finfo(np.float32).eps)
CONTEXT = 3
SMALL = dict(c_embed_hidden_sizes=(16, 16, 6))

BLOCKS = {
    "toy": (lambda: nets.DenseNet(dimension=2, densenet_depth=3, densenet_growth=16,
                                  activation_function=activations.CSin(10)), False),
    "default8": (lambda: nets.DenseNet(dimension=8), False),
    "wide16": (lambda: nets.DenseNet(dimension=16, densenet_depth=4, densenet_growth=28), False),
    "lipswish": (lambda: nets.DenseNet(dimension=4, activation_function=activations.LipSwish()), False),
    "tanh": (lambda: nets.DenseNet(dimension=5, densenet_growth=12, activation_function="tanh"), False),
    "elu": (lambda: nets.DenseNet(dimension=5, densenet_growth=12, activation_function="elu"), False),
    "relu": (lambda: nets.DenseNet(dimension=5, densenet_growth=12, activation_function="relu"), False),
    "d1": (lambda: nets.DenseNet(dimension=1), False),
    "input_conditional": (lambda: nets.InputConditionalDenseNet(
        dimension=4, context_features=CONTEXT, densenet_depth=2, activation_function=activations.Swish(), **SMALL),
        True),
    "multiplicative_input": (lambda: nets.MultiplicativeAndInputConditionalDenseNet(
        dimension=4, context_features=CONTEXT, densenet_depth=2, activation_function="CLipSwish",
        m_embed_hidden_sizes=(16, 16), **SMALL), True),
    "last_layer": (lambda: nets.LastLayerConditionalDenseNet(
        dimension=3, context_features=CONTEXT, densenet_depth=2, activation_function="CLipSwish"), True),
}


def fixture(name):
    return np.load(os.path.join(GOLDEN, "iresblock_%s.npz" % name))


def state_dict_of(g):
    return {k[4:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("sd::")}


def load_block(name, **kwargs):
    g = fixture(name)
    block = transforms.iResBlock(BLOCKS[name][0](), brute_force=True, **kwargs)
    sd = state_dict_of(g)
    assert set(sd) == set(block.state_dict()), set(sd) ^ set(block.state_dict())
    block.load_state_dict(sd, strict=True)
    return block.eval(), g


def build_toy_flow():
    factory = (transforms.iResBlock.Factory().set_logabsdet_estimator(brute_force=True)
               .set_densenet(dimension=2, densenet_depth=3, densenet_growth=16,
                             activation_function=activations.CSin(10)))
    layers = []
    for _ in range(10):
        layers += [transforms.ActNorm(features=2), factory.build()]
    return flows.Flow(transforms.CompositeTransform(layers), distributions.StandardNormal(shape=[2]))


def worst(a, b):
    return float(np.max(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)))) if np.size(a) else 0.0


def test_exports():
    assert transforms.iResBlock is lipschitz.iResBlock
    for name in ("DenseNet", "InputConditionalDenseNet", "MultiplicativeConditionalDenseNet",
                 "MultiplicativeAndInputConditionalDenseNet", "LastLayerConditionalDenseNet",
                 "MixedConditionalDenseNet"):
        assert getattr(nets, name) is getattr(invertible_densenet, name)
    assert nets.activations is activations
    for name in ("Swish", "LipSwish", "CLipSwish", "LeakyLSwish", "Sin", "CSin", "LipschitzCube", "FullSort", "MaxMin"):
        assert issubclass(getattr(activations, name), torch.nn.Module)
    assert activations.CLipSwish()._does_concat and activations.CSin()._does_concat
    assert not hasattr(activations.LipSwish(), "_does_concat")
    assert set(invertible_densenet.ACTIVATION_FNS) == {"relu", "tanh", "elu", "selu", "fullsort", "maxmin", "swish",
                                                       "LeakyLSwish", "CLipSwish", "lcube", "csin"}
    for name in ("DeterminantEstimator", "BruteForceDeterminantEstimator", "ApproxTraceDeterminantEstimator"):
        assert hasattr(lipschitz, name)
    for name in ("UnbiasedParameterGenerator", "BiasedParameterGenerator", "GeometricSampler", "find_fixed_point",
                 "find_fixed_point_noaccel"):
        assert callable(getattr(lip_util, name))


def test_constructor_assertions():
    with pytest.raises(AssertionError, match="n_lipschitz_iters must be > 0"):
        nets.DenseNet(dimension=2, n_lipschitz_iters=0)
    with pytest.raises(AssertionError, match="lip_coeff must be > 0"):
        nets.DenseNet(dimension=2, lip_coeff=0.0)
    with pytest.raises(AssertionError, match="Activation function nope not found."):
        nets.DenseNet(dimension=2, activation_function="nope")
    with pytest.raises(AssertionError, match="Select an even densenet growth size for CLipSwish!"):
        nets.DenseNet(dimension=2, densenet_growth=7)
    with pytest.raises(AssertionError, match="Context not supported for this Class."):
        nets.DenseNet(dimension=2)(torch.zeros(1, 2), torch.zeros(1, 1))
    with pytest.raises(NotImplementedError, match="Unknown estimator 'x'. Has to be 'neumann' or 'basic'."):
        transforms.iResBlock(nets.DenseNet(dimension=2), trace_estimator="x")
    with pytest.raises(AssertionError, match="iResBlock arguments not set"):
        transforms.iResBlock.Factory().set_densenet(dimension=2).build()
    with pytest.raises(AssertionError, match="DenseNet arguments not set"):
        transforms.iResBlock.Factory().set_logabsdet_estimator().build()


def test_factory_dispatch():
    conditional = dict(dimension=2, context_features=3, densenet_depth=1, activation_function="CLipSwish")
    table = {
        (False, False, False): nets.DenseNet,
        (True, False, False): nets.InputConditionalDenseNet,
        (False, True, False): nets.LastLayerConditionalDenseNet,
        (False, False, True): nets.LastLayerConditionalDenseNet,
        (True, True, False): nets.MixedConditionalDenseNet,
        (True, False, True): nets.MultiplicativeAndInputConditionalDenseNet,
    }
    for (ci, cl, cm), cls in table.items():
        kwargs = dict(dimension=2) if cls is nets.DenseNet else conditional
        net = nets.DenseNet.factory(condition_input=ci, condition_lastlayer=cl, condition_multiplicative=cm, **kwargs)()
        assert type(net) is cls
    for key in ((False, True, True), (True, True, True)):
        with pytest.raises(NotImplementedError, match="This combination of conditions"):
            nets.DenseNet.factory(condition_input=key[0], condition_lastlayer=key[1], condition_multiplicative=key[2])


def test_shared_activation_and_keys():
    net = nets.DenseNet(dimension=3)
    assert net.dense_net[0].network[1] is net.activation and net.dense_net[1].network[1] is net.activation
    keys = set(transforms.iResBlock(net).state_dict())
    for key in ("nnet.dense_net.0.network.0.parametrizations.weight.original",
                "nnet.dense_net.0.network.0.parametrizations.weight.0._u",
                "nnet.dense_net.0.network.0.parametrizations.weight.0._v", "nnet.dense_net.0.K1_unnormalized",
                "nnet.activation.swish.beta"):
        assert key in keys


def test_repr_works():
    text = repr(transforms.iResBlock(nets.DenseNet(dimension=2), trace_estimator="basic"))
    assert "brute_force=False" in text and "unbiased_estimator=True" in text and "basic_logdet_estimator" in text


@pytest.mark.parametrize("name", sorted(BLOCKS))
def test_composition_reproduces_reference(name):
    block, g = load_block(name)
    context = torch.from_numpy(g["context"]) if BLOCKS[name][1] else None
    with torch.no_grad():
        y, lad = block(torch.from_numpy(g["x"]), context)
        x, ilad = block.inverse(torch.from_numpy(g["inv_in"]), context)
    for got, ref32, ref64 in ((y, "y32", "y64"), (lad, "lad32", "lad64"), (x, "inv_x32", "inv_x64"),
                              (ilad, "inv_lad32", "inv_lad64")):
        floor = worst(g[ref32], g[ref64])
        err = worst(got.numpy(), g[ref32])
        print("%s %s: |port - ref32| %.3g, floor %.3g" % (name, ref32, err, floor))
        assert err <= 4 * floor, (name, ref32, err, floor)
    assert not y.requires_grad and not lad.requires_grad


def test_float64_composition_matches_reference64():
    block, g = load_block("default8")
    block = block.double()
    with torch.no_grad():
        y, lad = block(torch.from_numpy(g["x"]).double())
    assert worst(y.numpy(), g["y64"]) < 1e-12 and worst(lad.numpy(), g["lad64"]) < 1e-12


def _toy_flow_on_cpu(flow, rows, inverse):
    """The cascade of the toy flow with ActNorm written out in torch (this package's ActNorm is a kernel; the blocks
    are what is under test): y = exp(log_scale) x + shift, logabsdet = sum(log_scale)."""
    total = torch.zeros(rows.shape[0])
    layers = list(flow._transform._transforms)
    for layer in (reversed(layers) if inverse else layers):
        if isinstance(layer, transforms.ActNorm):
            scale, shift = torch.exp(layer.log_scale), layer.shift
            rows = (rows - shift) / scale if inverse else scale * rows + shift
            lad = torch.sum(layer.log_scale).expand(rows.shape[0])
            lad = -lad if inverse else lad
        else:
            rows, lad = layer.inverse(rows) if inverse else layer(rows)
        total = total + lad
    return rows, total


def test_toy_flow_reproduces_reference():
    g = fixture("toy_flow")
    flow = build_toy_flow()
    sd = state_dict_of(g)
    assert set(sd) == set(flow.state_dict())
    flow.load_state_dict(sd, strict=True)
    flow.eval()
    with torch.no_grad():
        z, lad_f = _toy_flow_on_cpu(flow, torch.from_numpy(g["x"]), inverse=False)
        lp = -0.5 * (z ** 2).sum(1) - float(np.log(2 * np.pi)) + lad_f      # StandardNormal([2]) written out
        s, lad = _toy_flow_on_cpu(flow, torch.from_numpy(g["noise"]), inverse=True)
    for got, ref32, ref64 in ((lp, "log_prob32", "log_prob64"), (s, "sample32", "sample64"),
                              (lad, "sample_lad32", "sample_lad64")):
        floor, err = worst(g[ref32], g[ref64]), worst(got.numpy(), g[ref32])
        print("toy_flow %s: |port - ref32| %.3g, floor %.3g" % (ref32, err, floor))
        assert err <= 4 * floor, (ref32, err, floor)


TRAIN_MODES = {
    "unbiased_neumann": dict(brute_force=False, unbiased_estimator=True, trace_estimator="neumann"),
    "biased_basic": dict(brute_force=False, unbiased_estimator=False, trace_estimator="basic"),
    "brute_force": dict(brute_force=True),
}


@pytest.mark.parametrize("mode", sorted(TRAIN_MODES))
def test_training_mode_reproduces_reference(mode):
    g = fixture("train")
    block = transforms.iResBlock(nets.DenseNet(dimension=3), **TRAIN_MODES[mode])
    block.load_state_dict(state_dict_of(g), strict=True)
    block.train()
    torch.manual_seed(7)
    np.random.seed(7)
    x = torch.from_numpy(g["x"])
    y, lad = block(x)
    assert not x.requires_grad            # the caller's tensor is left alone
    lad.sum().backward()

    def close(got, ref, what):
        bound = 64 * EPS32 * max(1.0, float(np.max(np.abs(ref))))
        err = worst(got, ref)
        print("%s %s: %.3g (bound %.3g)" % (mode, what, err, bound))
        assert err <= bound, (mode, what, err, bound)

    close(y.detach().numpy(), g[mode + "::y"], "y")
    close(lad.detach().numpy(), g[mode + "::lad"], "lad")
    grads = {k[len(mode) + 8:]: g[k] for k in g.files if k.startswith(mode + "::grad::")}
    assert grads
    seen = 0
    for name, p in block.named_parameters():
        if p.grad is None:
            assert name not in grads, name
            continue
        assert name in grads, name
        close(p.grad.numpy(), grads[name], "grad " + name)
        seen += 1
    assert seen == len(grads)


def test_power_iterations_only_in_training():
    block, g = load_block("default8")
    x = torch.from_numpy(g["x"])
    par = block.nnet.dense_net[0].network[0].parametrizations.weight[0]
    with torch.no_grad():
        par._u.copy_(torch.nn.functional.normalize(torch.randn_like(par._u), dim=0))     # off the fixed point
    before = par._u.clone()
    with torch.no_grad():
        block(x)
        block(x)
    assert torch.equal(par._u, before)
    block.train()
    block(x)
    assert not torch.equal(par._u, before)
    # eval-mode soft normalisation: W / max(1, sigma / coeff) from the stored vectors
    block.eval()
    lin = block.nnet.dense_net[0].network[0]
    with torch.no_grad():
        original = lin.parametrizations.weight.original
        sigma = torch.dot(par._u, original @ par._v)
        expected = original / torch.clamp(sigma / block.nnet.lip_coeff, min=1.0)
        assert torch.allclose(lin.weight, expected, rtol=1e-6, atol=0)


def test_copies_and_checkpoints():
    """``copy.deepcopy`` after a call gives an independent block; checkpoints go through ``state_dict`` -- torch refuses
    to pickle modules that carry ``torch.nn.utils.parametrize`` parametrisations (the reference's blocks likewise), and
    that refusal must be torch's own message, not a failure on one of this package's caches."""
    block, g = load_block("toy")
    x = torch.from_numpy(g["x"])
    with torch.no_grad():
        y, lad = block(x)
        block.inverse(x)
    clone = copy.deepcopy(block)
    with torch.no_grad():
        y2, lad2 = clone(x)
    assert torch.equal(y, y2) and torch.equal(lad, lad2)
    assert clone.nnet is clone.test_time_determinant_estimator.nnet is clone.train_determinant_estimator.nnet
    with torch.no_grad():
        clone.nnet.dense_net[-1].bias.add_(1.0)
        y_same, _ = block(x)
    assert torch.equal(y, y_same)
    buffer = io.BytesIO()
    torch.save(block.state_dict(), buffer)
    buffer.seek(0)
    fresh = transforms.iResBlock(BLOCKS["toy"][0](), brute_force=True).eval()
    fresh.load_state_dict(torch.load(buffer), strict=True)
    with torch.no_grad():
        y3, lad3 = fresh(x)
    assert torch.equal(y, y3) and torch.equal(lad, lad3)
    with pytest.raises(RuntimeError):        # torch.nn.utils.parametrize's refusal, whatever its wording
        pickle.dumps(block)


@pytest.mark.parametrize("solver", [lip_util.find_fixed_point, lip_util.find_fixed_point_noaccel])
def test_fixed_point_solvers(solver):
    """Known fixed points: a linear contraction x = A x + b (solution (I - A)^-1 b, |A|_2 = 0.9), per-sample
    x = cos(x) + c, and a map whose plain iteration diverges (slope -1.5) but whose relaxed one converges.  The solvers
    stop at a residual |f(x) - x| <= eps (1 + |x0|); a contraction of modulus L then puts x within residual / (1 - L) of
    the fixed point."""
    gen = torch.Generator().manual_seed(0)
    q, _ = torch.linalg.qr(torch.randn(6, 6, generator=gen, dtype=torch.float64))
    a = q @ torch.diag(torch.tensor([0.9, -0.8, 0.5, 0.3, -0.1, 0.0], dtype=torch.float64)) @ q.T
    b = torch.randn(5, 6, generator=gen, dtype=torch.float64)
    x0 = torch.randn(5, 6, generator=gen, dtype=torch.float64)
    eps = 1e-9
    x = solver(lambda v: v @ a.T + b, x0, eps=eps)
    exact = torch.linalg.solve(torch.eye(6, dtype=torch.float64) - a, b.T).T
    assert (x - exact).abs().max() <= eps * (1 + x0.abs().max()) / (1 - 0.9) * 6 ** 0.5
    shift = torch.linspace(-0.5, 0.5, 7, dtype=torch.float64).view(7, 1)
    x = solver(lambda v: torch.cos(v) + shift, torch.zeros(7, 1, dtype=torch.float64), eps=eps)
    assert (torch.cos(x) + shift - x).abs().max() <= eps
    assert x.shape == (7, 1) and not x.requires_grad
    x = solver(lambda v: 2.0 - 1.5 * v, torch.zeros(3, 2, dtype=torch.float64), eps=eps)
    assert (x - 0.8).abs().max() <= eps / 2.5 * 1.0001
    # images: any trailing shape
    x = solver(lambda v: 0.5 * torch.tanh(v) + 0.1, torch.zeros(2, 3, 4, 4), eps=1e-6)
    assert (0.5 * torch.tanh(x) + 0.1 - x).abs().max() <= 1e-6


@pytest.mark.parametrize("domain,codomain,order", [(1, 1, 1), (float("inf"), float("inf"), float("inf")), (2, 2, 2)])
def test_induced_norms(domain, codomain, order):
    """The generalised power method behind ``scaled_spectral_norm`` against ``torch.linalg.matrix_norm`` for the three
    induced norms that have a closed form (largest column sum, largest row sum, largest singular value), on a matrix
    with positive entries (where the iteration has one fixed point), and the soft normalisation built on it."""
    gen = torch.Generator().manual_seed(3)
    weight = torch.rand(5, 7, generator=gen, dtype=torch.float64) + 0.1
    expected = torch.linalg.matrix_norm(weight, ord=order)
    lin = torch.nn.Linear(7, 5).double()
    with torch.no_grad():
        lin.weight.copy_(weight)
    lin = nets.spectral_norm.scaled_spectral_norm(lin, domain=domain, codomain=codomain, coeff=0.5,
                                                  n_power_iterations=50)
    lin.train()
    normalised = lin.weight
    par = lin.parametrizations.weight[0]
    sigma = torch.dot(par._u, weight @ par._v)
    assert abs(sigma - expected) <= 1e-9 * expected
    assert abs(torch.linalg.matrix_norm(normalised.detach(), ord=order) - 0.5) <= 1e-6    # float32 factor, see forward
    # a weight whose norm is already below coeff is left alone
    small = nets.spectral_norm.scaled_spectral_norm(torch.nn.Linear(7, 5).double(), domain=domain, codomain=codomain,
                                                    coeff=1e3, n_power_iterations=5)
    assert torch.equal(small.weight, small.parametrizations.weight.original)


def test_dual_vectors_of_general_norms():
    """``dual_vector`` / ``maximiser`` for a norm order without a special case: Hoelder's inequality is attained."""
    from flowconductor_amd.nn.nets.spectral_norm import dual_vector, maximiser
    y = torch.tensor([0.3, -1.7, 0.0, 2.2, -0.4], dtype=torch.float64)
    for q in (1.5, 3.0, 1, 2, float("inf")):
        u = dual_vector(y, q)
        conjugate = float("inf") if q == 1 else (1.0 if q == float("inf") else q / (q - 1))
        assert abs(torch.linalg.vector_norm(u, ord=conjugate) - 1) < 1e-12
        assert abs(torch.dot(u, y) - torch.linalg.vector_norm(y, ord=q)) < 1e-12
        v = maximiser(y, q)
        assert abs(torch.linalg.vector_norm(v, ord=q) - 1) < 1e-12
        assert abs(torch.dot(v, y) - torch.linalg.vector_norm(y, ord=conjugate)) < 1e-12
    with pytest.raises(NotImplementedError):
        nets.spectral_norm.scaled_spectral_norm(torch.nn.Linear(2, 2), domain=torch.tensor(2.0), codomain=2)


def test_unbiased_coefficients():
    """The Russian-roulette weights: 1 for the exact terms, share of draws reaching term k over P(N >= k - exact)."""
    np.random.seed(5)
    generator = lip_util.UnbiasedParameterGenerator(n_exact_terms=2, n_samples=4)
    coeff, terms = generator.sample_parameters(training=True)
    np.random.seed(5)
    draws = np.random.geometric(0.5, 4)
    assert terms == draws.max() + 2
    assert coeff(1) == 1 and coeff(2) == 1 and coeff(3) == 1
    for k in range(4, terms + 2):
        assert coeff(k) == pytest.approx(np.mean(draws >= k - 2) / 0.5 ** (k - 3), rel=1e-15)
    np.random.seed(5)
    assert generator.sample_parameters(training=False)[1] == terms + 20
    assert lip_util.BiasedParameterGenerator(7).sample_parameters()[1] == 7


def test_kernel_plan_boundaries():
    """What goes to the kernels is decided on the host: the limits of include/flowcon_hip.h."""
    def plan(net):
        return transforms.iResBlock(net, brute_force=True)._kernel_plan()

    assert plan(nets.DenseNet(dimension=2, densenet_depth=3, densenet_growth=16,
                              activation_function=activations.CSin(10)))[0] == ops.IRES_ACT_CSIN
    assert plan(nets.DenseNet(dimension=8))[0] == ops.IRES_ACT_CLIPSWISH
    assert plan(nets.DenseNet(dimension=16, densenet_depth=4, densenet_growth=28)) is not None      # width 128
    assert plan(nets.DenseNet(dimension=16, densenet_depth=4, densenet_growth=30)) is None          # width 136
    assert plan(nets.DenseNet(dimension=17)) is None
    assert plan(nets.DenseNet(dimension=4, densenet_depth=5, densenet_growth=8)) is None
    assert plan(nets.DenseNet(dimension=4, activation_function="fullsort")) is None
    assert plan(nets.DenseNet(dimension=4, activation_function="maxmin")) is None
    assert plan(BLOCKS["last_layer"][0]()) is None
    assert plan(BLOCKS["input_conditional"][0]())[3:] == (6, False)
    assert plan(BLOCKS["multiplicative_input"][0]())[3:] == (6, True)
    assert ops.iresnet_image_floats(8, 0, 2, 16, ops.IRES_ACT_CLIPSWISH) == 4 + (4 + 8 + 64) + (4 + 8 + 192) + 8 + 320


def test_host_tensors_take_the_composition():
    block, g = load_block("default8")
    assert block._use_kernels(torch.from_numpy(g["x"]), None) is None
    with pytest.raises(RuntimeError, match="HIP device"), torch.no_grad():
        ops.iresnet_forward(torch.zeros(2, 8), torch.zeros(612), 8, 0, 2, 16, ops.IRES_ACT_CLIPSWISH)


def test_new_abi_entries():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "flowcon_hip.h")).read(), flags=re.S)
    lib = ctypes.CDLL(_hip.LIB_PATH)
    for name in ("fc_iresnet_forward", "fc_iresnet_inverse"):
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
        assert name in _hip.SIGNATURES
        assert hasattr(lib, name)
    for macro, value in (("FC_IRES_MAX_DIM", ops.IRES_MAX_DIM), ("FC_IRES_MAX_DEPTH", ops.IRES_MAX_DEPTH),
                         ("FC_IRES_MAX_WIDTH", ops.IRES_MAX_WIDTH), ("FC_IRES_ACT_CLIPSWISH", ops.IRES_ACT_CLIPSWISH),
                         ("FC_IRES_ACT_CSIN", ops.IRES_ACT_CSIN), ("FC_IRES_ACT_LEAKY_LSWISH", ops.IRES_ACT_LEAKY_LSWISH)):
        assert re.search(r"#define %s %d\b" % (macro, value), text), macro
    assert _hip.ABI_VERSION == 3
