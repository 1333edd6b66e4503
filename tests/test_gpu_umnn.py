"""UMNN layers on the GPU: ``fc_umnn`` against the reference's float64 vectors (tests/golden/make_umnn_golden.py) in
both directions, bit-exactness under a change of position, the fallbacks to the torch composition, flows and caches."""
import copy
import io
import math
import pickle

import pytest
import torch

import flowconductor_amd.transforms as T
from flowconductor_amd import distributions, flows, ops
from flowconductor_amd.nn import nets
from flowconductor_amd.transforms.UMNN import MonotonicNormalizer

import _umnn_util as U

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

_modules = {}


def module_of(name):
    if name not in _modules:
        _modules[name] = U.build(name).to(DEV)
    return _modules[name]


def on_dev(z, key, rows=None):
    t = U.tensor(z, key, torch.float32, DEV)
    return None if t is None else t[:rows]


@pytest.mark.parametrize("rows", [1, 63, 257])
@pytest.mark.parametrize("name", U.FIXTURES)
def test_forward(name, rows):
    z = U.fixture(name)
    module = module_of(name)
    far = int(z["far_rows"])
    with torch.no_grad(), ops.KernelTimer("fc_umnn") as timer:
        y, lad = module(on_dev(z, "x", rows), on_dev(z, "context", rows))
    assert len(timer.pairs) == 1
    U.check_rows(name, y, z, "y64", "floor_y", far, rows=rows)
    U.check_rows(name, lad, z, "lad64", "floor_lad", far, rows=rows)


@pytest.mark.parametrize("name", U.FIXTURES)
def test_inverse(name):
    z = U.fixture(name)
    module = module_of(name)
    far = int(z["far_rows"])
    ctx = on_dev(z, "context")
    features = z["x"].shape[1]
    launches = features if name.startswith("made_") else 1      # the autoregressive inverse: one pass per feature
    with torch.no_grad():
        with ops.KernelTimer("fc_umnn") as timer:
            x, lad = module.inverse(on_dev(z, "y64"), ctx)
        assert len(timer.pairs) == launches
        y2, lad2 = module(x, ctx)
        xsat, _ = module.inverse(on_dev(z, "ysat"), None if ctx is None else ctx[:2])
    U.check_rows(name, x, z, "xinv64", "floor_xinv", far)
    U.check_rows(name, lad, z, "ladinv64", "floor_ladinv", far)
    U.check_rows(name, y2, z, "y64", "floor_y", far, factor=2.0)
    cancel = U.maxdiff(lad + lad2, torch.zeros_like(lad))
    lim = 2.0 * U.bound(torch.from_numpy(z["lad64"]), max(float(z["floor_lad_far"]), float(z["floor_lad_body"])))
    print("%s lad + lad_inv: %.3e bound %.3e" % (name, cancel, lim))
    assert cancel <= lim
    sat = torch.from_numpy(z["ysat"]).abs() > 1e3
    off = float((xsat.cpu().double().abs()[sat] - 20.0).abs().max())
    print("%s saturated rows: %.3e from +-20" % (name, off))
    assert off <= 2e-4
    assert torch.equal(torch.sign(xsat.cpu().double())[sat], torch.sign(torch.from_numpy(z["ysat"]))[sat])


@pytest.mark.parametrize("inverse", [False, True])
def test_position_independent(inverse):
    z = U.fixture(U.DEFAULT)
    norm = module_of(U.DEFAULT).transformer
    torch.manual_seed(0)
    x = on_dev(z, "x")
    h = torch.randn(257, x.shape[1], norm.cond_size, device=DEV)
    idx = torch.arange(1000, device=DEV) % 257
    with torch.no_grad():
        if inverse:
            x = norm.apply_with_logabsdet(x, h)[0]
        base, base_lad = norm.apply_with_logabsdet(x, h, inverse=inverse)
        out, lad = norm.apply_with_logabsdet(x[idx].contiguous(), h[idx].contiguous(), inverse=inverse)
    assert torch.equal(out, base[idx]) and torch.equal(lad, base_lad[idx])


def _fallback_case(kind):
    torch.manual_seed(21)
    kw = dict(integrand_net_layers=[16, 16], cond_size=6, nb_steps=8)
    if kind == "cond_size":
        kw["cond_size"] = 40
    elif kind == "layers":
        kw["integrand_net_layers"] = [16, 16, 16, 16]
    elif kind == "width":
        kw["integrand_net_layers"] = [100]
    elif kind == "steps":
        kw["nb_steps"] = 80
    return T.MaskedUMNNAutoregressiveTransform(4, 16, **kw).eval()


@pytest.mark.parametrize("kind", ["cond_size", "layers", "width", "steps"])
def test_fallback_shapes_take_the_composition(kind):
    module = _fallback_case(kind)
    x = torch.randn(40, 4)
    with torch.no_grad():
        want_y, want_lad = copy.deepcopy(module).double()(x.double())
        with ops.KernelTimer("fc_umnn") as timer:
            y, lad = module.to(DEV)(x.to(DEV))
    assert len(timer.pairs) == 0
    assert U.maxdiff(y, want_y) <= U.bound(want_y, 2e-6) and U.maxdiff(lad, want_lad) <= U.bound(want_lad, 2e-6)


def test_fallback_image_input():
    torch.manual_seed(22)
    module = T.UMNNCouplingTransform([1, 0, 1, 0], lambda i, o: nets.ConvResidualNet(i, o, hidden_channels=8),
                                     integrand_net_layers=[8], cond_size=3, nb_steps=6).eval()
    x = torch.randn(2, 4, 3, 3)
    with torch.no_grad():
        want_y, want_lad = copy.deepcopy(module).double()(x.double())
        with ops.KernelTimer("fc_umnn") as timer:
            y, lad = module.to(DEV)(x.to(DEV))
    assert len(timer.pairs) == 0
    assert U.maxdiff(y, want_y) <= 1e-4 and U.maxdiff(lad, want_lad) <= 1e-4


def test_training_takes_the_composition_and_inference_the_kernel():
    z = U.fixture(U.DEFAULT)
    module = copy.deepcopy(module_of(U.DEFAULT))
    x = on_dev(z, "x", 63)
    with ops.KernelTimer("fc_umnn") as timer:
        y, lad = module(x)
        (y.sum() + lad.sum()).backward()
    assert len(timer.pairs) == 0
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in module.transformer.parameters())
    U.check_rows("training", y, z, "y64", "floor_y", int(z["far_rows"]), rows=63)
    with torch.no_grad(), ops.KernelTimer("fc_umnn") as timer:
        y2, _ = module(x)
    assert len(timer.pairs) == 1
    U.check_rows("no_grad", y2, z, "y64", "floor_y", int(z["far_rows"]), rows=63)


def test_user_integrand_takes_the_composition():
    class Mine(torch.nn.Module):
        def forward(self, x, h):
            return torch.ones_like(x) * 2.0

    norm = MonotonicNormalizer(Mine(), 3, nb_steps=4)
    x, h = torch.randn(5, 2, device=DEV), torch.randn(5, 2, 3, device=DEV)
    with torch.no_grad(), ops.KernelTimer("fc_umnn") as timer:
        zed, lad = norm.apply_with_logabsdet(x, h)
    assert len(timer.pairs) == 0 and U.maxdiff(zed, h[:, :, 0] + 2.0 * x) <= 1e-5


def _flow():
    torch.manual_seed(31)
    layers = []
    for _ in range(2):
        layers += [T.MaskedUMNNAutoregressiveTransform(4, 16, integrand_net_layers=[24, 24], cond_size=8, nb_steps=10),
                   T.RandomPermutation(4)]
    flow = flows.Flow(T.CompositeTransform(layers), distributions.StandardNormal([4])).eval()
    with torch.no_grad():
        for p in flow.parameters():
            p.mul_(1.5)
    return flow


def _log_prob_float64(flow, x):
    """log_prob of ``_flow`` in float64 on the CPU: the UMNN layers' torch composition, the permutations as an index (the
    package's permutation and base-density kernels run on the device in float32 only), the standard normal written out."""
    twin = copy.deepcopy(flow).double()
    z, total = x.double(), torch.zeros(x.shape[0], dtype=torch.float64)
    for layer in twin._transform._transforms:
        if isinstance(layer, T.Permutation):
            z = z[:, layer._permutation]
        else:
            z, lad = layer(z)
            total = total + lad
    return total - 0.5 * (z * z).sum(1) - 0.5 * z.shape[1] * math.log(2.0 * math.pi)


def test_flow_and_caches():
    flow = _flow()
    x = torch.randn(130, 4)
    with torch.no_grad():
        want = _log_prob_float64(flow, x)
        dev = flow.to(DEV)
        with ops.KernelTimer("fc_umnn") as timer:
            got = dev.log_prob(x.to(DEV))
        assert len(timer.pairs) == 2
        err = U.maxdiff(got, want)
        print("flow log_prob err %.3e" % err)
        assert err <= U.bound(want, 2e-6)
        torch.manual_seed(1)
        samples, lp = dev.sample_and_log_prob(130)
        again = dev.log_prob(samples)
        err = U.maxdiff(lp, again)
        print("sample_and_log_prob vs log_prob(samples) %.3e" % err)
        assert err <= 2.0 * U.bound(again, 2e-6)
        layer = dev._transform._transforms[0]
        assert ops.cached(layer.transformer, "umnn_image") is not None
        clone = copy.deepcopy(dev)
        buf = io.BytesIO()
        pickle.dump(dev, buf)
        loaded = pickle.loads(buf.getvalue())
        for twin in (clone, loaded):
            assert ops.cached(twin._transform._transforms[0].transformer, "umnn_image") is None
            assert torch.equal(twin.log_prob(x.to(DEV)), got)
