"""UMNN layers off the GPU: the quadrature rule, the reference's API and state keys, the torch composition against the
reference's vectors (tests/golden/make_umnn_golden.py) in both precisions, its inverse and its gradients."""
import copy

import numpy as np
import pytest
import torch

import flowconductor_amd.transforms as T
from flowconductor_amd.transforms.UMNN import ELUPlus, IntegrandNet, MonotonicNormalizer, cc_weights

import _umnn_util as U


@pytest.mark.parametrize("n", [1, 2, 5, 8, 20, 50])
def test_cc_weights_are_the_interpolatory_rule(n):
    nodes, weights = cc_weights(n)
    assert nodes.dtype == np.float64 and weights.dtype == np.float64 and nodes.shape == weights.shape == (n + 1,)
    assert np.abs(nodes - np.cos(np.arange(n + 1) * np.pi / n)).max() <= 1e-15
    assert np.array_equal(weights, weights[::-1])
    assert abs(weights.sum() - 2.0) <= 1e-12
    for k in range(n + 1):
        exact = 0.0 if k % 2 else 2.0 / (k + 1)
        assert abs(float((weights * nodes ** k).sum()) - exact) <= 1e-12, k


def test_exports():
    for name in ("MaskedUMNNAutoregressiveTransform", "UMNNCouplingTransform", "ConditionalUMNNTransform"):
        assert hasattr(T, name)
    assert isinstance(ELUPlus()(torch.tensor([-1.0, 2.0])), torch.Tensor)


@pytest.mark.parametrize("name", U.FIXTURES)
def test_state_keys_load_strictly(name):
    assert len(U.FIXTURES) == 5
    module = U.build(name)
    want = set(U.state(U.fixture(name)))
    assert set(module.state_dict()) == want
    keys = [k for k in want if k.startswith("transformer.")]
    assert keys and all(k.startswith("transformer.integrand_net.net.") for k in keys)


def test_coupling_with_unconditional_transform_constructs():
    module = T.UMNNCouplingTransform([1, 0, 1, 0], lambda i, o: torch.nn.Linear(i, o), integrand_net_layers=[8],
                                     cond_size=3, apply_unconditional_transform=True)
    assert "unconditional_transform.integrand_net.net.0.weight" in module.state_dict()
    assert module.unconditional_transform.integrand_net.net[0].in_features == 1


@pytest.mark.parametrize("name", U.FIXTURES)
def test_composition_float64(name):
    z = U.fixture(name)
    module = U.build(name).double()
    ctx = U.tensor(z, "context", torch.float64)
    with torch.no_grad():
        y, lad = module(U.tensor(z, "x", torch.float64), ctx)
    assert U.maxdiff(y, z["y64"]) <= 1e-10 and U.maxdiff(lad, z["lad64"]) <= 1e-10


@pytest.mark.parametrize("name", U.FIXTURES)
def test_composition_float32(name):
    z = U.fixture(name)
    module = U.build(name)
    far = int(z["far_rows"])
    with torch.no_grad():
        y, lad = module(U.tensor(z, "x"), U.tensor(z, "context"))
    U.check_rows(name, y, z, "y64", "floor_y", far)
    U.check_rows(name, lad, z, "lad64", "floor_lad", far)


@pytest.mark.parametrize("name", U.FIXTURES)
def test_composition_inverse(name):
    z = U.fixture(name)
    module = U.build(name)
    far = int(z["far_rows"])
    ctx = U.tensor(z, "context")
    y = U.tensor(z, "y64", torch.float32)
    with torch.no_grad():
        x, lad = module.inverse(y, ctx)
        y2, lad2 = module(x, ctx)
        xsat, _ = module.inverse(U.tensor(z, "ysat", torch.float32), None if ctx is None else ctx[:2])
    U.check_rows(name, x, z, "xinv64", "floor_xinv", far)
    U.check_rows(name, lad, z, "ladinv64", "floor_ladinv", far)
    # round trip: the bisection's resolution 40 / 2^25 times the slope, inside twice the forward bound
    U.check_rows(name, y2, z, "y64", "floor_y", far, factor=2.0)
    assert U.maxdiff(lad + lad2, torch.zeros_like(lad)) <= 1e-6
    sat = torch.from_numpy(z["ysat"]).abs() > 1e3
    assert sat.any()
    assert float((xsat.double().abs()[sat] - 20.0).abs().max()) <= 2e-4
    assert torch.equal(torch.sign(xsat.double())[sat], torch.sign(torch.from_numpy(z["ysat"]))[sat])


def _restated(normalizer, x, h):
    """z with the limits detached: h_0 + (x / 2) sum_i w_i f((x / 2)(s_i + 1), h), written out per node."""
    nodes, weights = cc_weights(normalizer.nb_steps)
    xd = x.detach()
    hflat = h.permute(0, 2, 1).reshape(x.shape[0], -1)
    total = torch.zeros_like(xd)
    for s, w in zip(nodes, weights):
        total = total + float(w) * normalizer.integrand_net(xd / 2 * (float(s) + 1.0), hflat)
    return h[:, :, 0] + xd / 2 * total


def test_gradients_follow_leibniz():
    torch.manual_seed(3)
    norm = MonotonicNormalizer([12, 9], 4, nb_steps=8).double()
    x = torch.randn(6, 3, dtype=torch.float64, requires_grad=True)
    h = torch.randn(6, 3, 4, dtype=torch.float64, requires_grad=True)
    z, jac = norm(x, h)
    gx, = torch.autograd.grad(z.sum(), x, retain_graph=True)
    assert U.maxdiff(gx, jac) <= 1e-14
    gout = torch.randn(6, 3, dtype=torch.float64)
    params = list(norm.parameters())
    got = torch.autograd.grad((z * gout).sum(), [h] + params)
    twin = copy.deepcopy(norm)
    h2 = h.detach().clone().requires_grad_(True)
    want = torch.autograd.grad((_restated(twin, x, h2) * gout).sum(), [h2] + list(twin.parameters()))
    assert U.maxdiff(z, _restated(twin, x, h2)) <= 1e-13
    for a, b in zip(got, want):
        assert U.maxdiff(a, b) <= 1e-12 * max(1.0, float(b.abs().max()))


def test_cc_and_ccparallel_agree_and_user_modules_compose():
    torch.manual_seed(4)
    a = MonotonicNormalizer([8], 3, nb_steps=6, solver="CC")
    b = MonotonicNormalizer(copy.deepcopy(a.integrand_net), 3, nb_steps=6, solver="CCParallel")
    x, h = torch.randn(5, 2), torch.randn(5, 2, 3)
    za, ja = a(x, h)
    zb, jb = b(x, h)
    assert torch.equal(za, zb) and torch.equal(ja, jb)
    assert isinstance(a.integrand_net, IntegrandNet) and a.integrand_net.linears() is not None

    class Mine(torch.nn.Module):
        def forward(self, x, h):
            return torch.ones_like(x) * 2.0

    z, jac = MonotonicNormalizer(Mine(), 3, nb_steps=4)(x, h)           # f = 2: z = h_0 + 2 x
    assert U.maxdiff(z, h[:, :, 0] + 2.0 * x) <= 1e-6 and torch.equal(jac, torch.full_like(x, 2.0))


def test_coupling_takes_images():
    torch.manual_seed(5)
    from flowconductor_amd.nn import nets
    module = T.UMNNCouplingTransform([1, 0, 1, 0], lambda i, o: nets.ConvResidualNet(i, o, hidden_channels=8),
                                     integrand_net_layers=[8], cond_size=3, nb_steps=6).eval()
    x = torch.randn(2, 4, 3, 3)
    with torch.no_grad():
        y, lad = module(x)
        xr, lad_inv = module.inverse(y)
    assert y.shape == x.shape and lad.shape == (2,)
    assert torch.equal(y[:, module.identity_features], x[:, module.identity_features])
    assert U.maxdiff(xr, x) <= 1e-4 and U.maxdiff(lad + lad_inv, torch.zeros(2)) <= 1e-4
