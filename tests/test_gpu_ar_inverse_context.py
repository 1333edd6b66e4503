"""fc_made_inverse_context: the D passes of a CONDITIONAL masked-autoregressive inverse inside one kernel, against the
reference's D full passes (autoregressive.py:44-53 with made.py's additive context) restated by the oracle in float32 and
float64, and against this package's own host loop (options ar_device_loop = False)."""
import copy

import pytest
import torch

from _util import maxdiff
from flowconductor_amd import options
from oracle import torch_oracle as O
from test_ar_inverse_context_host import SHAPES, build, inputs

pytestmark = pytest.mark.gpu


def _references(t, x, c):
    """Oracle inverse in float32 and float64, the project's bounds for this kernel family, and the conditions on the
    fixture itself (an ill-conditioned one makes both bounds vacuous)."""
    with torch.no_grad():
        y32, lad32 = O.transform_apply(t, x.clone(), c, inverse=True)
        y64, lad64 = O.transform_apply(copy.deepcopy(t).double(), x.double(), c.double(), inverse=True)
    assert float(y64.abs().max()) <= 100, "fixture: the float64 inverse leaves the usable range"
    assert maxdiff(y32, y64) <= 2e-4 * max(1.0, float(y64.abs().max())), "fixture: the float32 oracle is itself far off"
    tol_y = 1e-4 * max(1.0, float(y32.abs().max())) + 4 * maxdiff(y32, y64)
    tol_l = 1e-3 * max(1.0, float(lad32.abs().max()) / 10) + 4 * maxdiff(lad32, lad64)
    return y64, lad64, tol_y, tol_l


def _device_inverse(t, x, c, launches=1):
    """``t.inverse(x, c)`` on the device loop: exactly ``launches`` fc_made_inverse_context, no host-loop hidden stack."""
    from flowconductor_amd import ops

    with ops.KernelTimer("fc_made_inverse_context") as timer, ops.KernelTimer("fc_resnet_hidden_context") as host_timer:
        y, lad = t.inverse(x, c)
    assert len(timer.pairs) == launches and not host_timer.pairs
    return y, lad


@pytest.mark.parametrize("kind,features,hidden,context_features,blocks,n", SHAPES)
def test_conditional_device_loop_matches_the_reference_scheme(kind, features, hidden, context_features, blocks, n, device):
    """Affine and RQ forms, one and two k-steps of the initial layer, 1-32 context features, 0-3 blocks, every parameter-tile
    count, batches that are not whole 16-row blocks.  K = 16 with three blocks has no instantiation (the stack, the context
    layers and three parameter tiles exceed the LDS): it steps aside and must still match."""
    from flowconductor_amd import ops

    t = build(kind, features, hidden, context_features, blocks)
    x, c = inputs(kind, n, features, context_features)
    ref_y64, ref_lad64, tol_y, tol_l = _references(t, x, c)
    t = t.to(device)
    xd, cd = x.to(device), c.to(device)
    per_dim = t._device_loop_form()[1]
    fits = ops.made_inverse_context_fits(features, blocks, per_dim)
    assert fits == (kind != "rq_k16_tails")
    with torch.no_grad():
        assert t._device_loop_ok(xd, cd) == fits
        if fits:
            y, lad = _device_inverse(t, xd, cd)
        else:
            with ops.KernelTimer("fc_made_inverse_context") as timer:
                y, lad = t.inverse(xd, cd)
            assert not timer.pairs
        with options.override(ar_device_loop=False):
            assert not t._device_loop_ok(xd, cd)
            y_host, lad_host = t.inverse(xd, cd)
        z, lad_fwd = t.forward(y, cd)
    print("%s D=%d: |dy| %.3g (tol %.3g)  |dlad| %.3g (tol %.3g)  vs host %.3g %.3g" % (
        kind, features, maxdiff(y, ref_y64), tol_y, maxdiff(lad, ref_lad64), tol_l, maxdiff(y, y_host), maxdiff(lad, lad_host)))
    assert maxdiff(y, ref_y64) <= tol_y and maxdiff(lad, ref_lad64) <= tol_l
    assert maxdiff(y, y_host) <= tol_y and maxdiff(lad, lad_host) <= tol_l
    assert maxdiff(z, x) <= 2 * tol_y and maxdiff(lad + lad_fwd, torch.zeros_like(lad)) <= 2 * tol_l


@pytest.mark.parametrize("features,hidden,context_features,blocks", [(8, 64, 4, 2), (64, 64, 16, 2), (33, 40, 32, 1), (5, 24, 1, 1)])
def test_prefix_passes_equal_whole_passes(features, hidden, context_features, blocks, device):
    """units_needed against the same kernel and pack computing all 64 units (and their context terms) in every pass."""
    from flowconductor_amd import ops

    t = build("rq_k8_tails", features, hidden, context_features, blocks).to(device)
    kind, per_dim, rq = t._device_loop_form()
    z = torch.randn(4096 + 16, features, device=device)
    c = torch.randn(4096 + 16, context_features, device=device)
    with torch.no_grad():
        net = t.autoregressive_net
        packed = ops.pack_made_inverse(net, features, per_dim)
        cpack = ops.pack_made_inverse_context(net, features, per_dim)
        need = packed[-1]
        assert int(need[0]) == 0
        y, lad = ops.made_inverse(z, packed, blocks, per_dim, kind, rq, context=c, context_pack=cpack)
        whole = packed[:-1] + (torch.full_like(need, 64),)
        y_all, lad_all = ops.made_inverse(z, whole, blocks, per_dim, kind, rq, context=c, context_pack=cpack)
        y_t, lad_t = t.inverse(z, c)
    assert maxdiff(y, y_all) <= 2e-6 * max(1.0, float(y_all.abs().max()))
    assert maxdiff(lad, lad_all) <= 2e-5 * max(1.0, float(lad_all.abs().max()) / 10)
    assert maxdiff(y, y_t) <= 1e-6 and maxdiff(lad, lad_t) <= 1e-5


@pytest.mark.parametrize("kind,features,hidden,context_features,blocks,n", SHAPES[:9])
def test_column_zero_ignores_the_context(kind, features, hidden, context_features, blocks, n, device):
    """Dim 0 reads no hidden unit: its parameters are the final layer's biases, whatever the context (bit for bit)."""
    t = build(kind, features, hidden, context_features, blocks).to(device)
    x, c1 = inputs(kind, n, features, context_features)
    c2 = 20 * torch.randn(n, context_features, generator=torch.Generator().manual_seed(6))
    with torch.no_grad():
        y1, _ = _device_inverse(t, x.to(device), c1.to(device))
        y2, _ = _device_inverse(t, x.to(device), c2.to(device))
    assert torch.equal(y1[:, 0], y2[:, 0])
    assert not torch.equal(y1[:, 1], y2[:, 1])


def test_large_contexts_next_to_small_activations(device):
    """Context features of O(20) beside O(1) hidden values: the context operand carries its own row scale."""
    kind, features, hidden, context_features, blocks, n = SHAPES[4]
    t = build(kind, features, hidden, context_features, blocks)
    x, c = inputs(kind, n, features, context_features, context_scale=20.0)
    ref_y64, ref_lad64, tol_y, tol_l = _references(t, x, c)
    t = t.to(device)
    with torch.no_grad():
        y, lad = _device_inverse(t, x.to(device), c.to(device))
        with options.override(ar_device_loop=False):
            y_host, lad_host = t.inverse(x.to(device), c.to(device))
    err_y, err_l = maxdiff(y, ref_y64), maxdiff(lad, ref_lad64)
    host_y, host_l = maxdiff(y_host, ref_y64), maxdiff(lad_host, ref_lad64)
    print("c = 20 randn: device |dy| %.3g |dlad| %.3g, host loop %.3g %.3g, tol %.3g %.3g" % (err_y, err_l, host_y, host_l, tol_y, tol_l))
    assert err_y <= tol_y or err_y <= 2 * host_y
    assert err_l <= tol_l or err_l <= 2 * host_l


@pytest.mark.parametrize("kind", ["maf", "rq"])
def test_conditional_flow_samples_on_the_device_loop(kind, device):
    from flowconductor_amd import distributions, flows, ops, transforms
    from flowconductor_amd.utils import torchutils

    torch.manual_seed(41)
    d, raw_c, emb_c = 6, 5, 4
    layers = []
    for _ in range(3 if kind == "maf" else 2):
        if kind == "maf":
            layers.append(transforms.MaskedAffineAutoregressiveTransform(d, 48, context_features=emb_c))
        else:
            layers.append(transforms.MaskedPiecewiseRationalQuadraticAutoregressiveTransform(
                d, 64, context_features=emb_c, num_bins=8, tails="linear", tail_bound=3.0))
        layers.append(transforms.ReversePermutation(d))
    n_ar = len(layers) // 2
    flow = flows.Flow(transforms.CompositeTransform(layers), distributions.StandardNormal([d]),
                      embedding_net=torch.nn.Linear(raw_c, emb_c)).eval()
    if kind == "rq":
        with torch.no_grad():
            for p in flow._transform.parameters():
                p.mul_(1.5)
    c = torch.randn(64, raw_c)
    flow_cpu = copy.deepcopy(flow)
    flow = flow.to(device)
    cd = c.to(device)
    with torch.no_grad():
        with ops.KernelTimer("fc_made_inverse_context") as timer, ops.KernelTimer("fc_resnet_hidden_context") as host_timer:
            samples = flow.sample(1000, context=cd[:3])
        assert samples.shape == (3, 1000, d)
        assert len(timer.pairs) == n_ar and not host_timer.pairs
        with ops.KernelTimer("fc_made_inverse_context") as timer:
            s, lp = flow.sample_and_log_prob(64, cd)
        assert len(timer.pairs) == n_ar and s.shape == (64, 64, d) and lp.shape == (64, 64)
        rows_c = torchutils.repeat_rows(cd, 64)
        lp_again = flow.log_prob(s.reshape(-1, d), rows_c).reshape(64, 64)
        assert maxdiff(lp, lp_again) <= 2e-3
        noise = torch.randn(64 * 64, d, generator=torch.Generator().manual_seed(3))
        emb = flow._embedding_net(rows_c)
        y_dev, _ = flow._transform.inverse(noise.to(device), emb)
        with options.override(ar_device_loop=False):
            y_host, _ = flow._transform.inverse(noise.to(device), emb)
        emb_cpu = flow_cpu._embedding_net(torchutils.repeat_rows(c, 64))
        y32, _ = O.transform_apply(flow_cpu._transform, noise.clone(), emb_cpu, inverse=True)
        y64, _ = O.transform_apply(copy.deepcopy(flow_cpu._transform).double(), noise.double(), emb_cpu.double(), inverse=True)
    tol_y = 1e-4 * max(1.0, float(y32.abs().max())) + 4 * maxdiff(y32, y64)
    assert maxdiff(y_dev, y_host) <= tol_y and maxdiff(y_dev, y64) <= tol_y


@pytest.mark.parametrize("case", ["context_33", "tanh", "autograd_parameters", "context_requires_grad", "sum_of_sigmoids",
                                  "option_off", "no_context"])
def test_conditional_device_loop_steps_aside(case, device):
    """What the kernel does not cover keeps the host loop and still matches the oracle."""
    from flowconductor_amd import ops
    from flowconductor_amd import transforms as T

    torch.manual_seed(9)
    features, hidden, cf, n = 5, 32, 33 if case == "context_33" else 4, 200
    kw = dict(context_features=cf, num_blocks=2)
    if case == "tanh":
        kw["activation"] = torch.tanh
    if case == "sum_of_sigmoids":
        t = T.MaskedSumOfSigmoidsTransform(features, hidden, n_sigmoids=6, **kw).eval()
    else:
        t = T.MaskedAffineAutoregressiveTransform(features, hidden, **kw).eval()
    g = torch.Generator().manual_seed(5)
    x = torch.randn(n, features, generator=g) * (0.6 if case == "sum_of_sigmoids" else 1.2)
    c = None if case == "no_context" else torch.randn(n, cf, generator=g)      # (no context: made.py adds nothing)
    with torch.no_grad():
        ref_y, ref_lad = O.transform_apply(t, x.clone(), c, inverse=True)
        ref_y64, ref_lad64 = O.transform_apply(copy.deepcopy(t).double(), x.double(), None if c is None else c.double(),
                                               inverse=True)
    tol_y = 1e-4 * max(1.0, float(ref_y.abs().max())) + 4 * maxdiff(ref_y, ref_y64)
    tol_l = 1e-3 * max(1.0, float(ref_lad.abs().max()) / 10) + 4 * maxdiff(ref_lad, ref_lad64)
    t = t.to(device)
    xd = x.to(device)
    cd = None if c is None else c.to(device)
    if case == "context_requires_grad":
        for p in t.parameters():
            p.requires_grad_(False)
        cd.requires_grad_(True)
    grad_on = case in ("autograd_parameters", "context_requires_grad")
    with torch.set_grad_enabled(grad_on), options.override(ar_device_loop=case != "option_off"), \
            ops.KernelTimer("fc_made_inverse_context") as timer, ops.KernelTimer("fc_made_inverse") as plain_timer:
        assert not t._device_loop_ok(xd, cd)
        y, lad = t.inverse(xd, cd)
    assert not timer.pairs and not plain_timer.pairs
    assert maxdiff(y.detach(), ref_y64) <= tol_y and maxdiff(lad.detach(), ref_lad64) <= tol_l


def test_float64_context_steps_aside(device):
    t = build("maf", 6, 64, 3, 2).to(device)
    x, c = inputs("maf", 64, 6, 3)
    with torch.no_grad():
        assert t._device_loop_ok(x.to(device), c.to(device))
        assert not t._device_loop_ok(x.to(device), c.to(device).double())
        assert not t._device_loop_ok(x.to(device), c[:32].to(device))            # rows that do not match the inputs
        assert not t._device_loop_ok(x.to(device), c)                            # a context on another device


def test_caches_follow_the_context_layers(device):
    from flowconductor_amd import ops

    kind, features, hidden, context_features, blocks, n = SHAPES[4]
    t = build(kind, features, hidden, context_features, blocks)
    x, c = inputs(kind, n, features, context_features)
    t = t.to(device)
    xd, cd = x.to(device), c.to(device)
    with torch.no_grad():
        y0, lad0 = _device_inverse(t, xd, cd)
        twin = copy.deepcopy(t)
        assert ops.cached(t.autoregressive_net, "made_inverse_context_pack") is not None
        assert [m for m in twin.modules() if m.__dict__.get("_fc_cache")] == []      # the copy starts cold
        y_twin, lad_twin = _device_inverse(twin, xd, cd)
        assert torch.equal(y_twin, y0) and torch.equal(lad_twin, lad0)
        t.autoregressive_net.blocks[1].context_layer.bias.add_(0.5)
        y1, lad1 = _device_inverse(t, xd, cd)
        ref_y64, ref_lad64, tol_y, tol_l = _references(copy.deepcopy(t).cpu(), x, c)
    assert maxdiff(y1, y0) > 10 * tol_y, "the changed bias did not reach the kernel"
    assert maxdiff(y1, ref_y64) <= tol_y and maxdiff(lad1, ref_lad64) <= tol_l
