"""iResBlock training on the GPU (options ``iresblock_training``): one autograd node, ``fc_iresnet_forward`` forward and
``fc_iresnet_backward`` backward, for a call that needs a gradient and computes the exact determinant.

The yardstick is this package's composition in float64 on the CPU.  The floor of each compared tensor is what the
float32 composition (CPU) is off by on the same inputs, and the bound is the project's own,
``1e-5 max(1, |ref|max) + 4 floor`` (``_umnn_util.bound``); every figure is printed before it is asserted.  A
training-mode call moves the power-method vectors, so each route runs once on its own deep copy of the block.
tests/test_iresblock_training_host.py pins the mathematics of the sweep to autograd in float64."""
import copy

import numpy as np
import pytest
import torch

from flowconductor_amd import ops, options, transforms
from flowconductor_amd.nn import nets

import _iresblock_training_util as U
from _umnn_util import bound, maxdiff
from test_iresblock_host import BLOCKS, CONTEXT, build_toy_flow, fixture, load_block, state_dict_of

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
FORWARD, BACKWARD = "fc_iresnet_forward", "fc_iresnet_backward"
KERNEL_BLOCKS = sorted(set(BLOCKS) - {"last_layer"})     # D = 1, 2, 4, 5, 8, 16: the G = 2, 4, 8, 16, 32 instances


@pytest.fixture(autouse=True)
def seeded():
    """The nets that are not loaded from fixtures draw their initial weights and power-method vectors from torch's
    global generator."""
    torch.manual_seed(20261021)


def get_block(name):
    if name == "d3":        # the second dimension of the G = 4 instance
        return U.make_block(nets.DenseNet(dimension=3, densenet_depth=2, densenet_growth=8), 13), 0
    return load_block(name)[0], (CONTEXT if BLOCKS[name][1] else 0)


def set_mode(block, train):
    if train:
        block.train()
        if getattr(block.nnet, "bn", None) is not None:
            block.nnet.bn.eval()        # batch statistics of the context would send the call to the composition
    else:
        block.eval()
    return block


def batch(d, n, context_features, seed):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(n, d, generator=gen)
    context = torch.randn(n, context_features, generator=gen) if context_features else None
    return x, context, torch.randn(n, d, generator=gen), torch.randn(n, generator=gen)


def to_dev(t):
    return None if t is None else t.to(DEV)


def references(block, x, context, gy, gl, inverse=False):
    """Gradients and outputs of the float64 composition, and the float32 composition's distance from them."""
    dbl = lambda t: None if t is None else t.double()
    ref, out = U.named_gradients(U.double_copy(block), dbl(x), dbl(context), gy.double(), gl.double(), inverse)
    with options.override(iresblock_training=False):
        low, out32 = U.named_gradients(copy.deepcopy(block).cpu(), x, context, gy, gl, inverse)
    ref.update(y=out[0], logabsdet=out[1])
    low.update(y=out32[0], logabsdet=out32[1])
    assert set(low) == set(ref)
    return ref, {k: maxdiff(low[k], ref[k]) for k in ref}


def on_gpu(block, x, context, gy, gl, on=True, inverse=False, cap=0):
    """``(gradients + outputs, forward launches, backward launches)`` of a deep copy of ``block`` on the GPU."""
    gpu = copy.deepcopy(block).to(DEV)
    gpu._backward_blocks = cap
    with options.override(iresblock_training=on), ops.KernelTimer(FORWARD) as fw, ops.KernelTimer(BACKWARD) as bw:
        got, out = U.named_gradients(gpu, to_dev(x), to_dev(context), to_dev(gy), to_dev(gl), inverse)
    got.update(y=out[0], logabsdet=out[1])
    return got, len(fw.pairs), len(bw.pairs), gpu


def check(tag, got, ref, floors):
    assert set(got) == set(ref), set(got) ^ set(ref)
    worst = 0.0
    for name in sorted(ref):
        err, limit = maxdiff(got[name], ref[name]), bound(ref[name], floors[name])
        worst = max(worst, err / limit)
        print("%s %s: |gpu - ref64| %.3g, floor %.3g, bound %.3g" % (tag, name, err, floors[name], limit))
    for name in sorted(ref):
        assert torch.isfinite(got[name]).all(), (tag, name)
        assert maxdiff(got[name], ref[name]) <= bound(ref[name], floors[name]), (tag, name)
    return worst


@pytest.mark.parametrize("train", [False, True], ids=["eval", "train"])
@pytest.mark.parametrize("n", [1, 63, 257])
@pytest.mark.parametrize("name", KERNEL_BLOCKS + ["d3"])
def test_gradients(name, n, train):
    block, cf = get_block(name)
    set_mode(block, train)
    args = batch(block.nnet.dimension, n, cf, 17 + n)
    ref, floors = references(block, *args)
    got, forwards, backwards, _ = on_gpu(block, *args)
    assert (forwards, backwards) == (1, 1), "the node did not run"
    assert len(ref) > 6
    check("%s N %d %s" % (name, n, "train" if train else "eval"), got, ref, floors)
    if n == 63:
        _, forwards, backwards, _ = on_gpu(block, *args, on=False)
        assert (forwards, backwards) == (0, 0), "the option is off and a kernel ran"


@pytest.mark.parametrize("act", sorted(U.ACTIVATIONS))
def test_every_activation(act):
    net = nets.DenseNet(dimension=3, densenet_depth=2, densenet_growth=8, activation_function=U.ACTIVATIONS[act]())
    block = U.make_block(net, 23)
    args = batch(3, 63, 0, 29)
    ref, floors = references(block, *args)
    clamped = [k for k in ref if k.endswith("parametrizations.weight.original")]
    assert clamped and all(float(ref[k].abs().max()) > 0 for k in clamped)
    got, forwards, backwards, _ = on_gpu(block, *args)
    assert (forwards, backwards) == (1, 1)
    check(act, got, ref, floors)


@pytest.mark.parametrize("name", ["toy", "default8", "multiplicative_input"])
def test_multi_partial_reduction(name):
    """257 rows with the grid capped at 1, 2 and 3 blocks that stride over the row tiles: the partials' sum stays within
    the bound, a rerun gives the same bits, and permuting the rows permutes dx bitwise."""
    block, cf = get_block(name)
    x, context, gy, gl = batch(block.nnet.dimension, 257, cf, 31)
    ref, floors = references(block, x, context, gy, gl)
    perm = torch.randperm(257, generator=torch.Generator().manual_seed(5))
    for cap in (1, 2, 3):
        got, _, backwards, _ = on_gpu(block, x, context, gy, gl, cap=cap)
        assert backwards == 1
        check("%s cap %d" % (name, cap), got, ref, floors)
        again, _, _, _ = on_gpu(block, x, context, gy, gl, cap=cap)
        for key in got:
            assert torch.equal(got[key], again[key]), (name, cap, key)
        moved, _, _, _ = on_gpu(block, x[perm], None if context is None else context[perm], gy[perm], gl[perm], cap=cap)
        assert torch.equal(moved["x"], got["x"][perm.to(DEV)]), (name, cap)


@pytest.mark.parametrize("train", [False, True], ids=["eval", "train"])
def test_forward_reproduction(train):
    """y and logabsdet of a training call are, bit for bit, ``ops.iresnet_forward`` on the image the call built."""
    block, cf = get_block("input_conditional")
    set_mode(block, train)
    x, context, _, _ = batch(block.nnet.dimension, 257, cf, 37)
    a, b = copy.deepcopy(block).to(DEV), copy.deepcopy(block).to(DEV)
    with options.override(iresblock_training=True), ops.KernelTimer(FORWARD) as fw:
        y, lad = a(to_dev(x).requires_grad_(True), to_dev(context))
    assert len(fw.pairs) == 1 and y.requires_grad and lad.requires_grad
    plan = b._kernel_plan()
    with torch.no_grad():
        image = b._training_image(plan)
        extra, scale = b._extras(plan, to_dev(context))
        y_ref, lad_ref = ops.iresnet_forward(to_dev(x), image, *b._shape_args(plan), extra=extra, scale=scale)
    assert torch.equal(y.detach(), y_ref) and torch.equal(lad.detach(), lad_ref)


def test_power_iteration_buffers():
    """One training-mode call on either route leaves every ``_u`` / ``_v`` buffer with the same bits."""
    block = U.make_block(nets.DenseNet(dimension=3, densenet_depth=2, densenet_growth=8), 41).train()
    args = batch(3, 63, 0, 43)
    _, _, backwards, on = on_gpu(block, *args, on=True)
    _, _, none, off = on_gpu(block, *args, on=False)
    assert (backwards, none) == (1, 0)
    moved = 0
    for (name, u), (_, v), (_, w) in zip(on.named_buffers(), off.named_buffers(), block.named_buffers()):
        if name.endswith("._u") or name.endswith("._v"):
            assert torch.equal(u, v), name
            moved += int(not torch.equal(u.cpu(), w))
    assert moved > 0


def fallback_case(kind):
    """``(block, context features, inverse)`` of a call that must stay on the composition with the option on."""
    if kind == "inverse":
        return load_block("default8")[0], 0, True
    if kind == "d17":
        return U.make_block(nets.DenseNet(dimension=17, densenet_depth=2, densenet_growth=8), 3, rough=False), 0, False
    if kind == "width129":
        return U.make_block(nets.DenseNet(dimension=15, densenet_depth=3, densenet_growth=38,
                                          activation_function="tanh"), 3, rough=False), 0, False
    if kind == "last_layer":
        return load_block("last_layer")[0], CONTEXT, False
    assert kind == "bn_train"
    block = load_block("input_conditional")[0]
    block.nnet.bn.train()
    return block, CONTEXT, False


@pytest.mark.parametrize("kind", ["inverse", "d17", "width129", "last_layer", "bn_train"])
def test_fallbacks(kind):
    block, cf, inverse = fallback_case(kind)
    args = batch(block.nnet.dimension, 63, cf, 47)
    ref, floors = references(block, *args, inverse=inverse)
    got, _, backwards, _ = on_gpu(block, *args, inverse=inverse)
    assert backwards == 0, "a call outside the route ran the backward kernel"
    check(kind, got, ref, floors)


def test_fallback_power_series_in_training_mode():
    """``brute_force=False`` in training mode is a random estimate: it stays on the composition, and under the same seeds
    (numpy draws the number of series terms, torch the probe vectors) the option changes nothing (floor 0: the two runs
    are the same float32 computation)."""
    block = transforms.iResBlock(nets.DenseNet(dimension=3, densenet_depth=2, densenet_growth=8), brute_force=False)
    block.train()
    args = batch(3, 63, 0, 53)
    runs = []
    for on in (False, True):
        np.random.seed(7)
        torch.manual_seed(7)
        got, forwards, backwards, _ = on_gpu(block, *args, on=on)
        assert (forwards, backwards) == (0, 0)
        runs.append(got)
    check("power series", runs[1], runs[0], {k: 0.0 for k in runs[0]})


def test_fallback_float64_module():
    block = U.make_block(nets.DenseNet(dimension=3, densenet_depth=2, densenet_growth=8), 59)
    x, _, gy, gl = batch(3, 63, 0, 61)
    ref, out = U.named_gradients(U.double_copy(block), x.double(), None, gy.double(), gl.double())
    ref.update(y=out[0], logabsdet=out[1])
    got, _, backwards, _ = on_gpu(copy.deepcopy(block).double(), x.double(), None, gy.double(), gl.double())
    assert backwards == 0
    check("float64", got, ref, {k: 0.0 for k in ref})


def test_double_backward_raises():
    block = load_block("toy")[0].to(DEV)
    x = torch.randn(8, 2, device=DEV, requires_grad=True)
    with options.override(iresblock_training=True):
        y, lad = block(x)
        (first,) = torch.autograd.grad(lad.sum() + (y ** 2).sum(), x)      # once is fine
        assert torch.isfinite(first).all()
        y, lad = block(x)
        with pytest.raises(RuntimeError, match="once differentiable"):
            torch.autograd.grad(lad.sum() + (y ** 2).sum(), x, create_graph=True)


def composition_loss(flow, rows):
    """``-log_prob(rows).mean()`` of the toy flow with every iResBlock on the package's composition in the flow's dtype
    on the CPU; ActNorm (``x exp(log_scale) + shift``) and the standard normal, which exist as HIP kernels only, are
    written out in torch."""
    total = rows.new_zeros(rows.shape[0])
    for layer in flow._transform._transforms:
        if isinstance(layer, transforms.ActNorm):
            assert bool(layer.initialized)
            rows, lad = rows * torch.exp(layer.log_scale) + layer.shift, layer.log_scale.sum().expand(rows.shape[0])
        else:
            rows, lad = layer(rows)
        total = total + lad
    log_prob = total - 0.5 * (rows ** 2).sum(1) - 0.5 * rows.shape[1] * float(np.log(2 * np.pi))
    return -log_prob.mean()


def test_toy_flow_training_step():
    """10 x (ActNorm, iResBlock), D 2, depth 3, growth 16, CSin(10), brute force, 257 rows: the loss and every parameter
    gradient of one training step against the float64 composition, ten backward launches, and the step itself."""
    g = fixture("toy_flow")
    flow = build_toy_flow()
    flow.load_state_dict(state_dict_of(g), strict=True)
    flow.train()
    x = torch.randn(257, 2, generator=torch.Generator().manual_seed(67))

    def step(model, rows, loss_fn):
        model.zero_grad()
        loss = loss_fn(model, rows)
        loss.backward()
        grads = {name: p.grad.detach().clone() for name, p in model.named_parameters() if p.grad is not None}
        grads["loss"] = loss.detach()
        return grads

    ref = step(copy.deepcopy(flow).double(), x.double(), composition_loss)
    with options.override(iresblock_training=False):
        low = step(copy.deepcopy(flow), x, composition_loss)
    floors = {k: maxdiff(low[k], ref[k]) for k in ref}
    gpu = copy.deepcopy(flow).to(DEV)
    optimizer = torch.optim.Adam(gpu.parameters(), lr=1e-3)
    with options.override(iresblock_training=True), ops.KernelTimer(FORWARD) as fw, ops.KernelTimer(BACKWARD) as bw:
        got = step(gpu, x.to(DEV), lambda model, rows: -model.log_prob(rows).mean())
    assert (len(fw.pairs), len(bw.pairs)) == (10, 10)
    assert len(ref) > 100
    check("toy flow", got, ref, floors)
    before = [p.detach().clone() for p in gpu.parameters()]
    optimizer.step()
    assert all(torch.isfinite(p).all() for p in gpu.parameters())
    assert any(not torch.equal(p, q) for p, q in zip(gpu.parameters(), before))
