"""Invertible residual blocks on the GPU: ``fc_iresnet_forward`` / ``fc_iresnet_inverse`` behind ``transforms.iResBlock``.

Bounds (none of them comes from what the kernels give):

* fixtures (tests/golden/iresblock_*.npz, recorded from the reference): kernel outputs and logabsdet against the
  fixture's float64 values within 4x the fixture's own float32 noise floor ``max|ref32 - ref64|`` (the factor of
  tests/test_gpu_golden.py: the floor is one realisation of a heavy-tailed error);
* random batches (N = 1, 63, 4096 + 7): the project's parity rule -- rms and p99 of the kernel's error against the
  float64 composition are no larger than those of this package's float32 composition (pinned to the reference by
  tests/test_iresblock_host.py) over the pooled rows; every single batch additionally stays within 4x the float32
  composition's largest error;
* inverse: with ``e_ref = max|ref_inv32 - inv_x64_exact|`` from the fixture, ``e_gpu <= e_ref + 8 eps32 max(1, max|x|)``
  (the added term is the float32 floor of evaluating ``y - g(x)`` once); the round trip ``forward(inverse(y))`` against
  ``y`` within ``(1 + lip_coeff)`` times that bound; no row may reach the 1000-iteration cap.  On random batches the
  same rule with ``e_ref`` taken from this package's float32 composition (the reference's loop) and the float64 fixed
  point iterated to a 1e-13 step.  The inverse's logabsdet is the forward kernel's at the solution, so it is held to
  the forward's bound AT THAT POINT: within 4x the fixture's forward logabsdet floor of the float64 composition
  evaluated at the kernel's own x;
* gradients of the composition on the device against float64: within 4x the error of the float32 composition on the CPU.

Inputs are finite standard-normal rows, the range the fixtures cover."""
import copy

import numpy as np
import pytest
import torch

from flowconductor_amd import ops, transforms
from flowconductor_amd.nn import nets
from flowconductor_amd.nn.nets import activations
from flowconductor_amd.utils.graphs import GraphedCall

from test_iresblock_host import BLOCKS, CONTEXT, EPS32, build_toy_flow, fixture, load_block, state_dict_of, worst

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
KERNEL_BLOCKS = sorted(set(BLOCKS) - {"last_layer"})
LIP = 0.98


def roughen(block, seed, context_features=0):
    """Non-trivial weights as in the golden script: alternate layers scaled past and below the Lipschitz coefficient,
    perturbed biases / concatenation weights, converged power-method vectors, eval mode."""
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        index = 0
        for name, p in block.nnet.named_parameters():
            if name.endswith("parametrizations.weight.original"):
                p.mul_(2.5 if index % 2 == 0 else 0.6)
                index += 1
            elif (name.endswith("bias") and "dense_net" in name) or "unnormalized" in name or name.endswith("beta"):
                p.add_(0.2 * torch.randn(p.shape, generator=gen))
    block.train()
    d = block.nnet.dimension
    context = torch.randn(32, context_features, generator=gen) if context_features else None
    for _ in range(30):
        block(torch.randn(32, d, generator=gen), context)
    return block.eval()


def launches(name, fn):
    with ops.KernelTimer(name) as timer:
        out = fn()
    return out, len(timer.pairs)


def on_cpu64(block, x, context=None, inverse=False):
    block64 = copy.deepcopy(block).double()
    with torch.no_grad():
        f = block64.inverse if inverse else block64
        return f(x.double(), None if context is None else context.double())


def stats(err):
    err = np.abs(np.asarray(err, np.float64)).reshape(-1)
    return float(np.sqrt(np.mean(err ** 2))), float(np.percentile(err, 99)), float(err.max())


@pytest.mark.parametrize("name", KERNEL_BLOCKS)
def test_forward_fixtures(name):
    block, g = load_block(name)
    block.to(DEV)
    context = torch.from_numpy(g["context"]).to(DEV) if BLOCKS[name][1] else None
    with torch.no_grad():
        (y, lad), count = launches("fc_iresnet_forward", lambda: block(torch.from_numpy(g["x"]).to(DEV), context))
    assert count == 1, "the kernel did not run"
    for got, ref32, ref64 in ((y, "y32", "y64"), (lad, "lad32", "lad64")):
        floor, err = worst(g[ref32], g[ref64]), worst(got.cpu().numpy(), g[ref64])
        print("%s %s: |gpu - ref64| %.3g, floor %.3g, ratio %.2f" % (name, ref64, err, floor, err / floor))
        assert err <= 4 * floor, (name, ref64, err, floor)


@pytest.mark.parametrize("name", KERNEL_BLOCKS)
def test_inverse_fixtures(name):
    block, g = load_block(name)
    block.to(DEV)
    context = torch.from_numpy(g["context"]).to(DEV) if BLOCKS[name][1] else None
    y = torch.from_numpy(g["inv_in"]).to(DEV)
    with torch.no_grad():
        (x, lad), count = launches("fc_iresnet_inverse", lambda: block.inverse(y, context))
        back, lad_back = block(x, context)
    assert count == 1, "the kernel did not run"
    iterations = block.inverse_iterations()
    e_ref = worst(g["inv_x32"], g["inv_x64_exact"])
    e_gpu = worst(x.cpu().numpy(), g["inv_x64_exact"])
    bound = e_ref + 8 * EPS32 * max(1.0, float(np.abs(g["inv_x64_exact"]).max()))
    round_trip = worst(back.cpu().numpy(), g["inv_in"])
    print("%s inverse: e_gpu %.3g, e_ref %.3g, bound %.3g, round trip %.3g, %d iterations"
          % (name, e_gpu, e_ref, bound, round_trip, iterations))
    assert iterations < 1000
    assert e_gpu <= bound, (name, e_gpu, bound)
    assert round_trip <= (1 + LIP) * bound, (name, round_trip, bound)
    # logabsdet of the inverse is minus the forward's at the solution: the same kernel at the same point
    assert torch.equal(lad, -lad_back)
    lad_at_x = on_cpu64(block.cpu(), x.cpu(), None if context is None else context.cpu())[1]
    floor = worst(g["lad32"], g["lad64"])
    err = worst(lad.cpu().numpy(), -lad_at_x.numpy())
    print("%s inverse logabsdet against float64 at the kernel's x: %.3g (forward floor %.3g)" % (name, err, floor))
    assert err <= 4 * floor, (name, err, floor)


def exact_fixed_point(block64, y64):
    with torch.no_grad():
        x = y64 - block64.nnet(y64)
        for _ in range(20000):
            new = y64 - block64.nnet(x)
            step = (new - x).abs().max().item()
            x = new
            if step < 1e-13:
                return x
    raise AssertionError("the float64 iteration did not reach a 1e-13 step")


INVERSE_BLOCKS = {      # one per instance of the inverse kernel (4, 8, 16 accumulators); the last one at the width limit
    "d3": lambda: nets.DenseNet(dimension=3),
    "d8": lambda: nets.DenseNet(dimension=8, densenet_depth=3),
    "d16_width128_tanh": lambda: nets.DenseNet(dimension=16, densenet_depth=4, densenet_growth=28,
                                               activation_function="tanh"),
}


@pytest.mark.parametrize("name", sorted(INVERSE_BLOCKS))
def test_inverse_random_batches(name):
    block = roughen(transforms.iResBlock(INVERSE_BLOCKS[name](), brute_force=True), 31)
    block64 = copy.deepcopy(block).double()
    gen = torch.Generator().manual_seed(32)
    d = block.nnet.dimension
    for n in (1, 63, 4096 + 7):
        y = torch.randn(n, d, generator=gen)
        with torch.no_grad():
            x32 = block._inverse_fixed_point(y)
        exact = exact_fixed_point(block64, y.double())
        block.to(DEV)
        with torch.no_grad():
            (x, _), count = launches("fc_iresnet_inverse", lambda: block.inverse(y.to(DEV)))
        iterations = block.inverse_iterations()
        block.cpu()
        assert count == 1, "the kernel did not run"
        e_ref, e_gpu = worst(x32.numpy(), exact.numpy()), worst(x.cpu().numpy(), exact.numpy())
        bound = e_ref + 8 * EPS32 * max(1.0, float(exact.abs().max()))
        print("%s N %d inverse: e_gpu %.3g, e_ref %.3g, bound %.3g, %d iterations" % (name, n, e_gpu, e_ref, bound,
                                                                                       iterations))
        assert iterations < 1000
        assert e_gpu <= bound, (name, n, e_gpu, bound)


def parity(block, name, sizes=(1, 63, 4096 + 7), context_features=0, seed=11):
    gen = torch.Generator().manual_seed(seed)
    d = block.nnet.dimension
    pooled = {"y": ([], []), "lad": ([], [])}
    per_batch = []
    for n in sizes:
        x = torch.randn(n, d, generator=gen)
        context = torch.randn(n, context_features, generator=gen) if context_features else None
        with torch.no_grad():
            y32, lad32 = block(x, context)
        y64, lad64 = on_cpu64(block, x, context)
        block.to(DEV)
        with torch.no_grad():
            (y, lad), count = launches("fc_iresnet_forward",
                                       lambda: block(x.to(DEV), None if context is None else context.to(DEV)))
        block.cpu()
        assert count == 1, "the kernel did not run"
        assert torch.isfinite(y).all() and torch.isfinite(lad).all()
        for key, got, ref32, ref64 in (("y", y, y32, y64), ("lad", lad, lad32, lad64)):
            pooled[key][0].append((got.cpu().double() - ref64).numpy().reshape(-1))
            pooled[key][1].append((ref32.double() - ref64).numpy().reshape(-1))
            per_batch.append((key, n, stats(pooled[key][0][-1])[2]))
    for key in pooled:
        gpu, ref = stats(np.concatenate(pooled[key][0])), stats(np.concatenate(pooled[key][1]))
        print("%s %s: gpu rms %.3g p99 %.3g max %.3g | float32 composition rms %.3g p99 %.3g max %.3g | ratios %.2f %.2f"
              % (name, key, *gpu, *ref, gpu[0] / ref[0], gpu[1] / ref[1]))
        pooled[key] = (gpu, ref)
    for key in pooled:
        gpu, ref = pooled[key]
        assert gpu[0] <= ref[0], (name, key, "rms", gpu, ref)
        assert gpu[1] <= ref[1], (name, key, "p99", gpu, ref)
        for k, n, worst_of_batch in per_batch:
            if k == key:
                assert worst_of_batch <= 4 * ref[2], (name, key, n, worst_of_batch, ref)


@pytest.mark.parametrize("name", KERNEL_BLOCKS)
def test_parity_random_batches(name):
    block, _ = load_block(name)
    parity(block, name, context_features=CONTEXT if BLOCKS[name][1] else 0)


@pytest.mark.parametrize("d", range(1, 17))
def test_every_dimension(d):
    block = roughen(transforms.iResBlock(nets.DenseNet(dimension=d, densenet_depth=2 + d % 2), brute_force=True), d)
    parity(block, "d%d" % d, sizes=(63, 1024 + 7), seed=d)


def test_width_limit_beyond_64k_of_lds():
    """D 16 / depth 4 / growth 28 with a non-concatenating activation: an 8692-float image and 128 x 64 floats of state,
    about 67.5 KiB -- the launches that need the raised dynamic-LDS limit, in 64-thread blocks."""
    block = roughen(transforms.iResBlock(INVERSE_BLOCKS["d16_width128_tanh"](), brute_force=True), 41)
    assert 4 * (ops.iresnet_image_floats(16, 0, 4, 28, ops.IRES_ACT_TANH) + 128 * 64) > 64 * 1024
    parity(block, "d16_width128_tanh", sizes=(63, 1024 + 7))


@pytest.mark.parametrize("activation", ["swish", "LeakyLSwish", "sin"])
def test_other_activations(activation):
    act = activations.Sin(3.0) if activation == "sin" else activation
    block = roughen(transforms.iResBlock(nets.DenseNet(dimension=6, densenet_depth=3, densenet_growth=10,
                                                       activation_function=act), brute_force=True), 5)
    parity(block, activation, sizes=(63, 1024 + 7))


def test_one_past_the_width_limit_falls_back():
    block = roughen(transforms.iResBlock(nets.DenseNet(dimension=16, densenet_depth=4, densenet_growth=30),
                                         brute_force=True), 3)
    x = torch.randn(63, 16, generator=torch.Generator().manual_seed(4))
    with torch.no_grad():
        y32, lad32 = block(x)
    y64, lad64 = on_cpu64(block, x)
    block.to(DEV)
    with torch.no_grad():
        (y, lad), count = launches("fc_iresnet_forward", lambda: block(x.to(DEV)))
        (xi, _), count_inverse = launches("fc_iresnet_inverse", lambda: block.inverse(y))
    assert count == 0 and count_inverse == 0
    for got, ref32, ref64 in ((y, y32, y64), (lad, lad32, lad64)):
        assert worst(got.cpu().numpy(), ref64.numpy()) <= 4 * worst(ref32.numpy(), ref64.numpy())
    for unsupported in ("fullsort", "maxmin"):
        other = transforms.iResBlock(nets.DenseNet(dimension=4, activation_function=unsupported)).eval().to(DEV)
        with torch.no_grad():
            _, count = launches("fc_iresnet_forward", lambda: other(torch.randn(8, 4, device=DEV)))
        assert count == 0


def test_last_layer_conditional_takes_the_composition():
    block, g = load_block("last_layer")
    block.to(DEV)
    with torch.no_grad():
        (y, lad), count = launches("fc_iresnet_forward", lambda: block(torch.from_numpy(g["x"]).to(DEV),
                                                                       torch.from_numpy(g["context"]).to(DEV)))
    assert count == 0
    for got, ref32, ref64 in ((y, "y32", "y64"), (lad, "lad32", "lad64")):
        assert worst(got.cpu().numpy(), g[ref64]) <= 4 * worst(g[ref32], g[ref64])


def test_training_and_gradients_take_the_composition():
    block, g = load_block("default8")
    x = torch.from_numpy(g["x"])

    def gradients(module, rows):
        module.zero_grad()
        rows = rows.clone().requires_grad_(True)
        y, lad = module(rows)
        (lad.sum() + (y ** 2).sum()).backward()
        return [rows.grad.clone()] + [p.grad.clone() for _, p in sorted(module.named_parameters())
                                      if p.grad is not None]

    ref32 = gradients(block, x)
    ref64 = gradients(copy.deepcopy(block).double(), x.double())
    block.to(DEV)
    got, count = launches("fc_iresnet_forward", lambda: gradients(block, x.to(DEV)))
    assert count == 0, "a call that needs gradients went to the kernel"
    assert len(got) == len(ref64) > 3
    for a, b, c in zip(got, ref32, ref64):
        assert worst(a.cpu().numpy(), c.numpy()) <= 4 * max(worst(b.numpy(), c.numpy()), EPS32 * float(c.abs().max()))
    # parameters that require grad send an eval-mode call with autograd on to the composition; no_grad to the kernel
    _, count = launches("fc_iresnet_forward", lambda: block(x.to(DEV)))
    assert count == 0
    with torch.no_grad():
        _, count = launches("fc_iresnet_forward", lambda: block(x.to(DEV)))
    assert count == 1
    block.train()
    with torch.no_grad():
        _, count = launches("fc_iresnet_forward", lambda: block(x.to(DEV)))
    assert count == 0, "train() mode took the kernel"
    # back in eval mode the image is rebuilt from the power-method vectors that the training pass moved
    block.eval()
    reference = copy.deepcopy(block).cpu()
    with torch.no_grad():
        (y, lad), count = launches("fc_iresnet_forward", lambda: block(x.to(DEV)))
        y32, lad32 = reference(x)
    y64, lad64 = on_cpu64(reference, x)
    assert count == 1
    assert worst(y.cpu().numpy(), y64.numpy()) <= 4 * worst(y32.numpy(), y64.numpy())
    assert worst(lad.cpu().numpy(), lad64.numpy()) <= 4 * worst(lad32.numpy(), lad64.numpy())


def test_image_follows_plain_number_constants():
    """``CSin.w0`` is a Python float inside the image: changing it must re-pack, as the composition changes."""
    block, g = load_block("toy")
    x = torch.from_numpy(g["x"])
    block.to(DEV)
    with torch.no_grad():
        before, _ = block(x.to(DEV))
        block.nnet.activation.w0 = 4.0
        (after, lad), count = launches("fc_iresnet_forward", lambda: block(x.to(DEV)))
    assert count == 1 and not torch.equal(before, after)
    block.cpu()
    with torch.no_grad():
        y32, lad32 = block(x)
    y64, lad64 = on_cpu64(block, x)
    assert worst(after.cpu().numpy(), y64.numpy()) <= 4 * worst(y32.numpy(), y64.numpy())
    assert worst(lad.cpu().numpy(), lad64.numpy()) <= 4 * worst(lad32.numpy(), lad64.numpy())


def test_submodule_in_training_mode_takes_the_composition():
    """``net.bn.train()`` on a warm block: the call goes to the composition (which then normalises by batch statistics, as
    the reference would), it does not raise and it does not run the kernel on a stale image."""
    block, g = load_block("input_conditional")
    block.to(DEV)
    x, context = torch.from_numpy(g["x"]).to(DEV), torch.from_numpy(g["context"]).to(DEV)
    with torch.no_grad():
        _, count = launches("fc_iresnet_forward", lambda: block(x, context))
        assert count == 1
        block.nnet.bn.train()
        (y, lad), count = launches("fc_iresnet_forward", lambda: block(x, context))
        assert count == 0
        reference = copy.deepcopy(block).cpu()
        y32, lad32 = reference(x.cpu(), context.cpu())
        y64, lad64 = on_cpu64(copy.deepcopy(block).cpu(), x.cpu(), context.cpu())
        assert worst(y.cpu().numpy(), y64.numpy()) <= 4 * worst(y32.numpy(), y64.numpy())
        block.nnet.bn.eval()
        _, count = launches("fc_iresnet_forward", lambda: block(x, context))
        assert count == 1


def test_round_trip_random():
    block = roughen(transforms.iResBlock(nets.DenseNet(dimension=8), brute_force=True), 21).to(DEV)
    y = torch.randn(4096 + 7, 8, generator=torch.Generator().manual_seed(22)).to(DEV)
    with torch.no_grad():
        x, lad = block.inverse(y)
        back, lad_back = block(x)
    # the stopping test bounds the residual: y - (x_prev + g(x_prev)) = x - x_prev, one more contraction for x itself
    tol = 1e-5 + 1e-5 * y.abs()
    excess = ((back - y).abs() - LIP * tol - 8 * EPS32 * torch.clamp(y.abs(), min=1.0)).max().item()
    print("round trip: largest excess over the stopping tolerance %.3g, %d iterations"
          % (excess, block.inverse_iterations()))
    assert excess <= 0
    assert block.inverse_iterations() < 1000
    assert torch.equal(lad, -lad_back)


def exact_flow_inverse(flow64, noise64):
    """The toy flow's inverse in float64 with every block's fixed point iterated to a 1e-13 step."""
    rows = noise64
    with torch.no_grad():
        for layer in reversed(list(flow64._transform._transforms)):
            if isinstance(layer, transforms.ActNorm):
                rows = (rows - layer.shift) / torch.exp(layer.log_scale)
                continue
            x = rows - layer.nnet(rows)
            for _ in range(20000):
                new = rows - layer.nnet(x)
                step = (new - x).abs().max().item()
                x = new
                if step < 1e-13:
                    break
            assert step < 1e-13
            rows = x
    return rows


def test_toy_flow():
    g = fixture("toy_flow")
    flow = build_toy_flow()
    flow.load_state_dict(state_dict_of(g), strict=True)
    flow.eval()
    exact = exact_flow_inverse(copy.deepcopy(flow).double(), torch.from_numpy(g["noise"]).double()).numpy()
    flow.to(DEV)
    x = torch.from_numpy(g["x"]).to(DEV)
    with torch.no_grad():
        lp, count = launches("fc_iresnet_forward", lambda: flow.log_prob(x))
        assert count == 10
        floor, err = worst(g["log_prob32"], g["log_prob64"]), worst(lp.cpu().numpy(), g["log_prob64"])
        print("toy flow log_prob: |gpu - ref64| %.3g, floor %.3g" % (err, floor))
        assert err <= 4 * floor
        (s, lad), count = launches("fc_iresnet_inverse",
                                   lambda: flow._transform.inverse(torch.from_numpy(g["noise"]).to(DEV)))
        assert count == 10
        e_ref, e_gpu = worst(g["sample32"], exact), worst(s.cpu().numpy(), exact)
        bound = e_ref + 10 * 8 * EPS32 * max(1.0, float(np.abs(exact).max()))       # one evaluation floor per block
        print("toy flow inverse: e_gpu %.3g, e_ref %.3g, bound %.3g" % (e_gpu, e_ref, bound))
        assert e_gpu <= bound
        for layer in flow._transform._transforms:
            if isinstance(layer, transforms.iResBlock):
                assert layer.inverse_iterations() < 1000
        (samples, log_prob), count = launches("fc_iresnet_inverse", lambda: flow.sample_and_log_prob(257))
        assert count == 10 and samples.shape == (257, 2) and log_prob.shape == (257,)
        assert torch.isfinite(samples).all() and torch.isfinite(log_prob).all()
        # replay inside a HIP graph: no host sync on the path, the same numbers as the direct call
        graphed = GraphedCall(flow.log_prob, x)
        assert torch.equal(graphed(x), lp)
        shifted = x + 0.25
        assert torch.equal(graphed(shifted), flow.log_prob(shifted))
        graphed_inverse = GraphedCall(lambda rows: flow._transform.inverse(rows)[0], x)
        assert torch.equal(graphed_inverse(x), flow._transform.inverse(x)[0])
