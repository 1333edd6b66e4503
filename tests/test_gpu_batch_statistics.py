"""Batch statistics on the GPU (``csrc/fc_colstats.hip``): BatchNorm in training mode and the scale / shift gradients of
ActNorm / point-wise affine maps on the batch-axis reduction kernels.

"reference f32" is the reference's expression (normalization.py:98-141) in float32 torch ops on the device, "f64" the same
expression in float64 on the CPU.  A kernel result passes when its error against f64 is at most

    4 * err(reference f32 vs f64) + 1e-6 * max(1, |f64 value|max)

and the variance when its relative error is at most 4 * (reference f32 relative error) + 4 * 2^-23."""
import functools

import pytest
import torch
from torch.nn import functional as F

from flowconductor_amd import flows, ops, options, transforms as T
from flowconductor_amd.transforms.base import InverseNotAvailable

from oracle import torch_oracle as O

from _util import maxdiff

pytestmark = pytest.mark.gpu

G, R = ops.COLSTATS_MAX_PARTIALS, ops.COLSTATS_ROWS_PER_ITERATION
EPS, MOMENTUM = 1e-5, 0.1
SHAPES = [(2, 1), (3, 3), (17, 5), (64, 64), (257, 65), (1000, 2), (4099, 7), (300, 512), (2 * G * R + 3, 4), (G - 1, 8),
          (G * 256 + 1, 4)]     # the last one: 512 slices of 257 rows cover the batch with 511, one partial row is empty
LAUNCHES = ("fc_batchnorm_train", "fc_batchnorm_train_backward", "fc_column_sums")


def timers():
    """A fresh ``KernelTimer`` per launch name of ``LAUNCHES`` (a timer keeps its pairs when it is entered again)."""
    return [ops.KernelTimer(name) for name in LAUNCHES]


def reference(x, uw, bias, eps=EPS):
    weight = F.softplus(uw) + eps
    var, mean = torch.var_mean(x, dim=0)
    y = weight * ((x - mean) / torch.sqrt(var + eps)) + bias
    return y, torch.sum(torch.log(weight) - 0.5 * torch.log(var + eps)) * x.new_ones(x.shape[0]), mean, var


def bound(ref32, ref64, factor=1.0):
    return factor * (4 * maxdiff(ref32, ref64) + 1e-6 * max(1.0, float(ref64.detach().abs().max())))


def check(name, got, ref32, ref64, factor=1.0):
    err, lim = maxdiff(got, ref64), bound(ref32, ref64, factor)
    print("%-28s err %.3e  reference f32 err %.3e  bound %.3e" % (name, err, maxdiff(ref32, ref64), lim))
    assert err <= lim, name


def module(d, device, params):
    t = T.BatchNorm(d, eps=EPS, momentum=MOMENTUM).to(device).train()
    with torch.no_grad():
        t.unconstrained_weight.copy_(params["uw"])
        t.bias.copy_(params["bias"])
        t.running_mean.copy_(params["rm"])
        t.running_var.copy_(params["rv"])
    return t


def gradients(fn, x, uw, bias, gy, gl):
    """``{"full" | "y" | "lad": (gx, guw, gbias)}`` of sum(y gy) + sum(logabsdet gl), of its first and of its second term."""
    x, uw, bias = (t.detach().clone().requires_grad_(True) for t in (x, uw, bias))
    y, lad = fn(x, uw, bias)[:2]
    gy_only = torch.autograd.grad((y, lad), (x, uw, bias), (gy, torch.zeros_like(gl)), retain_graph=True, allow_unused=True)
    gl_only = torch.autograd.grad((y, lad), (x, uw, bias), (torch.zeros_like(gy), gl), retain_graph=True, allow_unused=True)
    full = torch.autograd.grad((y, lad), (x, uw, bias), (gy, gl), allow_unused=True)
    fill = lambda gs: tuple(torch.zeros_like(p) if g is None else g for g, p in zip(gs, (x, uw, bias)))
    return {"full": fill(full), "y": fill(gy_only), "lad": fill(gl_only)}


@functools.lru_cache(maxsize=None)
def case(n, d, offset=0.0):
    """Inputs, the f64 and reference-f32 results, once per shape (shared by the tests; never modified)."""
    device = torch.device("cuda:0")
    g = torch.Generator().manual_seed(1000 * d + n % 997)
    c = {"x": torch.randn(n, d, generator=g) * 1.5 + 0.4 + offset, "uw": torch.randn(d, generator=g),
         "bias": torch.randn(d, generator=g), "rm": torch.randn(d, generator=g), "rv": torch.rand(d, generator=g) + 0.5,
         "gy": torch.randn(n, d, generator=g), "gl": torch.randn(n, generator=g) + 0.25}
    dev = {k: v.to(device) for k, v in c.items()}
    f64 = {k: v.double() for k, v in c.items()}
    with torch.no_grad():
        c["f64"] = reference(f64["x"], f64["uw"], f64["bias"])
        c["f32"] = reference(dev["x"], dev["uw"], dev["bias"])
    c["g64"] = gradients(reference, f64["x"], f64["uw"], f64["bias"], f64["gy"], f64["gl"])
    c["g32"] = gradients(reference, dev["x"], dev["uw"], dev["bias"], dev["gy"], dev["gl"])
    c["dev"] = dev
    return c


def check_forward(c, n, d, device):
    dev = c["dev"]
    t = module(d, device, dev)
    with torch.no_grad(), ops.KernelTimer("fc_batchnorm_train") as launches:
        y, lad = t(dev["x"])
        weight = t.weight
        _, mean, var, invstd, _ = ops.batchnorm_train(dev["x"], weight, t.bias, EPS)
    assert len(launches.pairs) == 2
    y64, lad64, mean64, var64 = c["f64"]
    y32, lad32, mean32, var32 = c["f32"]
    check("y", y, y32, y64)
    check("mean", mean, mean32, mean64)
    check("var", var, var32, var64)
    check("logabsdet", lad, lad32, lad64)
    rel = float(((var.cpu().double() - var64).abs() / var64).max())
    rel32 = float(((var32.cpu().double() - var64).abs() / var64).max())
    print("var relative err %.3e  reference f32 %.3e" % (rel, rel32))
    assert rel <= 4 * rel32 + 4 * 2.0 ** -23
    assert maxdiff(invstd, 1.0 / torch.sqrt(var64 + EPS)) <= 1e-6 * float((1.0 / torch.sqrt(var64 + EPS)).max())
    assert lad.shape == (n,) and bool((lad == lad[0]).all())
    for name, got, start, stat in (("running_mean", t.running_mean, c["rm"], mean64), ("running_var", t.running_var, c["rv"], var64)):
        expect = torch.lerp(start.double(), stat, MOMENTUM)
        assert maxdiff(got, expect) <= 1e-6 * max(1.0, float(expect.abs().max())), name


@pytest.mark.parametrize("n,d", SHAPES)
def test_forward(device, n, d):
    check_forward(case(n, d), n, d, device)


def test_forward_offset_input(device):
    """x = 1000 + noise: a sum-of-squares variance loses every digit here."""
    check_forward(case(4099, 7, 1000.0), 4099, 7, device)


def test_constant_column(device):
    n, d = 257, 5
    x = torch.randn(n, d, device=device)
    x[:, 2] = 3.25
    t = T.BatchNorm(d).to(device).train()
    with torch.no_grad():
        t.bias.copy_(torch.arange(d, dtype=torch.float32))
        y, lad = t(x)
        y64, lad64, _, _ = reference(x.cpu().double(), t.unconstrained_weight.cpu().double(), t.bias.cpu().double())
        y32, lad32, _, _ = reference(x, t.unconstrained_weight, t.bias)
    assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(lad).all())
    assert maxdiff(y[:, 2], torch.full((n,), 2.0)) <= bound(y32, y64)
    check("y", y, y32, y64)
    check("logabsdet", lad, lad32, lad64)


def run_backward(c, d, device, which="full", frozen=False, input_grad=True):
    dev = c["dev"]
    t = module(d, device, dev)
    if frozen:
        t.requires_grad_(False)
    x = dev["x"].clone().requires_grad_(input_grad)
    with ops.KernelTimer("fc_batchnorm_train_backward") as launches:
        y, lad = t(x)
        loss = {"full": lambda: (y * dev["gy"]).sum() + (lad * dev["gl"]).sum(), "y": lambda: (y * dev["gy"]).sum(),
                "lad": lambda: (lad * dev["gl"]).sum()}[which]()
        loss.backward()
    assert len(launches.pairs) == 1
    return x.grad, t.unconstrained_weight.grad, t.bias.grad


@pytest.mark.parametrize("n,d", SHAPES)
def test_backward(device, n, d):
    c = case(n, d)
    for which in ("full", "y", "lad"):
        got = run_backward(c, d, device, which)
        for name, g, g32, g64 in zip(("x.grad", "unconstrained_weight.grad", "bias.grad"), got, c["g32"][which], c["g64"][which]):
            if which == "lad" and name == "bias.grad":
                assert g is None or float(g.abs().max()) == 0.0
                continue
            check("%s %s" % (which, name), g, g32, g64)
    gx, guw, gb = run_backward(c, d, device, frozen=True)
    assert guw is None and gb is None
    check("frozen x.grad", gx, c["g32"]["full"][0], c["g64"]["full"][0])
    gx, guw, gb = run_backward(c, d, device, input_grad=False)
    assert gx is None
    check("no-input-grad weight", guw, c["g32"]["full"][1], c["g64"]["full"][1])
    check("no-input-grad bias", gb, c["g32"]["full"][2], c["g64"]["full"][2])


def test_routing(device):
    n, d = 257, 6
    c = case(n, d)
    dev = c["dev"]

    def step(t, x):
        y, lad = t(x)
        ((y * dev["gy"]).sum() + (lad * dev["gl"]).sum()).backward()
        return y.detach(), lad.detach(), x.grad, t.unconstrained_weight.grad, t.bias.grad, t.running_mean.clone(), t.running_var.clone()

    fwd, bwd, sums = timers()
    with fwd, bwd, sums:
        kernel = step(module(d, device, dev), dev["x"].clone().requires_grad_(True))
    assert (len(fwd.pairs), len(bwd.pairs), len(sums.pairs)) == (1, 1, 0)
    fwd, bwd, sums = timers()
    with options.override(batch_statistics_kernels=False), fwd, bwd, sums:
        torch_route = step(module(d, device, dev), dev["x"].clone().requires_grad_(True))
    assert (len(fwd.pairs), len(bwd.pairs), len(sums.pairs)) == (0, 0, 0)
    y64, lad64 = c["f64"][:2]
    refs64 = (y64, lad64) + c["g64"]["full"]
    refs32 = c["f32"][:2] + c["g32"]["full"]
    for name, a, b, r32, r64 in zip(("y", "logabsdet", "x.grad", "uw.grad", "bias.grad"), kernel, torch_route, refs32, refs64):
        print("%-10s kernels vs torch route %.3e  allowed %.3e" % (name, maxdiff(a, b), 2 * bound(r32, r64)))
        assert maxdiff(a, b) <= 2 * bound(r32, r64), name
    for a, b in zip(kernel[5:], torch_route[5:]):
        assert maxdiff(a, b) <= 2e-6 * max(1.0, float(b.abs().max()))

    act = T.ActNorm(d).to(device).train()
    x = dev["x"].clone().requires_grad_(True)
    with torch.no_grad():
        act(x)                                           # the one-off initialisation
    with ops.KernelTimer("fc_column_sums") as sums:
        y, lad = act(x)
        (y * dev["gy"]).sum().backward()
    assert len(sums.pairs) == 1
    act.zero_grad()
    with options.override(batch_statistics_kernels=False), ops.KernelTimer("fc_column_sums") as sums:
        y, lad = act(x)
        (y * dev["gy"]).sum().backward()
    assert len(sums.pairs) == 0
    act4 = T.ActNorm(d).to(device).train()
    x4 = torch.randn(8, d, 3, 3, device=device, requires_grad=True)
    with ops.KernelTimer("fc_column_sums") as sums:
        y4, _ = act4(x4)
        y4.square().sum().backward()
    assert len(sums.pairs) == 0 and act4.log_scale.grad is not None


@pytest.mark.parametrize("n,d", [(4099, 7), (300, 512), (G * 256 + 1, 4)])
def test_determinism(device, n, d):
    c = case(n, d)
    dev = c["dev"]
    runs = []
    for _ in range(2):
        t = module(d, device, dev)
        x = dev["x"].clone().requires_grad_(True)
        y, lad = t(x)
        ((y * dev["gy"]).sum() + (lad * dev["gl"]).sum()).backward()
        runs.append((y.detach(), lad.detach(), t.running_mean.clone(), t.running_var.clone(), x.grad,
                     t.unconstrained_weight.grad, t.bias.grad))
    assert all(torch.equal(a, b) for a, b in zip(*runs))


def test_support_rule_on_the_device(device):
    ok = ops.batch_statistics_supported
    assert ok(torch.zeros(2, 1, device=device)) and ok(torch.zeros(8, 512, device=device))
    assert ok(torch.zeros(8, 4, device=device).t())                    # (made contiguous by the wrappers)
    assert not ok(torch.zeros(1, 4, device=device)) and not ok(torch.zeros(8, 513, device=device))
    assert not ok(torch.zeros(8, 4, dtype=torch.float64, device=device))
    assert not ok(torch.zeros(8, 4, 2, device=device)) and not ok(torch.zeros(8, device=device))
    with options.override(batch_statistics_kernels=False):
        assert not ops.batch_statistics_route(torch.zeros(8, 4, device=device))
    assert ops.batch_statistics_route(torch.zeros(8, 4, device=device))


def test_strided_input_and_unaligned_view(device):
    """A transposed input is copied to rows by the wrapper; a contiguous view that starts 4 bytes off a 16-byte boundary
    takes the scalar kernels (D % 4 == 0 notwithstanding).  Both against float64."""
    n, d = 300, 8
    base = torch.randn(n * d + 1, device=device) * 1.5 + 0.4
    for x in (base[1:].view(n, d), base[:n * d].view(d, n).t()):
        t = T.BatchNorm(d, eps=EPS).to(device).train()
        xg = x.detach().requires_grad_(True)
        y, lad = t(xg)
        (y.square().sum() + lad.sum()).backward()
        x64 = x.detach().cpu().double().requires_grad_(True)
        y64, lad64 = reference(x64, t.unconstrained_weight.detach().cpu().double(), t.bias.detach().cpu().double())[:2]
        (y64.square().sum() + lad64.sum()).backward()
        x32 = x.detach().clone().requires_grad_(True)
        y32, lad32 = reference(x32, t.unconstrained_weight.detach(), t.bias.detach())[:2]
        (y32.square().sum() + lad32.sum()).backward()
        check("y", y, y32, y64)
        check("logabsdet", lad, lad32, lad64)
        check("x.grad", xg.grad, x32.grad, x64.grad)


def test_fallbacks(device):
    d = 6
    c = case(257, d)
    dev = c["dev"]
    fwd, bwd, sums = timers()
    with fwd, bwd, sums:
        # one row: the reference's unbiased variance is NaN
        t = module(d, device, dev)
        with torch.no_grad():
            y1, lad1 = t(dev["x"][:1])
        assert bool(torch.isnan(y1).all()) and bool(torch.isnan(lad1).all())
        # wider than the kernels take
        wide = T.BatchNorm(513).to(device).train()
        xw = torch.randn(9, 513, device=device, requires_grad=True)
        yw, ladw = wide(xw)
        (yw.square().sum() + ladw.sum()).backward()
        with torch.no_grad():
            y32, lad32, _, _ = reference(xw.detach(), wide.unconstrained_weight, wide.bias)
        assert torch.equal(yw.detach(), y32) and xw.grad is not None
        # float64 on the device
        t64 = module(d, device, dev).double()
        x64 = dev["x"].double().requires_grad_(True)
        y, lad = t64(x64)
        assert y.dtype == torch.float64 and maxdiff(y, c["f64"][0]) <= 1e-12
        assert (len(fwd.pairs), len(bwd.pairs), len(sums.pairs)) == (0, 0, 0)
    # a double backward: the backward is the reference's expression in torch ops
    f64 = {k: v.double() for k, v in c.items() if k in ("x", "uw", "bias", "gy", "gl")}

    def second_order(fn, x, uw, bias, gy, gl):
        x, uw, bias = (v.detach().clone().requires_grad_(True) for v in (x, uw, bias))
        y, lad = fn(x, uw, bias)[:2]
        gx, = torch.autograd.grad((y * gy).sum() + (lad * gl).sum(), x, create_graph=True)
        return torch.autograd.grad(gx.square().sum(), (x, uw))

    ref64 = second_order(reference, f64["x"], f64["uw"], f64["bias"], f64["gy"], f64["gl"])
    ref32 = second_order(reference, dev["x"], dev["uw"], dev["bias"], dev["gy"], dev["gl"])
    t = module(d, device, dev)
    x = dev["x"].clone().requires_grad_(True)
    with ops.KernelTimer("fc_batchnorm_train_backward") as bwd:
        y, lad = t(x)
        gx, = torch.autograd.grad((y * dev["gy"]).sum() + (lad * dev["gl"]).sum(), x, create_graph=True)
        got = torch.autograd.grad(gx.square().sum(), (x, t.unconstrained_weight))
    assert len(bwd.pairs) == 0
    check("second-order x", got[0], ref32[0], ref64[0])
    check("second-order weight", got[1], ref32[1], ref64[1])
    # inverse in training mode, and eval mode
    with pytest.raises(InverseNotAvailable):
        t.inverse(dev["x"])
    t.eval()
    with torch.no_grad(), ops.KernelTimer("fc_batchnorm_train") as fwd:
        y, lad = t(dev["x"])
        expect = ops.batchnorm_eval(dev["x"], t.running_mean, torch.sqrt(t.running_var + t.eps), t.weight, t.bias)
        back, _ = t.inverse(y)
    assert torch.equal(y, expect) and len(fwd.pairs) == 0
    assert maxdiff(back, dev["x"]) <= 1e-4 * float(dev["x"].abs().max())


@pytest.mark.parametrize("n,d", [(3, 3), (257, 65), (4099, 8), (2 * G * R + 3, 4)])
@pytest.mark.parametrize("inverse", [False, True])
def test_pointwise_affine_gradients(device, n, d, inverse):
    """ActNorm / point-wise affine scale, shift and input gradients, [N, D], both directions: f64 against the torch backward
    (``batch_statistics_kernels=False``) as the f32 reference."""
    c = case(n, d)
    dev = c["dev"]
    scale, shift = torch.exp(0.3 * c["uw"]), c["bias"]

    def grads(x, scale, shift, gy, fn):
        x, scale, shift = (v.detach().clone().requires_grad_(True) for v in (x, scale, shift))
        return torch.autograd.grad((fn(x, scale, shift) * gy).sum(), (x, scale, shift))

    plain = (lambda x, s, b: (x - b) / s) if inverse else (lambda x, s, b: x * s + b)
    hip = lambda x, s, b: ops.pointwise_affine_autograd(x, s, b, inverse=inverse)
    ref64 = grads(c["x"].double(), scale.double(), shift.double(), c["gy"].double(), plain)
    with options.override(batch_statistics_kernels=False), ops.KernelTimer("fc_column_sums") as none:
        ref32 = grads(dev["x"], scale.to(device), shift.to(device), dev["gy"], hip)
    with ops.KernelTimer("fc_column_sums") as sums:
        got = grads(dev["x"], scale.to(device), shift.to(device), dev["gy"], hip)
    assert (len(none.pairs), len(sums.pairs)) == (0, 1)
    for name, g, g32, g64 in zip(("x", "scale", "shift"), got, ref32, ref64):
        check("%s grad" % name, g, g32, g64)


def test_actnorm_module_gradients(device):
    n, d = 1000, 2
    c = case(n, d)
    dev = c["dev"]

    def grads(t, x, gy, inverse):
        x = x.detach().clone().requires_grad_(True)
        y, lad = (t.inverse if inverse else t)(x)
        ((y * gy).sum() + lad.sum()).backward()
        out = (x.grad, t.log_scale.grad, t.shift.grad)
        t.zero_grad()
        return out

    act = T.ActNorm(d).to(device).train()
    with torch.no_grad():
        act(dev["x"])
    for inverse in (False, True):
        s64, b64 = (p.detach().cpu().double().requires_grad_(True) for p in (act.log_scale, act.shift))
        x64 = c["x"].double().requires_grad_(True)
        y64 = (x64 - b64) / torch.exp(s64) if inverse else x64 * torch.exp(s64) + b64
        lad64 = (-s64.sum() if inverse else s64.sum()) * x64.new_ones(n)
        ref64 = torch.autograd.grad((y64 * c["gy"].double()).sum() + lad64.sum(), (x64, s64, b64))
        with options.override(batch_statistics_kernels=False):
            ref32 = grads(act, dev["x"], dev["gy"], inverse)
        got = grads(act, dev["x"], dev["gy"], inverse)
        for name, g, g32, g64 in zip(("x", "log_scale", "shift"), got, ref32, ref64):
            check("inverse=%s %s grad" % (inverse, name), g, g32, g64)


def test_maf_with_batch_norm_trains(device):
    import copy

    torch.manual_seed(71)
    n = 400
    flow = flows.MaskedAutoregressiveFlow(features=6, hidden_features=32, num_layers=3, num_blocks_per_layer=1,
                                          batch_norm_between_layers=True)
    ref = copy.deepcopy(flow).double().train()
    gpu = copy.deepcopy(flow).to(device).train()
    x = torch.randn(n, 6) * 1.3 + 0.4
    v, total = x.double(), torch.zeros(n, dtype=torch.float64)
    for layer in ref._transform._transforms:
        if isinstance(layer, T.BatchNorm):
            v, lad = reference(v, layer.unconstrained_weight, layer.bias, layer.eps)[:2]
        else:
            v, lad = O.transform_apply(layer, v)
        total = total + lad
    loss_ref = -(O.standard_normal_log_prob(v) + total).mean()
    loss_ref.backward()
    with ops.KernelTimer("fc_batchnorm_train") as fwd, ops.KernelTimer("fc_batchnorm_train_backward") as bwd:
        loss = -gpu.log_prob(x.to(device)).mean()
        loss.backward()
    assert (len(fwd.pairs), len(bwd.pairs)) == (3, 3)
    assert abs(float(loss.detach()) - float(loss_ref.detach())) <= 1e-4 * max(1.0, abs(float(loss_ref.detach())))
    for (name, p_ref), (_, p) in zip(ref.named_parameters(), gpu.named_parameters()):
        if p_ref.grad is None:
            continue
        scale = max(1e-5, float(p_ref.grad.abs().max()))
        assert p.grad is not None and maxdiff(p.grad, p_ref.grad) <= 1e-3 * scale + 1e-6, name
    gpu.eval()
    with torch.no_grad():
        samples = gpu.sample(64)
        log_prob = gpu.log_prob(samples)
        noise, lad = gpu._transform(samples)
        back, lad_back = gpu._transform.inverse(noise)
    assert bool(torch.isfinite(log_prob).all())
    assert maxdiff(back, samples) <= 1e-4 * max(1.0, float(samples.abs().max()))
    assert maxdiff(lad + lad_back, torch.zeros(64)) <= 1e-4 * max(1.0, float(lad.abs().max()))


def test_saved_memory(device):
    """Forward + backward add at most x.grad, y, gy and one more [N, D] tensor (+ 1 MiB): nothing [N, D] is kept for the
    backward beside the input itself."""
    n, d = 1 << 16, 16
    t = T.BatchNorm(d).to(device).train()
    x = torch.randn(n, d, device=device, requires_grad=True)

    def step():
        y, lad = t(x)
        (y.square().sum() + lad.sum()).backward()

    step()                                               # warm-up: the allocator's pools, the zero / ones helpers
    x.grad = None
    t.zero_grad()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(device)
    before = torch.cuda.memory_allocated(device)
    step()
    torch.cuda.synchronize()
    added = torch.cuda.max_memory_allocated(device) - before
    print("peak added %.2f MiB, allowed %.2f MiB" % (added / 2 ** 20, (4 * n * d * 4 + 2 ** 20) / 2 ** 20))
    assert added <= 4 * n * d * 4 + 2 ** 20
