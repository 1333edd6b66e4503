"""GPU tests of the image-flow layers (SqueezeTransform, OneByOneConvolution, MultiscaleCompositeTransform with
ConvResidualNet couplings): the reference's fixtures, torch view / permute bit for bit, fresh shapes against float64,
round trips, an ill-conditioned inverse, gradients and a whole two-level flow."""
import math

import numpy as np
import pytest
import torch

from _util import golden, maxdiff
from flowconductor_amd import distributions, flows, ops, transforms, utils
from flowconductor_amd.nn import nets

pytestmark = pytest.mark.gpu


class _Lib:
    transforms, nets, utils, flows, distributions = transforms, nets, utils, flows, distributions


def _bound(ref, ref64):
    """The golden rule of test_gpu_golden: 1e-5 x scale + 4 x the reference's own float32 noise floor."""
    ref, ref64 = np.asarray(ref, np.float64), np.asarray(ref64, np.float64)
    return 1e-5 * max(1.0, float(np.max(np.abs(ref64)))) + 4.0 * float(np.max(np.abs(ref - ref64)))


def _check(got, ref, ref64, what):
    bound = _bound(ref, ref64)
    err, err64 = maxdiff(got, ref), maxdiff(got, ref64)
    assert err <= bound and err64 <= bound, (what, err, err64, bound)


def _torch_squeeze(x, f):
    b, c, h, w = x.shape
    return x.reshape(b, c, h // f, f, w // f, f).permute(0, 1, 3, 5, 2, 4).reshape(b, c * f * f, h // f, w // f)


def _torch_unsqueeze(x, f):
    b, c, h, w = x.shape
    return x.reshape(b, c // f ** 2, f, f, h, w).permute(0, 1, 4, 2, 5, 3).reshape(b, c // f ** 2, h * f, w * f)


# ---- SqueezeTransform ---------------------------------------------------------------------------------------------

def test_squeeze_fixture(device):
    g = golden("image_squeeze")
    for f in (2, 3):
        t = transforms.SqueezeTransform(factor=f)
        with torch.no_grad():
            x = torch.from_numpy(g["f%d_x" % f]).to(device)
            z = torch.from_numpy(g["f%d_inv_x" % f]).to(device)
            for y, lad in (t(x), (ops.squeeze(x, f), None)):       # the layer and the kernel itself
                assert torch.equal(y.cpu(), torch.from_numpy(g["f%d_y" % f])) and (lad is None or not lad.any())
            for back, lad in (t.inverse(z), (ops.squeeze(z, f, inverse=True), None)):
                assert torch.equal(back.cpu(), torch.from_numpy(g["f%d_inv_y" % f])) and (lad is None or not lad.any())


@pytest.mark.parametrize("f", (2, 3, 4))
@pytest.mark.parametrize("shape", ((2, 3, 12, 12), (1, 5, 24, 36), (3, 1, 48, 12), (2, 7, 60, 132), (1, 2, 12, 4104)))
def test_squeeze_matches_torch(f, shape, device):
    """The kernel (``ops.squeeze``) and the layer, bit for bit against torch's view / permute."""
    b, c, h, w = shape
    t = transforms.SqueezeTransform(factor=f)
    x = torch.randn(shape, device=device)
    with torch.no_grad():
        z = torch.randn(b, 4 * f * f * c, h // f, w // f, device=device)
        wide = torch.randn(b, c + 2, h, w, device=device)
        tr = torch.randn(b, c, w, h, device=device).transpose(2, 3)
        for fwd, inv in ((lambda v: t(v)[0], lambda v: t.inverse(v)[0]),
                         (lambda v: ops.squeeze(v, f), lambda v: ops.squeeze(v, f, inverse=True))):
            y = fwd(x)
            assert torch.equal(y, _torch_squeeze(x, f))
            assert torch.equal(inv(z), _torch_unsqueeze(z, f))
            if (c * f * f) % 4 == 0:      # the inverse's channel check (see test_image_host)
                assert torch.equal(inv(y), x)
            # a non-contiguous input (a channel slice of a wider tensor, and a transposed view)
            assert torch.equal(fwd(wide[:, 1:c + 1]), _torch_squeeze(wide[:, 1:c + 1], f))
            assert torch.equal(fwd(tr), _torch_squeeze(tr, f))


@pytest.mark.parametrize("f", (2, 3))
@pytest.mark.parametrize("size", (6, 24))
def test_squeeze_gradients_bit_exact(f, size, device):
    """Gradients of both directions bit for bit (the kernel's backward is the other direction of the kernel)."""
    t = transforms.SqueezeTransform(factor=f)
    x = torch.randn(2, 3, size * f, size * f, device=device, requires_grad=True)
    with ops.KernelTimer("fc_squeeze") as timer:
        y, _ = t(x)
        gy = torch.randn_like(y)
        (gx,) = torch.autograd.grad(y, x, gy)
    assert len(timer.pairs) == 2
    x2 = x.detach().clone().requires_grad_(True)
    (gx_ref,) = torch.autograd.grad(_torch_squeeze(x2, f), x2, gy)
    assert torch.equal(gx, gx_ref)
    z = torch.randn(2, 4 * f * f, size, size, device=device, requires_grad=True)
    back, _ = t.inverse(z)
    gb = torch.randn_like(back)
    (gz,) = torch.autograd.grad(back, z, gb)
    z2 = z.detach().clone().requires_grad_(True)
    (gz_ref,) = torch.autograd.grad(_torch_unsqueeze(z2, f), z2, gb)
    assert torch.equal(gz, gz_ref)
    xk = x.detach().clone().requires_grad_(True)       # the kernel's own autograd node at any size
    (gk,) = torch.autograd.grad(ops.squeeze(xk, f), xk, gy)
    assert torch.equal(gk, gx_ref)


# ---- OneByOneConvolution ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", (1, 3, 12, 48, 128))
def test_conv_fixture(c, device):
    g = golden("image_conv_c%d" % c)
    t = transforms.OneByOneConvolution(c)
    t.load_state_dict({k[4:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("sd::")}, strict=True)
    t = t.to(device).eval()
    with torch.no_grad(), ops.KernelTimer("fc_conv1x1") as timer:
        y, lad = t(torch.from_numpy(g["fwd_x"]).to(device))
        x, lad_inv = t.inverse(torch.from_numpy(g["inv_x"]).to(device))
    assert len(timer.pairs) == 2
    _check(y, g["fwd_y"], g["fwd_y64"], "forward")
    _check(lad, g["fwd_lad"], g["fwd_lad64"], "forward logabsdet")
    _check(x, g["inv_y"], g["inv_y64"], "inverse")
    _check(lad_inv, g["inv_lad"], g["inv_lad64"], "inverse logabsdet")


def _random_conv(c, seed, device, offdiag=0.5):
    torch.manual_seed(seed)
    t = transforms.OneByOneConvolution(c, identity_init=False)
    with torch.no_grad():
        t.lower_entries.mul_(2.0 * offdiag)      # uniform(+-offdiag / sqrt(c)) off the diagonal
        t.upper_entries.mul_(2.0 * offdiag)
        t.bias.uniform_(-0.5, 0.5)
    return t.to(device).eval()


def _reference64(t, x, inverse):
    """The reference's composition in float64 on the host: permute, LULinear on rows, permute back."""
    lower, upper = (m.detach().cpu().double() for m in t._create_lower_upper())
    perm = t.permutation._permutation.cpu()
    b, c, h, w = x.shape
    xs = x.detach().cpu().double()
    bias = t.bias.detach().cpu().double()
    if not inverse:
        rows = xs[:, perm].permute(0, 2, 3, 1).reshape(-1, c)
        out = rows @ (lower @ upper).T + bias
        return out.reshape(b, h, w, c).permute(0, 3, 1, 2)
    rows = xs.permute(0, 2, 3, 1).reshape(-1, c) - bias
    out = torch.linalg.solve(lower @ upper, rows.T).T.reshape(b, h, w, c).permute(0, 3, 1, 2)
    return out[:, torch.argsort(perm)]


def _reference32(t, x, inverse):
    """The same composition in float32 on the device (the reference's own float32 noise)."""
    lower, upper = (m.detach() for m in t._create_lower_upper())
    perm = t.permutation._permutation.to(x.device)
    b, c, h, w = x.shape
    if not inverse:
        rows = x[:, perm].permute(0, 2, 3, 1).reshape(-1, c)
        out = (rows @ upper.T) @ lower.T + t.bias.detach()
        return out.reshape(b, h, w, c).permute(0, 3, 1, 2)
    rows = (x.permute(0, 2, 3, 1).reshape(-1, c) - t.bias.detach()).T
    rows = torch.linalg.solve_triangular(lower, rows, upper=False, unitriangular=True)
    out = torch.linalg.solve_triangular(upper, rows, upper=True).T.reshape(b, h, w, c).permute(0, 3, 1, 2)
    return out[:, torch.argsort(perm)]


@pytest.mark.parametrize("c", (1, 2, 3, 4, 5, 8, 12, 16, 17, 31, 32, 48, 64, 96, 127, 128))
@pytest.mark.parametrize("shape", ((3, 5, 7), (1, 16, 16), (2, 9, 4)))
def test_conv_fresh_against_float64(c, shape, device):
    b, h, w = shape
    t = _random_conv(c, 1000 + c, device)
    x = torch.randn(b, c, h, w, device=device)
    with torch.no_grad():
        for inverse in (False, True):
            got, lad = t.inverse(x) if inverse else t(x)
            ref64 = _reference64(t, x, inverse)
            ref32 = _reference32(t, x, inverse)
            _check(got, ref32.cpu().numpy(), ref64.numpy(), ("inverse" if inverse else "forward", c, shape))
            lad64 = h * w * torch.log(t.upper_diag.detach().cpu().double()).sum().item()
            assert abs(lad.cpu().double() - (-lad64 if inverse else lad64)).max() <= 1e-5 * max(1.0, abs(lad64))


@pytest.mark.parametrize("c", (3, 48, 128, 130))
def test_conv_round_trip(c, device):
    t = _random_conv(c, 7 + c, device, offdiag=0.2)
    x = torch.randn(2, c, 8, 6, device=device)
    with torch.no_grad():
        y, lad = t(x)
        back, lad_inv = t.inverse(y)
    assert maxdiff(back, x) <= 1e-5 * max(1.0, x.abs().max().item()) * max(1.0, y.abs().max().item())
    assert maxdiff(lad + lad_inv, torch.zeros_like(lad)) <= 1e-5 * max(1.0, lad.abs().max().item())


def test_conv_ill_conditioned_inverse(device):
    c = 12
    torch.manual_seed(3)
    t = transforms.OneByOneConvolution(c)
    diag = torch.logspace(math.log10(2e-3), 2, c, dtype=torch.float64)[torch.randperm(c)]
    with torch.no_grad():
        t.unconstrained_upper_diag.copy_(torch.log(torch.expm1(diag - t.eps)).float())
        t.lower_entries.copy_(torch.randn(c * (c - 1) // 2) * 0.3)
        t.upper_entries.copy_(torch.randn(c * (c - 1) // 2) * 0.3)
        t.bias.copy_(torch.randn(c))
    t = t.to(device).eval()
    assert float(t.upper_diag.detach().min()) < 3e-3 and float(t.upper_diag.detach().max()) > 90
    x = torch.randn(4, c, 16, 16, device=device)
    with torch.no_grad():
        got, _ = t.inverse(x)
        ref64 = _reference64(t, x, True)
        ref32 = _reference32(t, x, True)
    err, err_ref = maxdiff(got, ref64), maxdiff(ref32, ref64)
    assert err <= 4.0 * err_ref + 1e-6, (err, err_ref)


@pytest.mark.parametrize("c", (1, 5, 12, 64, 128))
@pytest.mark.parametrize("inverse", (False, True))
def test_conv_gradients(c, inverse, device):
    t = _random_conv(c, 50 + c, device, offdiag=0.2).train()
    x = torch.randn(2, c, 5, 6, device=device, requires_grad=True)
    r = torch.randn(2, c, 5, 6, device=device)
    with ops.KernelTimer("fc_conv1x1") as timer:
        y, lad = t.inverse(x) if inverse else t(x)
        loss = (y * r).sum() + 0.5 * lad.sum()
        names = ["lower_entries", "upper_entries", "unconstrained_upper_diag", "bias"]
        grads = torch.autograd.grad(loss, [x] + [getattr(t, n) for n in names])
    assert len(timer.pairs) == 2      # the forward and grad_x both ran the kernel

    # float64 torch restatement
    p64 = {n: getattr(t, n).detach().cpu().double().requires_grad_(True) for n in names}
    x64 = x.detach().cpu().double().requires_grad_(True)
    lower = torch.eye(c, dtype=torch.float64).index_put(tuple(torch.tril_indices(c, c, -1)), p64["lower_entries"])
    diag = torch.nn.functional.softplus(p64["unconstrained_upper_diag"]) + t.eps
    upper = torch.diag(diag).index_put(tuple(torch.triu_indices(c, c, 1)), p64["upper_entries"])
    perm = t.permutation._permutation.cpu()
    w = lower @ upper
    if inverse:
        rows = x64.permute(0, 2, 3, 1).reshape(-1, c) - p64["bias"]
        y64 = torch.linalg.solve(w, rows.T).T.reshape(2, 5, 6, c).permute(0, 3, 1, 2)[:, torch.argsort(perm)]
        lad64 = -30 * torch.log(diag).sum()
    else:
        rows = x64[:, perm].permute(0, 2, 3, 1).reshape(-1, c)
        y64 = (rows @ w.T + p64["bias"]).reshape(2, 5, 6, c).permute(0, 3, 1, 2)
        lad64 = 30 * torch.log(diag).sum()
    loss64 = (y64 * r.cpu().double()).sum() + 0.5 * 2 * lad64
    ref = torch.autograd.grad(loss64, [x64] + [p64[n] for n in names])
    for name, g, g64 in zip(["x"] + names, grads, ref):
        if g64.numel() == 0:          # C = 1 has no strict triangles
            continue
        scale = max(1.0, g64.abs().max().item())
        assert torch.isfinite(g).all(), name
        assert maxdiff(g, g64) <= 2e-5 * scale * max(1.0, math.sqrt(c)), (name, maxdiff(g, g64), scale)


def test_conv_cache(device):
    t = _random_conv(12, 99, device)
    x = torch.randn(3, 12, 7, 5, device=device)
    with torch.no_grad():
        y0, l0 = t(x)
        i0, li0 = t.inverse(x)
        t.use_cache(True)
        for _ in range(2):
            y1, l1 = t(x)
            i1, li1 = t.inverse(x)
            assert maxdiff(y1, y0) <= 1e-6 * max(1.0, y0.abs().max().item())
            assert maxdiff(i1, i0) <= 1e-6 * max(1.0, i0.abs().max().item())
            assert torch.equal(l1, l0) and torch.equal(li1, li0)
        assert t.cache.weight is not None and t.cache.inverse is not None
        t.train()
        assert t.cache.weight is None


# ---- the whole multiscale flow ------------------------------------------------------------------------------------

def _image_flow(device):
    from make_image_golden import build_image_flow

    g = golden("image_flow")
    flow = build_image_flow(_Lib)
    flow.load_state_dict({k[4:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("sd::")}, strict=True)
    return flow.to(device).eval(), g


def test_image_flow_fixture(device):
    flow, g = _image_flow(device)
    with torch.no_grad(), ops.KernelTimer("fc_conv1x1") as conv, ops.KernelTimer("fc_squeeze") as sq:
        lp = flow.log_prob(torch.from_numpy(g["x"]).to(device))
        sample, _ = flow._transform.inverse(torch.from_numpy(g["noise"]).to(device))
    assert len(conv.pairs) == 8 and len(sq.pairs) == 4
    _check(lp, g["log_prob"], g["log_prob64"], "log_prob")
    _check(sample, g["sample"], g["sample64"], "sample")


def test_image_flow_training_step(device):
    flow, g = _image_flow(device)
    flow.train()
    loss = -flow.log_prob(torch.from_numpy(g["x"]).to(device)).mean()
    assert abs(loss.item() - float(g["loss64"])) <= 1e-4 * abs(float(g["loss64"]))
    loss.backward()
    for name, p in flow.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), name
        ref = torch.from_numpy(g["grad::" + name]).double()
        scale = max(1e-2, ref.abs().max().item())
        err = maxdiff(p.grad, ref)
        assert err <= 2e-3 * scale, (name, err, scale)


def test_conv_operands_follow_the_input_device(device):
    """A module left on the host, fed a device input with autograd on (a fresh module is in training mode): the matrix
    and the bias are moved to the input's device, and the result and gradients match the module moved there."""
    torch.manual_seed(5)
    host = transforms.OneByOneConvolution(12, identity_init=False)
    moved = transforms.OneByOneConvolution(12)
    moved.load_state_dict(host.state_dict())
    moved = moved.to(device)
    x = torch.randn(2, 12, 6, 5, device=device)
    y, _ = host(x)
    y_ref, _ = moved(x)
    assert y.device == x.device and maxdiff(y, y_ref) <= 1e-6 * max(1.0, y_ref.abs().max().item())
    y.square().sum().backward()
    y_ref.square().sum().backward()
    for name, p in host.named_parameters():
        assert p.grad is not None and p.grad.device.type == "cpu", name
        ref = dict(moved.named_parameters())[name].grad
        assert maxdiff(p.grad, ref) <= 1e-6 * max(1.0, ref.abs().max().item()), name
    with torch.no_grad():
        back, back_ref = host.eval().inverse(x)[0], moved.eval().inverse(x)[0]
        assert back.device == x.device and maxdiff(back, back_ref) <= 1e-6 * max(1.0, back_ref.abs().max().item())


def test_conv_refuses_float64_parameters(device):
    t = transforms.OneByOneConvolution(4).double().to(device)
    x = torch.randn(1, 4, 3, 3, device=device)
    with pytest.raises(TypeError, match="must be float32"):
        t(x)
    with torch.no_grad(), pytest.raises(TypeError, match="must be float32"):
        t.eval().inverse(x)
    with pytest.raises(TypeError, match="must be float32"):
        ops.conv1x1(x, torch.eye(4, dtype=torch.float64, device=device))
