"""GPU tests of the SPD-matrix layers (FillTriangular, TransformDiagonal*, CholeskyOuterProduct): the reference's
fixtures, fresh inputs against float64 torch, Jacobians, gradients, exceptions and a whole flow."""
import numpy as np
import pytest
import torch

from _util import golden, maxdiff
from flowconductor_amd import distributions, flows, ops, transforms, utils
from flowconductor_amd.nn import nets

pytestmark = pytest.mark.gpu

SIZES = (1, 3, 4, 17, 53, 64, 128)


def _check(got, g, key, what):
    """The golden rule of test_gpu_golden: 1e-5 x scale + 4 x the reference's own float32 noise floor, against the
    reference's float32 and float64 results."""
    ref, ref64 = g[key], g[key + "64"]
    scale = max(1.0, float(np.max(np.abs(ref))))
    floor = float(np.max(np.abs(ref.astype(np.float64) - ref64)))
    bound = 1e-5 * scale + 4.0 * floor
    err, err64 = maxdiff(got, ref), maxdiff(got, ref64)
    assert err <= bound and err64 <= bound, (what, err, err64, bound)


def _sd(g, name):
    return {k.split("::", 2)[2]: torch.from_numpy(g[k]) for k in g.files if k.startswith("sd::%s::" % name)}


def _spd(n, m, seed, device):
    gen = torch.Generator().manual_seed(seed)
    a = torch.randn(n, m, m, generator=gen, dtype=torch.float64)
    s = (a @ a.mT / m + torch.eye(m, dtype=torch.float64)).float()
    return (0.5 * (s + s.mT)).to(device)


def _lower(n, m, seed, device):
    """Well-conditioned lower-triangular matrices (off-diagonal ~ 0.2 / sqrt(m), diagonal in [1, 2])."""
    gen = torch.Generator().manual_seed(seed)
    low = torch.tril(torch.randn(n, m, m, generator=gen), -1) * (0.2 / m ** 0.5)
    return (low + torch.diag_embed(torch.rand(n, m, generator=gen) + 1.0)).to(device)


def _ref_lad(diag64, m):
    powers = torch.arange(m, 0, -1, dtype=torch.float64)
    return m * np.log(2.0) + (powers * diag64.log()).sum(-1)


@pytest.mark.parametrize("m", SIZES)
def test_fixture_parity(m, device):
    g = golden("spd_m%d" % m)
    d = m * (m + 1) // 2
    fill = transforms.FillTriangular(features=d).to(device)
    with torch.no_grad():
        y, lad = fill(torch.from_numpy(g["fill_x"]).to(device))
        assert torch.equal(y.cpu(), torch.from_numpy(g["fill_y"])) and not lad.any()
        back, _ = fill.inverse(y)
        assert torch.equal(back.cpu(), torch.from_numpy(g["fill_inv"]))

    diag = transforms.TransformDiagonalSoftplus(m)
    diag.load_state_dict(_sd(g, "diag"), strict=True)
    diag = diag.to(device)
    with torch.no_grad():
        for direction, inverse in (("fwd", False), ("inv", True)):
            x = torch.from_numpy(g["diag_x" if direction == "fwd" else "diag_inv_x"]).to(device)
            y, lad = (diag.inverse if inverse else diag)(x)
            off = ~torch.eye(m, dtype=torch.bool)
            assert torch.equal(y.cpu()[:, off], x.cpu()[:, off])   # the copy is bit-exact off the diagonal
            _check(y, g, "diag_%s_y" % direction, ("diag", direction))
            _check(lad, g, "diag_%s_lad" % direction, ("diag lad", direction))

    chol = transforms.CholeskyOuterProduct(m)
    chol.load_state_dict(_sd(g, "chol"), strict=True)
    chol = chol.to(device)
    with torch.no_grad():
        y, lad = chol(torch.from_numpy(g["chol_fwd_x"]).to(device))
        _check(y, g, "chol_fwd_y", "chol fwd")
        _check(lad, g, "chol_fwd_lad", "chol fwd lad")
        assert torch.equal(y, y.mT)
        y, lad = chol.inverse(torch.from_numpy(g["chol_inv_x"]).to(device))
        _check(y, g, "chol_inv_y", "chol inv")
        _check(lad, g, "chol_inv_lad", "chol inv lad")
        assert not torch.triu(y, 1).any()


@pytest.mark.parametrize("m", [1, 2, 3, 5, 8, 9, 15, 16, 17, 31, 32, 33, 47, 53, 63, 64, 65, 100, 127, 128, 129])
def test_fresh_inputs_against_float64(m, device):
    n = 37 if m <= 64 else 5        # not a multiple of the matrices per wave
    chol = transforms.CholeskyOuterProduct(m).to(device)
    low = _lower(n, m, 100 + m, device)
    a = _spd(n, m, 200 + m, device)
    with torch.no_grad():
        y, lad = chol(low)
        l64 = low.double().cpu()
        want = l64 @ l64.mT
        assert maxdiff(y, want) <= 2e-6 * max(1.0, want.abs().max().item()) * max(1, m) ** 0.5
        assert maxdiff(lad, _ref_lad(torch.diagonal(l64, dim1=-2, dim2=-1), m)) <= 1e-5 * max(1, m * m)
        got, lad_inv = chol.inverse(a)
        jit = a.double().cpu() + 1e-6 * torch.eye(m, dtype=torch.float64)
        c64 = torch.linalg.cholesky(jit)
        assert maxdiff(got, c64) <= 1e-5 * m
        assert maxdiff(lad_inv, -_ref_lad(torch.diagonal(c64, dim1=-2, dim2=-1), m)) <= 1e-5 * max(1, m * m)
        assert not torch.triu(got, 1).any()
        # round trip
        back, lad_back = chol.inverse(y)
        assert maxdiff(back, low) <= 1e-3
        assert (lad + lad_back).abs().max().item() <= 1e-3 * max(1, m)
    if m <= 128:
        with ops.KernelTimer("fc_cholesky") as t:
            with torch.no_grad():
                chol.inverse(a)
        assert len(t.pairs) == 1, "the HIP factorisation did not run"


@pytest.mark.parametrize("m", [1, 2, 3, 4])
def test_jacobian_logabsdet(m, device):
    """log|det d vec_tril(L L^T) / d vec_tril(L)| by brute force (float64 autograd on the CPU) = the kernel's."""
    chol = transforms.CholeskyOuterProduct(m).to(device)
    idx = torch.tril_indices(m, m)
    low = _lower(3, m, 300 + m, "cpu").double()

    def f(v):
        mat = torch.zeros(m, m, dtype=torch.float64)
        mat[idx[0], idx[1]] = v
        return (mat @ mat.T)[idx[0], idx[1]]

    with torch.no_grad():
        _, lad = chol(low.float().to(device))
    for b in range(3):
        jac = torch.autograd.functional.jacobian(f, low[b][idx[0], idx[1]])
        assert abs(torch.linalg.slogdet(jac)[1].item() - lad[b].item()) <= 1e-4


@pytest.mark.parametrize("m", [1, 3, 8, 17, 64, 100])
def test_forward_gradients(m, device):
    n = 5
    gen = torch.Generator().manual_seed(400 + m)
    # CholeskyOuterProduct without checkargs on a full matrix: the upper part has a gradient too
    chol = transforms.CholeskyOuterProduct(m, checkargs=False).to(device)
    full = (torch.randn(n, m, m, generator=gen) * 0.3 + torch.eye(m) * 2.0)
    gy, gl = torch.randn(n, m, m, generator=gen), torch.randn(n, generator=gen)
    x = full.to(device).requires_grad_(True)
    y, lad = chol(x)
    ((y * gy.to(device)).sum() + (lad * gl.to(device)).sum()).backward()
    x64 = full.double().requires_grad_(True)
    p = x64 @ x64.mT
    y64 = 0.5 * (p + p.mT)
    lad64 = _ref_lad(torch.diagonal(x64, dim1=-2, dim2=-1), m)
    ((y64 * gy.double()).sum() + (lad64 * gl.double()).sum()).backward()
    assert maxdiff(x.grad, x64.grad) <= 1e-4 * max(1.0, x64.grad.abs().max().item())
    assert x.grad.triu(1).abs().sum() > 0 or m == 1

    # FillTriangular
    d = m * (m + 1) // 2
    fill = transforms.FillTriangular(features=d).to(device)
    v = torch.randn(n, d, generator=gen).to(device).requires_grad_(True)
    g = torch.randn(n, m, m, generator=gen).to(device)
    (fill(v)[0] * g).sum().backward()
    idx = torch.tril_indices(m, m)
    assert torch.equal(v.grad.cpu(), g.cpu()[:, idx[0], idx[1]])
    mat = torch.randn(n, m, m, generator=gen).to(device).requires_grad_(True)
    gv = torch.randn(n, d, generator=gen).to(device)
    (fill.inverse(mat)[0] * gv).sum().backward()
    want = torch.zeros(n, m, m)
    want[:, idx[0], idx[1]] = gv.cpu()
    assert torch.equal(mat.grad.cpu(), want)

    # TransformDiagonal (inner transform with a backward of its own, trainable)
    diag = transforms.TransformDiagonal(m, transforms.ScalarScale(scale=1.7, trainable=True)).to(device)
    mat = torch.randn(n, m, m, generator=gen)
    gy = torch.randn(n, m, m, generator=gen)
    gl = torch.randn(n, generator=gen)
    xg = mat.to(device).requires_grad_(True)
    y, lad = diag(xg)
    ((y * gy.to(device)).sum() + (lad * gl.to(device)).sum()).backward()
    x64 = mat.double().requires_grad_(True)
    s64 = torch.tensor(np.log(1.7), dtype=torch.float64, requires_grad=True)
    scale = torch.exp(s64) + 1e-4
    y64 = torch.diagonal_scatter(x64, torch.diagonal(x64, dim1=-2, dim2=-1) * scale, dim1=-2, dim2=-1)
    lad64 = torch.ones(n, dtype=torch.float64) * torch.log(scale) * m
    ((y64 * gy.double()).sum() + (lad64 * gl.double()).sum()).backward()
    assert maxdiff(xg.grad, x64.grad) <= 1e-5 * max(1.0, x64.grad.abs().max().item())
    assert maxdiff(diag.diag_transform._scale.grad, s64.grad) <= 1e-4 * max(1.0, abs(s64.grad.item()))


def test_inverse_gradient_takes_torch_path(device):
    m = 4
    chol = transforms.CholeskyOuterProduct(m).to(device)
    a = _spd(3, m, 9, device).requires_grad_(True)
    with ops.KernelTimer("fc_cholesky") as t:
        y, lad = chol.inverse(a)
    assert not t.pairs
    (y.sum() + lad.sum()).backward()
    a64 = a.detach().double().cpu().requires_grad_(True)
    c = torch.linalg.cholesky(a64 + 1e-6 * torch.eye(m, dtype=torch.float64))
    (c.sum() - _ref_lad(torch.diagonal(c, dim1=-2, dim2=-1), m).sum()).backward()
    assert maxdiff(a.grad, a64.grad) <= 1e-3


def test_checkargs_errors(device):
    m = 5
    chol = transforms.CholeskyOuterProduct(m).to(device)
    low = _lower(4, m, 17, device)
    upper = low.clone()
    upper[2, 0, 3] = 0.5
    negdiag = low.clone()
    negdiag[1, 4, 4] = -1.0
    a = _spd(4, m, 18, device)
    asym = a.clone()
    asym[3, 0, 1] += 1e-3
    notpd = a.clone()
    notpd[2] = -torch.eye(m, device=device)
    cases = [(chol, False, upper, AssertionError, "lower triangular matrices$"),
             (chol, False, negdiag, AssertionError, "positive diagonal elements"),
             (chol, False, torch.ones(2, m, m + 1, device=device), AssertionError, "square"),
             (chol, True, asym, AssertionError, "Input matrix is not symmetric."),
             (chol, True, notpd, AssertionError, "positive semi-definite")]
    for t, inverse, x, exc, msg in cases:
        with torch.no_grad():
            with pytest.raises(exc, match=msg):
                (t.inverse if inverse else t)(x)
            # inside a cascade the device error word is read once at the end: the same exception
            stack = transforms.CompositeTransform([transforms.IdentityTransform(), t])
            with pytest.raises(exc, match=msg):
                (stack.inverse if inverse else stack)(x)
    loose = transforms.CholeskyOuterProduct(m, checkargs=False).to(device)
    with torch.no_grad():
        with pytest.raises(torch.linalg.LinAlgError):
            loose.inverse(notpd)
        with pytest.raises(torch.linalg.LinAlgError):
            transforms.CompositeTransform([loose]).inverse(notpd)
        y, lad = loose(negdiag)          # no check: log of a negative diagonal, as the reference
        assert torch.isnan(lad[1]) and torch.isfinite(lad[0])
        # a clean call after the errors: nothing left in the error word
        chol.inverse(a)
        chol(low)


def _flow(m=3):
    d = m * (m + 1) // 2
    return flows.Flow(transforms.InverseTransform(transforms.CompositeTransform([
        transforms.PiecewiseRationalQuadraticCouplingTransform(
            utils.create_alternating_binary_mask(d, even=True),
            lambda i, o: nets.ResidualNet(i, o, hidden_features=32, num_blocks=2),
            num_bins=8, tails="linear", tail_bound=5.0),
        transforms.FillTriangular(features=d),
        transforms.TransformDiagonalSoftplus(m),
        transforms.CholeskyOuterProduct(m)])), distributions.StandardNormal([d]))


def test_whole_flow(device):
    g = golden("spd_flow_m3")
    flow = _flow()
    sd = {k[4:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("sd::")}
    flow.load_state_dict(sd, strict=True)
    flow = flow.to(device).eval()
    x = torch.from_numpy(g["x"]).to(device)
    with torch.no_grad():
        lp = flow.log_prob(x)
        ref = g["log_prob"]
        assert maxdiff(lp, ref) <= 1e-4 * max(1.0, float(np.abs(ref).max()))
        torch.manual_seed(0)
        s = flow.sample(200)
        assert s.shape == (200, 3, 3) and torch.equal(s, s.mT)
        torch.linalg.cholesky(s.double().cpu())
        s2, lp2 = flow.sample_and_log_prob(200)
        assert torch.equal(s2, s2.mT)
        torch.linalg.cholesky(s2.double().cpu())
        # the same density from both directions; a sample whose L has a tiny diagonal entry feels the eps jitter
        # of the inverse (the reference's own design), hence a bulk bound plus a loose one for every sample
        gap = (flow.log_prob(s2) - lp2).abs()
        assert (gap <= 1e-3 * (1.0 + lp2.abs())).float().mean().item() >= 0.95
        assert gap.max().item() <= 0.1
