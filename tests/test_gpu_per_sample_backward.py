"""The per-sample backward kernels (fc_linear_per_sample_backward, fc_householder_backward_per_sample,
fc_planar_backward_per_sample) against float64 autograd, and the six conditional matrix layers trained through them.

Kernel-level bound, the rule of test_rq_spline_backward_matches_oracle_autograd: 1e-4 of the largest float64 gradient
entry + 8 x what float32 CPU autograd of the same expression loses against float64.  Class- and flow-level bounds are
those of test_hyper_network_transforms_train."""
import copy

import pytest
import torch

import _per_sample_backward_util as U
from _util import maxdiff
from flowconductor_amd import _hip, distributions, flows, ops
from flowconductor_amd import transforms as T
from oracle import torch_oracle as O

pytestmark = pytest.mark.gpu


def _close(got, ref64, ref32, what):
    scale = float(ref64.abs().max())
    err, floor = maxdiff(got.double().cpu(), ref64), maxdiff(ref32.double(), ref64)
    print("%s: err %.3e scale %.3e floor %.3e" % (what, err, scale, floor))
    assert err <= 1e-4 * scale + 8 * floor, what


def _linear_backward(x, gy, gl, m, mode, want_sp=True):
    """One raw launch of fc_linear_per_sample_backward -> (grad_in, grad_m, grad_sp_rows)."""
    lib = _hip.load()
    n, d = x.shape
    gin, gm = torch.empty_like(x), torch.empty_like(m)
    gsp = torch.empty(n, dtype=torch.float32, device=x.device) if want_sp else None
    ops._call("fc_linear_per_sample_backward", lib.fc_linear_per_sample_backward, x.device, _hip.ptr(x), _hip.ptr(gy),
              _hip.ptr(gl), _hip.ptr(m), _hip.ptr(gin), _hip.ptr(gm), _hip.ptr(gsp), n, d, mode, U.OFFDIAG_SCALE, U.EPS,
              _hip.stream_ptr(x.device))
    return gin, gm, gsp


@pytest.mark.parametrize("n,d", U.LINEAR_SHAPES)
@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_linear_backward_kernel_matches_float64(mode, n, d, device):
    x, m, gy, gl = U.linear_case(n, d, 1000 + 10 * d + mode)
    ref64 = U.linear_truth(x, m, gy, gl, mode, torch.float64)
    ref32 = U.linear_truth(x, m, gy, gl, mode, torch.float32)
    # mode 3 takes the saved OUTPUT of the forward call
    first = U.linear_forward(x.double(), m.double(), mode, U.OFFDIAG_SCALE, U.EPS)[0].float() if mode == 3 else x
    args = [t.to(device) for t in (first, gy, gl, m)]
    got = _linear_backward(*args, mode)
    again = _linear_backward(*args, mode)
    for g, a, r64, r32, what in zip(got, again, ref64, ref32, ("grad_in", "grad_m", "grad_sp_rows")):
        assert torch.equal(g, a), what                      # written once per row: bit-identical runs
        if what == "grad_sp_rows" and mode < 2:
            assert float(g.abs().max()) == 0.0
            continue
        _close(g.reshape(r64.shape), r64, r32, "mode %d n %d d %d %s" % (mode, n, d, what))
    # grad_logabsdet = NULL is zeros; grad_sp_rows = NULL is accepted
    zero64 = U.linear_truth(x, m, gy, torch.zeros(n), mode, torch.float64)
    zero32 = U.linear_truth(x, m, gy, torch.zeros(n), mode, torch.float32)
    gin, gm, none = _linear_backward(args[0], args[1], None, args[3], mode, want_sp=False)
    assert none is None
    _close(gin, zero64[0], zero32[0], "no gl: grad_in")
    _close(gm, zero64[1], zero32[1], "no gl: grad_m")


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_linear_autograd_node_and_empty_batch(mode, device):
    """The ops-level node: gradients of inputs, matrices and a 0-dim offdiag_scale tensor; n = 0; no double backward."""
    n, d = 37, 17
    x, m, gy, gl = U.linear_case(n, d, 2000 + mode)
    ref64 = U.linear_truth(x, m, gy, gl, mode, torch.float64)
    ref32 = U.linear_truth(x, m, gy, gl, mode, torch.float32)
    xd, md = x.to(device).requires_grad_(True), m.to(device).requires_grad_(True)
    sp = torch.tensor(U.OFFDIAG_SCALE, device=device, requires_grad=True)
    with ops.KernelTimer("fc_linear_per_sample_backward") as timer:
        y, lad = ops.linear_per_sample_autograd(xd, md, mode=mode, offdiag_scale=sp, eps=U.EPS, want_logabsdet=True)
        assert type(y.grad_fn).__name__ == "_LinearPerSampleFunctionBackward"
        ((y * gy.to(device)).sum() + (lad * gl.to(device)).sum()).backward()
    assert len(timer.pairs) == 1
    with torch.no_grad():
        plain = ops.linear_per_sample(xd, md, mode=mode, offdiag_scale=U.OFFDIAG_SCALE, eps=U.EPS, want_logabsdet=True)
    assert torch.equal(y.detach(), plain[0]) and torch.equal(lad.detach(), plain[1])
    _close(xd.grad, ref64[0], ref32[0], "grad_in")
    _close(md.grad, ref64[1], ref32[1], "grad_m")
    if mode >= 2:
        _close(sp.grad.reshape(1), ref64[2].sum().reshape(1), ref32[2].sum().reshape(1), "grad offdiag_scale")
    else:
        assert float(sp.grad) == 0.0
    # n = 0
    xe, me = torch.zeros(0, d, device=device, requires_grad=True), torch.zeros(0, d, d, device=device, requires_grad=True)
    ye, le = ops.linear_per_sample_autograd(xe, me, mode=mode, offdiag_scale=0.3, eps=U.EPS, want_logabsdet=True)
    (ye.sum() + le.sum()).backward()
    assert xe.grad.shape == (0, d) and me.grad.shape == (0, d, d)
    # double backward is refused
    x2 = x.to(device).requires_grad_(True)
    y2 = ops.linear_per_sample_autograd(x2, m.to(device), mode=mode, offdiag_scale=0.3, eps=U.EPS)
    g2, = torch.autograd.grad(y2.sum(), x2, create_graph=True)
    with pytest.raises(RuntimeError):
        g2.sum().backward()


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("d,k", U.HOUSEHOLDER_SHAPES)
def test_householder_backward_kernel_matches_float64(d, k, reverse, device):
    gen = torch.Generator().manual_seed(31 * d + k)
    n = 21
    x, q, gy = (torch.randn(*s, generator=gen) for s in ((n, d), (n, k, d), (n, d)))
    fwd = lambda a, b: U.householder_forward(a, b, reverse)      # noqa: E731
    ref64 = U.autograd_grads(fwd, (x, q), gy, None, torch.float64)
    ref32 = U.autograd_grads(fwd, (x, q), gy, None, torch.float32)
    runs = []
    for _ in range(2):
        xd, qd = x.to(device).requires_grad_(True), q.to(device).requires_grad_(True)
        with ops.KernelTimer("fc_householder_backward_per_sample") as timer:
            y, lad = ops.householder_autograd(xd, qd, reverse=reverse)
            assert type(y.grad_fn).__name__ == "_HouseholderPerSampleFunctionBackward"
            (y * gy.to(device)).sum().backward()
        assert len(timer.pairs) == 1 and float(lad.abs().max()) == 0.0
        runs.append((xd.grad, qd.grad))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    y64, _ = U.householder_forward(x.double(), q.double(), reverse)
    assert maxdiff(y.detach(), y64) <= 1e-5 * float(y64.abs().max()) * k
    _close(runs[0][0], ref64[0], ref32[0], "d %d k %d gx" % (d, k))
    _close(runs[0][1], ref64[1], ref32[1], "d %d k %d gq" % (d, k))


def test_householder_backward_empty_batch(device):
    xe = torch.zeros(0, 5, device=device, requires_grad=True)
    qe = torch.zeros(0, 3, 5, device=device, requires_grad=True)
    y, _ = ops.householder_autograd(xe, qe)
    y.sum().backward()
    assert xe.grad.shape == (0, 5) and qe.grad.shape == (0, 3, 5)


@pytest.mark.parametrize("d", U.PLANAR_WIDTHS)
def test_planar_backward_kernel_matches_float64(d, device):
    gen = torch.Generator().manual_seed(500 + d)
    n = 37
    x, w, u, gy = (torch.randn(n, d, generator=gen) for _ in range(4))
    w, u = w / d ** 0.5, 0.5 * u / d ** 0.5      # |u.w| stays well below 1: psi = 1 + (1 - t^2) u.w away from 0
    b, gl = torch.randn(n, generator=gen), torch.randn(n, generator=gen)
    truths = {}
    for name, glv in (("gl", gl), ("no gl", torch.zeros(n))):
        truths[name] = (U.autograd_grads(U.planar_forward, (x, w, u, b), gy, glv, torch.float64),
                        U.autograd_grads(U.planar_forward, (x, w, u, b), gy, glv, torch.float32))
    runs = []
    for _ in range(2):
        leaves = [t.to(device).requires_grad_(True) for t in (x, w, u, b)]
        with ops.KernelTimer("fc_planar_backward_per_sample") as timer:
            y, lad = ops.planar_autograd(*leaves, per_sample=True)
            assert type(y.grad_fn).__name__ == "_PlanarPerSampleFunctionBackward"
            ((y * gy.to(device)).sum() + (lad * gl.to(device)).sum()).backward()
        assert len(timer.pairs) == 1
        runs.append([t.grad for t in leaves])
    for a, c in zip(*runs):
        assert torch.equal(a, c)
    for g, r64, r32, what in zip(runs[0], *truths["gl"], ("gx", "gw", "gu", "gb")):
        _close(g, r64, r32, "d %d %s" % (d, what))
    # grad_logabsdet = NULL through the raw entry
    lib = _hip.load()
    xd, wd, ud, bd, gyd = (t.to(device) for t in (x, w, u, b, gy))
    outs = [torch.empty_like(t) for t in (xd, wd, ud, bd)]
    ops._call("fc_planar_backward_per_sample", lib.fc_planar_backward_per_sample, device, _hip.ptr(xd), _hip.ptr(gyd), None,
              _hip.ptr(wd), _hip.ptr(ud), _hip.ptr(bd), *[_hip.ptr(t) for t in outs], n, d, _hip.stream_ptr(device))
    for g, r64, r32, what in zip(outs, *truths["no gl"], ("gx", "gw", "gu", "gb")):
        _close(g, r64, r32, "no gl d %d %s" % (d, what))
    # n = 0
    empty = [torch.zeros(0, d, device=device, requires_grad=True) for _ in range(3)] + [
        torch.zeros(0, device=device, requires_grad=True)]
    ye, le = ops.planar_autograd(*empty, per_sample=True)
    (ye.sum() + le.sum()).backward()
    assert empty[1].grad.shape == (0, d) and empty[3].grad.shape == (0,)


# ---- the six classes under autograd ---------------------------------------------------------------------------------

LINEAR_ENTRY, HOUSEHOLDER_ENTRY, PLANAR_ENTRY = ("fc_linear_per_sample_backward", "fc_householder_backward_per_sample",
                                                 "fc_planar_backward_per_sample")
CLASSES = {
    "lu": (lambda: T.ConditionalLUTransform(5, 16, 4), 5, (LINEAR_ENTRY,)),
    "rotation": (lambda: T.ConditionalRotationTransform(2, 16, 4), 2, (LINEAR_ENTRY,)),
    "orthogonal": (lambda: T.ConditionalOrthogonalTransform(5, 16, 4), 5, (HOUSEHOLDER_ENTRY,)),
    "svd": (lambda: T.ConditionalSVDTransform(5, 16, 4), 5, (HOUSEHOLDER_ENTRY,)),
    "planar": (lambda: T.ConditionalPlanarTransform(5, 16, 4), 5, (PLANAR_ENTRY,)),
    "sylvester": (lambda: T.ConditionalSylvesterTransform(5, 16, 4), 5, (LINEAR_ENTRY, HOUSEHOLDER_ENTRY)),
}


def _check_against_oracle(t, x, c, gy, gl, inverse, entries, device):
    """Outputs, every parameter gradient and the input gradient of ``t`` on the GPU against float64 autograd through the
    oracle; every entry in ``entries`` must have launched."""
    ref = copy.deepcopy(t).double().train()
    x_ref = x.double().requires_grad_(True)
    with O.differentiable_parameters():      # scale_non_diag is a parameter of the layer itself
        y_ref, lad_ref = O.transform_apply(ref, x_ref, c.double(), inverse=inverse)
        ((y_ref * gy.double()).sum() + (lad_ref * gl.double()).sum()).backward()
    gpu = copy.deepcopy(t).to(device).train()
    x_gpu = x.to(device).requires_grad_(True)
    timers = [ops.KernelTimer(name) for name in entries]
    for timer in timers:
        timer.__enter__()
    try:
        y, lad = (gpu.inverse if inverse else gpu)(x_gpu, c.to(device))
        ((y * gy.to(device)).sum() + (lad * gl.to(device)).sum()).backward()
    finally:
        for timer in reversed(timers):
            timer.__exit__(None, None, None)
    for timer in timers:
        assert len(timer.pairs) > 0, timer.name
    assert maxdiff(y.detach(), y_ref.detach()) <= 3e-5 * max(1.0, float(y_ref.detach().abs().max()))
    scale = max(1e-5, float(x_ref.grad.abs().max()))
    assert maxdiff(x_gpu.grad.cpu().double(), x_ref.grad) <= 2e-3 * scale + 1e-6, "input gradient"
    checked = []
    for (name, p_ref), (_, p) in zip(ref.named_parameters(), gpu.named_parameters()):
        if p_ref.grad is None:
            continue
        scale = max(1e-5, float(p_ref.grad.abs().max()))
        assert p.grad is not None and maxdiff(p.grad.cpu().double(), p_ref.grad) <= 2e-3 * scale + 1e-6, name
        checked.append(name)
    return checked


def _class_case(kind):
    torch.manual_seed(79)
    build, d, entries = CLASSES[kind]
    t = build()
    n = 300
    return t, torch.randn(n, d) * 1.2, torch.randn(n, 4), torch.randn(n, d), torch.randn(n), entries


@pytest.mark.parametrize("kind", sorted(CLASSES))
def test_conditional_matrix_layers_train(kind, device):
    t, x, c, gy, gl, entries = _class_case(kind)
    checked = _check_against_oracle(t, x, c, gy, gl, False, entries, device)
    assert len(checked) > 1
    if kind == "lu":
        assert "scale_non_diag" in checked


@pytest.mark.parametrize("kind", ["lu", "rotation", "orthogonal", "svd"])
def test_conditional_matrix_layers_train_through_inverse(kind, device):
    t, x, c, gy, gl, entries = _class_case(kind)
    checked = _check_against_oracle(t, x, c, gy, gl, True, entries, device)
    assert len(checked) > 1
    if kind == "lu":
        assert "scale_non_diag" in checked


def test_conditional_flow_trains(device):
    """-log_prob.mean() of a conditional flow [LU, SVD, planar] over a standard normal: every gradient against the
    float64 oracle."""
    torch.manual_seed(83)
    d, n, ctx_f = 4, 256, 3
    flow = flows.Flow(T.CompositeTransform([T.ConditionalLUTransform(d, 16, ctx_f), T.ConditionalSVDTransform(d, 16, ctx_f),
                                            T.ConditionalPlanarTransform(d, 16, ctx_f)]),
                      distributions.StandardNormal([d])).train()
    x, c = torch.randn(n, d), torch.randn(n, ctx_f)
    ref = copy.deepcopy(flow).double().train()
    with O.differentiable_parameters():
        loss_ref = -O.flow_log_prob(ref, x.double(), c.double()).mean()
        loss_ref.backward()
    gpu = copy.deepcopy(flow).to(device).train()
    with ops.KernelTimer(LINEAR_ENTRY) as t1, ops.KernelTimer(HOUSEHOLDER_ENTRY) as t2, ops.KernelTimer(PLANAR_ENTRY) as t3:
        loss = -gpu.log_prob(x.to(device), c.to(device)).mean()
        loss.backward()
    assert len(t1.pairs) == 1 and len(t2.pairs) == 2 and len(t3.pairs) == 1
    assert abs(loss.item() - loss_ref.item()) <= 3e-5 * max(1.0, abs(loss_ref.item()))
    checked = 0
    for (name, p_ref), (_, p) in zip(ref.named_parameters(), gpu.named_parameters()):
        if p_ref.grad is None:
            continue
        scale = max(1e-5, float(p_ref.grad.abs().max()))
        assert p.grad is not None and maxdiff(p.grad.cpu().double(), p_ref.grad) <= 2e-3 * scale + 1e-6, name
        checked += 1
    assert checked > 6
