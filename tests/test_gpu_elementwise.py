"""fc_elementwise against float64 at every lane-group width, at every branch edge of its nine bijectors, and under autograd.

Cases, edge values and references: tests/_elementwise_util.py.  Bounds against float64 are the project's
(``test_gpu_golden._check``): 1e-5 max(1, max |truth|) + 4 x the float32 reference's own distance from float64, for the
outputs and for the per-row logabsdet (per element for ExtendedSoftplus and GatedLinearUnit).  Tanh forward's logabsdet is
bounded by the first term alone: the float32 reference loses 0.33 at |x| = 8.5 to the cancellation the kernel exists to
avoid, and with that as a floor a wrong cut-over constant would pass.

The bound is one number per tensor, and the edge values set it (exp(80), tan(pi / 2) = 1.6e16 in float64 where float32
gives 2.3e7): each comparison is therefore made twice, over all elements and again over the elements (rows) that hold no
edge value with the scale and the floor of those alone.  No element is left out of the first.

Worst error / bound over all widths and variants, measured on an MI355X (all elements | elements off the edges):

    bijector, direction          outputs         logabsdet
    exp forward                  0.002 | 0.004   0.057 | 0.009
    exp inverse                  0.005 | 0.009   0.076 | 0.051
    tanh forward                 0.009 | 0.009   0.010 | 0.009
    tanh inverse                 0.006 | 0.014   0.047 | 0.019
    logtanh forward              0.011 | 0.017   0.250 | 0.042
    logtanh inverse              0.085 | 0.072   0.250 | 0.025
    leaky_relu forward           0.003 | 0.004   0.010 | 0.010
    leaky_relu inverse           0.002 | 0.004   0.010 | 0.010
    sigmoid forward              0.008 | 0.008   0.010 | 0.013
    sigmoid inverse              0.249 | 0.014   0.249 | 0.038
    logit forward                0.249 | 0.014   0.249 | 0.036
    logit inverse                0.009 | 0.009   0.013 | 0.012
    softplus forward             0.003 | 0.008   0.013 | 0.010
    softplus inverse             0.010 | 0.012   0.012 | 0.012
    cauchy_cdf forward           0.007 | 0.007   0.015 | 0.013
    cauchy_cdf inverse           0.250 | 0.137   0.250 | 0.053
    extended_softplus forward    0.023 | 0.023   0.038 | 0.038
    glu forward                  0.010 | 0.010   0.006 | 0.011
    glu inverse                  0.011 | 0.012   0.006 | 0.011

(0.25: at an edge value the float32 reference is far from float64 and the kernel returns the reference's own number.)

Gradients: the kernel runs forward, ``_ElementwiseFunction.backward`` recomputes the bijector as a float32 torch expression
on the device (there is no HIP backward kernel); max |g - g64| / max |g64| <= 2e-4 (tests/test_gpu_fused_backward.py)."""
import copy

import numpy as np
import pytest
import torch

import _elementwise_util as U
from flowconductor_amd import ops
from flowconductor_amd import transforms as T
from oracle import torch_oracle as O

pytestmark = pytest.mark.gpu

RATIOS = {}


def _apply(name, module, x, context, inverse):
    if name == "extended_softplus":
        return module(x)
    return module.inverse(x, context) if inverse else module(x, context)


def _run(name, module, x, context, inverse, device):
    """The module on the device under no_grad, results on the CPU."""
    with torch.no_grad():
        y, lad = _apply(name, module, x.to(device), None if context is None else context.to(device), inverse)
    return y.cpu(), lad.cpu()


def _ratio(key, got, truth, floor, what):
    err, limit = U.maxabs(got.double() - truth), U.bound(truth, floor)
    RATIOS[key] = max(RATIOS.get(key, 0.0), err / limit)
    assert err <= limit, what + ("err %.3g > bound %.3g (floor %.3g)" % (err, limit, floor),)


def _compare(name, direction, label, y, lad, x, context, edge, module, what):
    """Outputs and logabsdet against float64: over everything, then over the part that holds no edge value."""
    inverse = direction == "inverse"
    y64, lad64, floor_y, floor_lad, y32, lad32 = U.references(name, module, x, context, inverse)
    assert y.shape == y64.shape and lad.shape == lad64.shape, what
    assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(lad).all()), what
    no_floor = name == "tanh" and not inverse
    _ratio((name, direction, "y", "all"), y, y64, floor_y, what + ("outputs",))
    _ratio((name, direction, "lad", "all"), lad, lad64, 0.0 if no_floor else floor_lad, what + ("logabsdet",))
    keep = ~edge
    keep_lad = keep.reshape(lad.shape) if name in U.PER_ELEMENT else ~edge.reshape(edge.shape[0], -1).any(dim=1)
    if bool(keep.any()):
        _ratio((name, direction, "y", "bulk"), y[keep], y64[keep], U.maxabs(y32[keep].double() - y64[keep]),
               what + ("outputs off the edges",))
    if bool(keep_lad.any()):
        floor = 0.0 if no_floor else U.maxabs(lad32[keep_lad].double() - lad64[keep_lad])
        _ratio((name, direction, "lad", "bulk"), lad[keep_lad], lad64[keep_lad], floor, what + ("logabsdet off the edges",))


def _misaligned(t, device):
    """``t`` on the device in a buffer that starts 4 bytes past a 16-byte boundary."""
    flat = torch.empty(t.numel() + 1, dtype=torch.float32, device=device)
    shifted = flat[1:].reshape(t.shape)
    shifted.copy_(t)
    assert shifted.data_ptr() % 16 == 4
    return shifted


@pytest.mark.parametrize("name,direction", U.CASES)
def test_every_width_matches_float64(name, direction, device):
    """Both launch forms at every lane-group width T = 1 ... 64, rows of one and of several trips, idle lanes, three full
    blocks and a partly filled one; n = 1, n = 0 and a 4-D batch; the misaligned twin of an aligned batch bit for bit."""
    inverse = direction == "inverse"
    for vector, widths in ((True, U.V4_WIDTHS), (False, U.SCALAR_WIDTHS)):
        for m in widths:
            shape = (U.rows_for(m, vector), m)
            for label, module in U.variants(name, m):
                x, context, edge = U.make_inputs(name, direction, module, shape)
                gpu = copy.deepcopy(module).to(device)
                y, lad = _run(name, gpu, x, context, inverse, device)
                _compare(name, direction, label, y, lad, x, context, edge, module, (name, direction, label, shape))
                if m in U.MISALIGNED_WIDTHS:
                    # the same rows from a buffer the 16-byte form cannot take: the one-element form at T = 64
                    xd = x.to(device)
                    assert xd.data_ptr() % 16 == 0
                    cd = None if context is None else context.to(device)
                    with torch.no_grad():
                        y_s, lad_s = _apply(name, gpu, _misaligned(x, device), cd, inverse)
                    assert torch.equal(y_s.cpu(), y), (name, direction, label, m)
                    if name in U.PER_ELEMENT:
                        assert torch.equal(lad_s.cpu(), lad), (name, direction, label, m)
                    else:
                        assert U.maxabs(lad_s.cpu() - lad) <= 1e-5 * max(1.0, U.maxabs(lad)), (name, direction, label, m)
                    _compare(name, direction, label, y_s.cpu(), lad_s.cpu(), x, context, edge, module,
                             (name, direction, label, shape, "misaligned"))
    for shape in ((1, 12), (0, 12), U.SHAPE_4D):
        m = int(np.prod(shape[1:]))
        for label, module in U.variants(name, m):
            x, context, edge = U.make_inputs(name, direction, module, shape)
            y, lad = _run(name, copy.deepcopy(module).to(device), x, context, inverse, device)
            # per-row logabsdet is summed over all item dims; the per-element kinds keep the inputs' shape (GLU: flattened)
            expect = {"extended_softplus": tuple(shape), "glu": (int(np.prod(shape)),)}.get(name, (shape[0],))
            assert y.shape == tuple(shape) and lad.shape == expect, (name, direction, label, shape)
            if shape[0]:
                _compare(name, direction, label, y, lad, x, context, edge, module, (name, direction, label, shape))
    print("RATIO %s %s: " % (name, direction) + "  ".join(
        "%s %s %.3f" % (k[2], k[3], v) for k, v in sorted(RATIOS.items()) if k[:2] == (name, direction)))


def test_tanh_saturation_is_exact(device):
    """Where a float32 tanh rounds to +-1 (|x| = 9.5, 50) the outputs are exactly +-1 and the row's logabsdet is -inf, like
    the reference's; at |x| = 8.5 both are finite.  Nothing here lies in (8.5, 9.5), where a correctly rounded tanh and the
    kernel's cut-over may differ."""
    t = T.Tanh().to(device)
    for m in (5, 12):
        x = torch.randn(7, m, generator=torch.Generator().manual_seed(m))
        x[1, 0], x[2, m - 1], x[3, 1], x[4, 2], x[5, 0], x[6, 3] = 9.5, -9.5, 50.0, -50.0, 8.5, -8.5
        with torch.no_grad():
            y, lad = t(x.to(device))
            y_ref, lad_ref = O.transform_apply(T.Tanh(), x)
        y, lad = y.cpu(), lad.cpu()
        assert [float(y[1, 0]), float(y[2, m - 1]), float(y[3, 1]), float(y[4, 2])] == [1.0, -1.0, 1.0, -1.0]
        assert bool((lad[1:5] == float("-inf")).all()) and bool((lad_ref[1:5] == float("-inf")).all())
        assert bool(torch.isfinite(lad[[0, 5, 6]]).all()) and float(y[5:].abs().max()) < 1.0


def test_leaky_relu_zeros_contribute_nothing(device):
    for slope in (0.01, 2.5):
        t = T.LeakyReLU(negative_slope=slope).to(device)
        for m in (3, 8):
            x = torch.zeros(5, m)
            x[:, ::2] = -0.0
            for fn in (t.forward, t.inverse):
                with torch.no_grad():
                    y, lad = fn(x.to(device))
                assert bool((lad == 0.0).all()) and bool((y == 0.0).all())


RAISES = [("Exp", 0.0), ("Tanh", 1.0), ("Tanh", -1.0), ("Sigmoid", float(np.nextafter(np.float32(1), np.float32(2)))),
          ("Sigmoid", -1e-6), ("CauchyCDF", float(np.nextafter(np.float32(1), np.float32(2)))), ("CauchyCDF", -1e-6)]


@pytest.mark.parametrize("kind,bad", RAISES)
def test_inverse_outside_the_domain_raises_and_the_next_call_succeeds(kind, bad, device):
    t = getattr(T, kind)().to(device)
    for shape in ((3, 5), (70, 12)):
        good = torch.full(shape, 0.5, device=device)
        x = good.clone()
        x[shape[0] - 1, shape[1] - 2] = bad
        with pytest.raises(T.InputOutsideDomain):
            with torch.no_grad():
                t.inverse(x)
        with torch.no_grad():           # the error word is cleared
            y, lad = t.inverse(good)
        assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(lad).all())


@pytest.mark.parametrize("kind,values", [("Sigmoid", (0.0, 1.0)), ("CauchyCDF", (0.0, 1.0)), ("Exp", ()), ("Tanh", ())])
def test_inverse_domain_ends_and_nan_do_not_raise(kind, values, device):
    """The closed ends of Sigmoid (clamped to eps) and CauchyCDF are inside the domain.  A NaN compares false like in the
    reference: no error, the NaN stays in its own output element (and its row's sum), every other element keeps its bits."""
    t = getattr(T, kind)().to(device)
    for shape in ((3, 5), (70, 12)):
        x = torch.rand(shape, generator=torch.Generator().manual_seed(3)) * 0.8 + 0.1
        for k, v in enumerate(values):
            x[k, 1] = v
        with torch.no_grad():
            y, lad = t.inverse(x.to(device))
        assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(lad).all())
        row, col = shape[0] - 1, shape[1] - 1
        xn = x.clone()
        xn[row, col] = float("nan")
        with torch.no_grad():
            yn, ladn = t.inverse(xn.to(device))
        others = torch.ones(shape, dtype=torch.bool)
        others[row, col] = False
        assert bool(torch.isnan(yn[row, col])) and torch.equal(yn.cpu()[others], y.cpu()[others])
        assert bool(torch.isnan(ladn[row])) and torch.equal(ladn.cpu()[:row], lad.cpu()[:row])


@pytest.mark.parametrize("name", [n for n, spec in U.BIJECTORS.items() if "inverse" in spec])
def test_round_trip(name, device):
    """inverse(forward(x)) on the bulk of the forward inputs: within 4 x the float32 oracle's own round trip
    + 1e-5 max(1, |x|) (the rule of test_gpu_golden)."""
    for m in (12, 65):
        shape = (U.rows_for(m, m % 4 == 0), m)
        for label, module in U.variants(name, m):
            x, context, _ = U.make_inputs(name, "forward", module, shape, edges=False)
            with torch.no_grad():
                y_ref, _ = U.oracle(name, module, x.clone(), context, False)
                x_ref, _ = U.oracle(name, module, y_ref, context, True)
                gpu = copy.deepcopy(module).to(device)
                cd = None if context is None else context.to(device)
                y, lad = gpu(x.to(device), cd)
                xb, ladb = gpu.inverse(y, cd)
            limit = 4.0 * U.maxabs(x_ref - x) + 1e-5 * max(1.0, U.maxabs(x))
            assert U.maxabs(xb.cpu() - x) <= limit, (name, label, m, U.maxabs(xb.cpu() - x), limit)


# ---- autograd: the kernel forward, the torch recompute backward ----------------------------------------------------------
@pytest.mark.parametrize("name,direction", U.CASES)
def test_gradients_match_float64_autograd(name, direction, device):
    inverse = direction == "inverse"
    for m in U.GRAD_WIDTHS:
        shape = (U.GRAD_ROWS, m)
        for label, module in U.variants(name, m):
            x, context = U.make_grad_inputs(name, direction, module, shape)
            g = torch.Generator().manual_seed(m)
            gy = torch.randn(shape, generator=g)
            gpu = copy.deepcopy(module).to(device)
            with torch.no_grad():
                y0, lad0 = _apply(name, gpu, x.to(device), None if context is None else context.to(device), inverse)
            gl = torch.randn(lad0.shape, generator=g)
            gx_ref, gp_ref, y64, lad64 = U.oracle_gradients(name, module, x, context, inverse, gy, gl)
            xd = x.to(device).requires_grad_(True)
            cd = None if context is None else context.to(device).requires_grad_(True)
            y, lad = _apply(name, gpu, xd, cd, inverse)
            assert torch.equal(y.detach(), y0) and torch.equal(lad.detach(), lad0), (label, m)
            parameter = U.parameter_of(name, gpu, cd)
            wanted = [xd] + ([] if parameter is None else [parameter])
            grads = torch.autograd.grad((y * gy.to(device)).sum() + (lad * gl.to(device)).sum(), wanted)
            assert all(bool(torch.isfinite(t).all()) for t in grads), (label, m)
            assert U.relerr(grads[0], gx_ref) <= 2e-4, (label, m, "inputs", U.relerr(grads[0], gx_ref))
            if parameter is not None:
                got = grads[1].reshape(gp_ref.shape)
                assert U.relerr(got, gp_ref) <= 2e-4, (label, m, "parameter", U.relerr(got, gp_ref))
                # the parameter alone: a layer whose inputs need no gradient still trains
                y, lad = _apply(name, gpu, x.to(device), cd, inverse)
                only, = torch.autograd.grad((y * gy.to(device)).sum() + (lad * gl.to(device)).sum(), [parameter])
                assert U.relerr(only.reshape(gp_ref.shape), gp_ref) <= 2e-4, (label, m, "parameter alone")


def test_flow_with_nonlinearities_trains_every_parameter(device):
    """A coupling layer followed by Sigmoid (learnable temperature), Logit, LeakyReLU and Tanh: one backward of the mean
    logabsdet gives every parameter, ``temperature`` and ``log_negative_slope`` included, the float64 oracle's gradient."""
    from flowconductor_amd import utils
    from flowconductor_amd.nn import nets

    torch.manual_seed(5)
    flow = T.CompositeTransform([
        T.AffineCouplingTransform(utils.create_alternating_binary_mask(6),
                                  lambda i, o: nets.ResidualNet(i, o, hidden_features=16, num_blocks=1)),
        T.Sigmoid(temperature=1.7, learn_temperature=True), T.Logit(), T.LeakyReLU(0.1), T.Tanh()]).eval()
    with torch.no_grad():
        for p in flow._transforms[0].parameters():
            p.add_(torch.randn(p.shape) * 0.1)
    x = torch.randn(64, 6) * 0.7
    ref = copy.deepcopy(flow).double()
    with O.differentiable_parameters():
        y_ref, lad_ref = O.transform_apply(ref, x.double())
    lad_ref.mean().backward()
    gpu = copy.deepcopy(flow).to(device)
    y, lad = gpu(x.to(device))
    lad.mean().backward()
    assert U.maxabs(lad.detach().cpu().double() - lad_ref.detach()) <= 1e-4 * max(1.0, U.maxabs(lad_ref.detach()))
    names = [n for n, _ in gpu.named_parameters()]
    assert "_transforms.1.temperature" in names and "_transforms.3.log_negative_slope" in names
    for (n, p), (_, p_ref) in zip(gpu.named_parameters(), ref.named_parameters()):
        assert p.grad is not None and p_ref.grad is not None, n
        assert float(p_ref.grad.abs().max()) > 0.0, n
        assert U.relerr(p.grad, p_ref.grad) <= 2e-4, (n, U.relerr(p.grad, p_ref.grad))


def test_tanh_returns_an_input_gradient(device):
    """Inputs that require grad and no parameters: a gradient, not the 'autograd is not available' error -- which the bare
    ``ops.elementwise`` keeps."""
    x = (torch.randn(9, 7, generator=torch.Generator().manual_seed(1)) * 2).to(device).requires_grad_(True)
    y, lad = T.Tanh().to(device)(x)
    gx, = torch.autograd.grad(y.sum() + lad.sum(), x)
    t64 = torch.tanh(x.detach().double())
    assert U.relerr(gx, (1 - t64 ** 2) - 2 * t64) <= 2e-4
    empty = torch.zeros(0, 7, device=device, requires_grad=True)
    y, lad = T.Tanh().to(device)(empty)
    g0, = torch.autograd.grad(y.sum() + lad.sum(), empty)
    assert g0.shape == (0, 7) and lad.shape == (0,)
    with pytest.raises(RuntimeError, match="autograd through them is not available"):
        ops.elementwise(x, ops.EW_TANH)
