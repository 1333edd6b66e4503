"""The element-wise bijector cases of tests/_elementwise_util.py, off the GPU: every input the GPU test feeds is one on which
the float32 reference is finite (so that test skips no element), and the differentiable torch expressions that
``_ElementwiseFunction.backward`` walks (``ops.elementwise_expression``) equal the oracle in float64, values and gradients.

Tolerance of the float64 comparisons: 1e-8 relative to max(1, |reference|) per element.  The two sides differ where the
expression is cancellation-free and the oracle is not; the worst such point of the cases is Tanh forward at |x| = 8.5, where
the oracle's 1 - y^2 = 1.7e-7 carries 2^-53 / 1.7e-7 = 7e-10 of relative error into its logarithm."""
import copy

import pytest
import torch

import _elementwise_util as U
from flowconductor_amd import ops
from oracle import torch_oracle as O

SHAPES = [(U.rows_for(1, False), 1), (U.rows_for(12, True), 12), (U.rows_for(65, False), 65), U.SHAPE_4D, (1, 12)]
TOL = 1e-8


def _close(got, ref, what):
    assert got.shape == ref.shape, what
    excess = (got - ref).abs() - TOL * ref.abs().clamp_min(1.0)
    assert bool((excess <= 0).all()), (what, float(excess.max()))


@pytest.mark.parametrize("name,direction", U.CASES)
def test_float32_reference_is_finite_on_every_case_element(name, direction):
    inverse = direction == "inverse"
    for widths in (U.V4_WIDTHS, U.SCALAR_WIDTHS):
        for m in widths:
            shape = (U.rows_for(m, widths is U.V4_WIDTHS), m)
            for label, module in U.variants(name, m):
                x, context, edge = U.make_inputs(name, direction, module, shape)
                assert bool(edge.any()) and bool(edge.reshape(shape[0], -1)[-1].any()), (label, m)
                y64, lad64, floor_y, floor_lad, y32, lad32 = U.references(name, module, x, context, inverse)
                for t in (y32, lad32, y64, lad64):
                    assert bool(torch.isfinite(t).all()), (label, m)
    for label, module in U.variants(name, 48):
        x, context, _ = U.make_inputs(name, direction, module, U.SHAPE_4D)
        refs = U.references(name, module, x, context, inverse)
        assert all(bool(torch.isfinite(t).all()) for t in (refs[0], refs[1], refs[4], refs[5])), label


def test_tanh_saturates_to_minus_infinity_in_the_float32_reference():
    """The exact cases of the GPU test: at |x| = 9.5 and 50 a float32 tanh is +-1 and the reference's log(1 - y^2) is -inf;
    at 8.5 it is finite, and off by 0.3 against float64 (why the GPU test bounds Tanh's logabsdet without the floor term)."""
    module = U.variants("tanh", 1)[0][1]
    x = torch.tensor([[9.5], [-9.5], [50.0], [-50.0], [8.5], [-8.5]])
    with torch.no_grad():
        y, lad = O.transform_apply(module, x)
        _, lad64 = O.transform_apply(copy.deepcopy(module).double(), x.double())
    assert torch.equal(y[:4], torch.tensor([[1.0], [-1.0], [1.0], [-1.0]]))
    assert bool((lad[:4] == float("-inf")).all()) and bool(torch.isfinite(lad[4:]).all())
    assert 0.2 < float((lad[4:].double() - lad64[4:]).abs().max()) < 0.5


@pytest.mark.parametrize("name,direction", U.CASES)
def test_backward_expression_equals_the_oracle_in_float64(name, direction):
    inverse = direction == "inverse"
    for shape in SHAPES:
        m = 1
        for s in shape[1:]:
            m *= s
        for label, module in U.variants(name, m):
            x, context, _ = U.make_inputs(name, direction, module, shape)
            g = torch.Generator().manual_seed(7)
            gy = torch.randn(shape, generator=g)
            m64 = copy.deepcopy(module).double()
            x64 = x.double().requires_grad_(True)
            c64 = None if context is None else context.double().requires_grad_(True)
            kind, inv, aux, p = U.expression_args(name, m64, c64, inverse)
            aux = None if aux is None else aux.detach().requires_grad_(True)
            y, lad = ops.elementwise_expression(x64, kind, inverse=inv, aux=aux, p=p)
            if name == "glu":
                lad = lad.reshape(-1)
            elif name not in U.PER_ELEMENT:
                lad = lad.reshape(shape[0], -1).sum(dim=1)
            gl = torch.randn(lad.shape, generator=g)
            gx_ref, gp_ref, y_ref, lad_ref = U.oracle_gradients(name, module, x, context, inverse, gy, gl)
            _close(y.detach(), y_ref, (label, shape, "outputs"))
            _close(lad.detach(), lad_ref, (label, shape, "logabsdet"))
            wanted = [x64] + ([] if gp_ref is None else [aux])
            grads = torch.autograd.grad((y * gy.double()).sum() + (lad * gl.double()).sum(), wanted, allow_unused=True)
            assert bool(torch.isfinite(grads[0]).all()), (label, shape)
            _close(grads[0], gx_ref, (label, shape, "input gradient"))
            if gp_ref is not None:
                _close(grads[1].reshape(gp_ref.shape), gp_ref, (label, shape, "parameter gradient"))


def test_backward_expression_stays_finite_where_the_kernel_value_is():
    """Float32, at the points where the textbook forms cancel: Tanh forward up to |x| = 8.5 (1 - y^2 has one or two bits
    left), Sigmoid forward at |temperature x| = 30 (sigmoid rounds to 1)."""
    x = torch.tensor([[0.0, 1e-6, -4.0, 8.5, -8.5]], requires_grad=True)
    y, lad = ops.elementwise_expression(x, ops.EW_TANH)
    gx, = torch.autograd.grad(lad.sum(), x)
    assert bool(torch.isfinite(gx).all())
    assert float((gx.double() + 2.0 * torch.tanh(x.detach().double())).abs().max()) <= 1e-6
    temp = torch.tensor([1.7], requires_grad=True)
    xs = torch.tensor([[30.0 / 1.7, -30.0 / 1.7, 0.3]], requires_grad=True)
    y, lad = ops.elementwise_expression(xs, ops.EW_SIGMOID, aux=temp, p=(1e-6,))
    grads = torch.autograd.grad(lad.sum() + y.sum(), (xs, temp))
    assert all(bool(torch.isfinite(g).all()) for g in grads)
