"""Cases for the element-wise bijectors of ``fc_elementwise`` (Exp, Tanh, LogTanh, LeakyReLU, Sigmoid / Logit, Softplus,
CauchyCDF, ExtendedSoftplus, GatedLinearUnit), shared by tests/test_elementwise_host.py and tests/test_gpu_elementwise.py.
Imports no GPU.

One table: per bijector its module variants and, per direction, the bulk distribution of the inputs and the edge values
written over it.  The edge values go to fixed flat positions counted from both ends of the tensor (every third element of
the first and of the last rows), so every row width holds some of them, in the first block and in the partly filled last.

The reference is ``oracle.torch_oracle``: on a ``copy.deepcopy(module).double()`` with double inputs for the truth, on the
module itself in float32 on the CPU for the noise floor, floor = max |oracle32 - oracle64| (the rule of
``test_gpu_golden._check``)."""
import copy

import numpy as np
import torch
import torch.nn.functional as F

from flowconductor_amd import ops
from flowconductor_amd import transforms as T
from oracle import torch_oracle as O

# 16-byte form, T = 1, 2, 4, 4, 8, 16, 32, 32, 64, 64 (two trips), 64 (four trips); 12, 100 and 260 leave lanes idle
V4_WIDTHS = (4, 8, 12, 16, 32, 64, 100, 128, 256, 260, 1024)
SCALAR_WIDTHS = (1, 2, 3, 5, 9, 17, 33, 63, 65, 130)      # one-element form, T = 1 ... 64; 65 and 130: two and three trips
MISALIGNED_WIDTHS = (64, 256)                             # one-element form at T = 64 with one and four trips
SHAPE_4D = (5, 3, 4, 4)
GRAD_WIDTHS = (5, 64)
GRAD_ROWS = 33
KINK_MARGIN = 0.01


def lane_group(m, vector):
    """T of the launch ``fc_elementwise`` chooses for rows of ``m`` floats (16-byte form or one-element form)."""
    t, units = 1, (m // 4 if vector else m)
    while t < units and t < 64:
        t <<= 1
    return t


def rows_for(m, vector):
    """Three full blocks of 256 / T rows and one more row."""
    return 3 * (256 // lane_group(m, vector)) + 1


def _f32(v):
    return float(np.float32(v))


def _around(v):
    """``v`` as float32 and its two float32 neighbours."""
    v = np.float32(v)
    return [float(np.nextafter(v, np.float32(-np.inf))), float(v), float(np.nextafter(v, np.float32(np.inf)))]


def _pm(values):
    return [s * v for v in values for s in (1.0, -1.0)]


def _esp(m):
    """ExtendedSoftplus over ``m`` features, raw shift cycling through -3, 0, 3, 10."""
    return T.ExtendedSoftplus(features=m, shift=[[(-3.0, 0.0, 3.0, 10.0)[j % 4] for j in range(m)]])


def _softplus_images(t, xs):
    """Float64 forward images of ``xs`` whose softplus part is >= 1e-6 (below, y - eps cancels to 0 in float32 and the
    reference's own log(expm1(0)) is -inf)."""
    sp = F.softplus(torch.tensor(xs, dtype=torch.float64), beta=1, threshold=t.softplus.threshold)
    return [float(v) + t.eps for v in sp if float(v) >= 1e-6]


def _sigmoid_forward_edges(t):
    """temperature * x at +-20 (where softplus becomes linear), its float32 neighbours, and at +-30."""
    temperature = float(t.temperature.detach())
    return _pm(_around(20.0 / temperature) + [30.0 / temperature])


def _softplus_forward_edges(t):
    return [-30.0, -1e-3, 0.0] + _around(t.softplus.threshold) + [50.0]


# name -> dict(variants=[(label, build(m) -> module)], parameter=attribute name or None, context=bool,
#              forward / inverse = (bulk(generator, shape, module) -> float32 tensor, edges(module) -> floats,
#                                   kinks(module) -> points the gradient inputs stay KINK_MARGIN away from))
def _randn(scale):
    return lambda g, shape, t: torch.randn(shape, generator=g) * scale


def _rand(lo, hi):
    return lambda g, shape, t: torch.rand(shape, generator=g) * (hi - lo) + lo


def _none(t):
    return []


BIJECTORS = {
    "exp": dict(
        variants=[("", lambda m: T.Exp())],
        forward=(_randn(1.5), lambda t: [-87.0, -1e-3, 0.0, 1e-3, 80.0], _none),
        inverse=(lambda g, shape, t: torch.exp(torch.randn(shape, generator=g) * 1.5), lambda t: [1e-20, 1e-3, 1.0, 1e20],
                 _none)),
    "tanh": dict(
        variants=[("", lambda m: T.Tanh())],
        forward=(_randn(1.5), lambda t: [0.0] + _pm([1e-6, 1e-3, 0.5, 4.0, 8.5]), _none),
        inverse=(_rand(-0.9, 0.9), lambda t: [0.0] + _pm([1e-6, 0.5, 0.999, 1.0 - 2.0 ** -20]), _none)),
    "logtanh": dict(
        variants=[("cut%g" % c, lambda m, c=c: T.LogTanh(cut_point=c)) for c in (0.3, 1, 2.5)],
        forward=(_randn(2.0), lambda t: _pm(_around(t.cut_point) + [1e-3, 50.0, 1e4]), lambda t: _pm([t.cut_point])),
        inverse=(_rand(-1.2, 1.2), lambda t: _pm(_around(t.inv_cut_point) + [3.0]), lambda t: _pm([t.inv_cut_point]))),
    "leaky_relu": dict(
        variants=[("slope%g" % s, lambda m, s=s: T.LeakyReLU(negative_slope=s)) for s in (0.01, 0.1, 2.5)],
        parameter="log_negative_slope",
        forward=(_randn(1.0), lambda t: [-0.0, 0.0] + _pm([1e-30, 1e3]), lambda t: [0.0]),
        inverse=(_randn(1.0), lambda t: [-0.0, 0.0] + _pm([1e-30, 1e3]), lambda t: [0.0])),
    "sigmoid": dict(
        variants=[("temp%g" % v, lambda m, v=v: T.Sigmoid(temperature=v, learn_temperature=True))
                  for v in (0.3, 1, 1.7, 5)],
        parameter="temperature",
        forward=(_randn(2.0), lambda t: _sigmoid_forward_edges(t), _none),
        inverse=(_rand(0.0, 1.0), lambda t: [0.0, t.eps / 2, t.eps, 1e-3, 0.5, 1 - 1e-3, 1 - t.eps, 1.0],
                 lambda t: [t.eps, 1 - t.eps])),
    "logit": dict(                                      # InverseTransform(Sigmoid): the same kernel through the module
        variants=[("temp%g" % v, lambda m, v=v: T.Logit(temperature=v)) for v in (0.3, 1, 1.7, 5)],
        forward=(_rand(0.0, 1.0), lambda t: [0.0, t._transform.eps / 2, t._transform.eps, 1e-3, 0.5, 1 - 1e-3,
                                             1 - t._transform.eps, 1.0],
                 lambda t: [t._transform.eps, 1 - t._transform.eps]),
        inverse=(_randn(2.0), lambda t: _sigmoid_forward_edges(t._transform), _none)),
    "softplus": dict(
        variants=[("thr%g_eps%g" % (thr, eps), lambda m, thr=thr, eps=eps: T.Softplus(threshold=thr, eps=eps))
                  for thr, eps in ((20, 0.0), (20, 1e-3), (5, 0.0))],
        forward=(_randn(3.0), _softplus_forward_edges, _none),
        inverse=(lambda g, shape, t: (F.softplus((torch.randn(shape, generator=g) * 2.5).clamp_min(-8.0).double(), beta=1,
                                                 threshold=t.softplus.threshold) + t.eps).float(),
                 lambda t: _softplus_images(t, _softplus_forward_edges(t)), _none)),
    "cauchy_cdf": dict(
        variants=[("", lambda m: T.CauchyCDF())],
        forward=(_randn(3.0), lambda t: [0.0] + _pm([1e-3, 1.0, 1e3, 1e6]), _none),
        inverse=(_rand(0.01, 0.99), lambda t: [0.0, 1e-4, 0.5, 1 - 1e-4, 1.0], _none)),
    "extended_softplus": dict(
        variants=[("", _esp)],
        parameter="shift",
        forward=(_randn(4.0), lambda t: _pm([0.0, 1.0, 10.0, 30.0, 100.0]), _none)),
    "glu": dict(
        variants=[("", lambda m: T.GatedLinearUnit())],
        parameter="context", context=True,
        forward=(_randn(1.0), _none, _none),
        inverse=(_randn(1.0), _none, _none)),
}
GLU_CONTEXT_EDGES = _pm([0.0, 5.0, 20.0, 30.0])

CASES = [(name, direction) for name, spec in BIJECTORS.items() for direction in ("forward", "inverse") if direction in spec]
PER_ELEMENT = ("extended_softplus", "glu")      # these return the log-derivative per element, not summed over the row


def variants(name, m):
    """[(label, float32 CPU module)] of bijector ``name`` for rows of ``m`` elements."""
    return [(label, build(m)) for label, build in BIJECTORS[name]["variants"]]


def _write_edges(x, edges):
    """Edge values over every third element from the front and from the back of ``x`` (in place); the mask of the
    positions written."""
    flat = x.reshape(-1)
    mask = torch.zeros(flat.numel(), dtype=torch.bool)
    for k, v in enumerate(edges):
        for pos in (3 * k, flat.numel() - 1 - 3 * k):
            if 0 <= pos < flat.numel() and not mask[pos]:
                flat[pos] = v
                mask[pos] = True
    return mask.reshape(x.shape)


def make_inputs(name, direction, module, shape, seed=0, edges=True):
    """``(inputs, context or None, edge mask)`` in float32 on the CPU: the bulk of the right domain with the edge values
    written in; the mask marks the elements that hold an edge value (in the inputs or in the context)."""
    spec = BIJECTORS[name]
    bulk, edge_values, _ = spec[direction]
    g = torch.Generator().manual_seed(1000 * seed + 17 * len(name) + (direction == "inverse"))
    x = bulk(g, shape, module).contiguous()
    mask = torch.zeros(shape, dtype=torch.bool)
    if edges:
        mask |= _write_edges(x, [_f32(v) for v in edge_values(module)])
    context = None
    if spec.get("context"):
        context = (torch.randn(shape, generator=g) * 3.0).contiguous()
        if edges:
            mask |= _write_edges(context, GLU_CONTEXT_EDGES)
    return x, context, mask


def make_grad_inputs(name, direction, module, shape, seed=0):
    """Inputs for the gradient checks: the bulk alone, moved out of the KINK_MARGIN neighbourhood of every point where the
    second derivative jumps; Tanh forward also holds |x| = 6 and 8.5."""
    spec = BIJECTORS[name]
    bulk, _, kinks = spec[direction]
    g = torch.Generator().manual_seed(5000 + 1000 * seed + 17 * len(name) + (direction == "inverse"))
    x = bulk(g, shape, module).contiguous()
    lo, hi = float(x.min()), float(x.max())
    for k in kinks(module):
        away = torch.where(x >= k, torch.full_like(x, k + 2.0 * KINK_MARGIN), torch.full_like(x, k - 2.0 * KINK_MARGIN))
        away = torch.where((away < lo) | (away > hi), 2.0 * k - away, away)      # (stay inside the bulk's range)
        x = torch.where((x - k).abs() < KINK_MARGIN, away, x)
    if name == "tanh" and direction == "forward":
        _write_edges(x, _pm([6.0, 8.5]))
    context = (torch.randn(shape, generator=g) * 3.0).contiguous() if spec.get("context") else None
    return x, context


def oracle(name, module, x, context=None, inverse=False):
    """``(outputs, logabsdet)`` of the CPU oracle in the dtype of ``module`` / ``x``: logabsdet summed over all item dims
    ([N]), per element for ExtendedSoftplus ([N, ...]) and GatedLinearUnit ([N * m])."""
    if name == "extended_softplus":
        shift = O._p(module.shift).reshape((1,) + tuple(x.shape[1:]))
        return O.extended_softplus(x, shift)
    y, lad = O.transform_apply(module, x, context, inverse)
    if name != "glu" and lad.dim() > 1:       # (the reference's Softplus sums over the last dim only)
        lad = lad.reshape(lad.shape[0], -1).sum(dim=1)
    return y, lad


def references(name, module, x, context=None, inverse=False):
    """``(y64, lad64, floor_y, floor_lad, y32, lad32)``: the float64 truth, the float32 oracle and its noise floors."""
    with torch.no_grad():
        y32, lad32 = oracle(name, module, x.clone(), None if context is None else context.clone(), inverse)
        y64, lad64 = oracle(name, copy.deepcopy(module).double(), x.double(),
                            None if context is None else context.double(), inverse)
    return y64, lad64, maxabs(y32.double() - y64), maxabs(lad32.double() - lad64), y32, lad32


def maxabs(t):
    return float(t.abs().max()) if t.numel() else 0.0


def bound(truth, floor):
    """The project's bound against float64 (``test_gpu_golden._check``)."""
    return 1e-5 * max(1.0, maxabs(truth)) + 4.0 * floor


def expression_args(name, module, context, inverse):
    """``(kind, inverse, aux, p)`` as the module hands them to ``ops.elementwise_autograd``."""
    if name == "logit":
        name, module, inverse = "sigmoid", module._transform, not inverse
    if name == "exp":
        return ops.EW_EXP, inverse, None, ()
    if name == "tanh":
        return ops.EW_TANH, inverse, None, ()
    if name == "logtanh":
        return ops.EW_LOGTANH, inverse, None, module._p()
    if name == "leaky_relu":
        return ops.EW_LEAKY_RELU, inverse, module.log_negative_slope.reshape(1), module._p()
    if name == "sigmoid":
        return ops.EW_SIGMOID, inverse, module.temperature, (module.eps,)
    if name == "softplus":
        return ops.EW_SOFTPLUS, inverse, None, (module.softplus.threshold, module.eps)
    if name == "cauchy_cdf":
        return ops.EW_CAUCHY_CDF, inverse, None, ()
    if name == "extended_softplus":
        return ops.EW_EXTENDED_SOFTPLUS, False, module.shift.reshape(-1), ()
    assert name == "glu", name
    return ops.EW_GLU, inverse, context, ()


def parameter_of(name, module, context):
    """The tensor the bijector learns (temperature, log-slope, shift, context), or None."""
    attribute = BIJECTORS[name].get("parameter")
    if attribute is None:
        return None
    return context if attribute == "context" else getattr(module, attribute)


def oracle_gradients(name, module, x, context, inverse, gy, gl):
    """Float64 gradients of ``(y * gy).sum() + (lad * gl).sum()`` w.r.t. the inputs and the parameter (or None) by
    ``torch.autograd`` on the oracle; also ``(y64, lad64)``."""
    m64 = copy.deepcopy(module).double()
    x64 = x.double().requires_grad_(True)
    c64 = None if context is None else context.double().requires_grad_(True)
    with O.differentiable_parameters():
        y, lad = oracle(name, m64, x64, c64, inverse)
    parameter = parameter_of(name, m64, c64)
    loss = (y * gy.double()).sum() + (lad * gl.double().reshape(lad.shape)).sum()
    wanted = [x64] + ([] if parameter is None else [parameter])
    grads = torch.autograd.grad(loss, wanted, allow_unused=True)
    return grads[0], (grads[1] if parameter is not None else None), y.detach(), lad.detach()


def relerr(got, truth):
    """The project's gradient rule (tests/test_gpu_fused_backward.py): max |g - g64| / max |g64|."""
    got, truth = got.detach().double().cpu(), truth.detach().double().cpu()
    return float((got - truth).abs().max() / truth.abs().max().clamp_min(1e-30))

