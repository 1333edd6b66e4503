"""Continuous normalizing flows (eval mode): one ODE-function evaluation, or a whole fixed-step solve, per launch."""
import ctypes

import torch

from flowconductor_amd import _hip
from ._core import _call, _prep_2d


CNF_MAX_DIM = 16
CNF_MAX_HIDDEN_LAYERS = 4
CNF_MAX_WIDTH = 64
CNF_LAYER_IGNORE, CNF_LAYER_CONCAT, CNF_LAYER_CONCAT_V2, CNF_LAYER_SQUASH, CNF_LAYER_CONCATSQUASH = 0, 1, 2, 3, 4
CNF_ACT_TANH, CNF_ACT_RELU, CNF_ACT_SOFTPLUS, CNF_ACT_ELU, CNF_ACT_SWISH, CNF_ACT_SQUARE, CNF_ACT_IDENTITY = range(7)
CNF_EULER, CNF_MIDPOINT, CNF_RK4 = 0, 1, 2
CNF_METHODS = {"euler": CNF_EULER, "midpoint": CNF_MIDPOINT, "rk4": CNF_RK4}
CNF_STAGES = {CNF_EULER: 1, CNF_MIDPOINT: 2, CNF_RK4: 4}


# A row occupies a group of lanes (the smallest power of two >= d + 1) and the kernels' time grows with the lanes of a
# batch, while the torch composition stays launch-bound up to far larger batches: the dispatch takes the kernels up to
# this many lanes, the largest size at which they measured faster (tools/probe/bench_cnf.py).
CNF_KERNEL_MAX_LANES = 1 << 16


def cnf_group_lanes(d):
    """Lanes that carry one row of ``d`` features."""
    lanes = 2
    while lanes < d + 1:
        lanes *= 2
    return lanes


def cnf_rows_pay(n, d):
    """Whether the dispatch sends a batch of ``n`` rows of ``d`` features to the kernels."""
    return n * cnf_group_lanes(d) <= CNF_KERNEL_MAX_LANES


def _cnf_pad4(v):
    return (v + 3) & ~3


def cnf_supported(d, hidden):
    """Whether ``fc_cnf_field`` / ``fc_cnf_integrate`` take a net ``d -> hidden... -> d``."""
    return (1 <= d <= CNF_MAX_DIM and len(hidden) <= CNF_MAX_HIDDEN_LAYERS
            and all(1 <= int(h) <= CNF_MAX_WIDTH for h in hidden))


def cnf_image_floats(d, hidden):
    """Length of the packed net image (the layout is described in include/flowcon_hip.h)."""
    widths = (d,) + tuple(int(h) for h in hidden) + (d,)
    return sum((5 + widths[l]) * _cnf_pad4(widths[l + 1]) for l in range(len(widths) - 1))


def _cnf_operands(rows, image, d, hidden, layer_kind, activation, evals):
    y = _prep_2d(rows)
    if y.shape[1] != d:
        raise ValueError("flowconductor_amd: rows of %d features for a net of dimension %d" % (y.shape[1], d))
    hidden = tuple(int(h) for h in hidden)
    if not cnf_supported(d, hidden):
        raise ValueError("flowconductor_amd: the CNF kernels take d <= %d and at most %d hidden layers of at most %d units"
                         % (CNF_MAX_DIM, CNF_MAX_HIDDEN_LAYERS, CNF_MAX_WIDTH))
    if not (CNF_LAYER_IGNORE <= layer_kind <= CNF_LAYER_CONCATSQUASH and CNF_ACT_TANH <= activation <= CNF_ACT_IDENTITY):
        raise ValueError("flowconductor_amd: unknown CNF layer kind %r or activation %r" % (layer_kind, activation))
    image = _hip.dev_f32(image, "image")
    if image.numel() != cnf_image_floats(d, hidden):
        raise ValueError("flowconductor_amd: net image of %d floats, expected %d"
                         % (image.numel(), cnf_image_floats(d, hidden)))
    if image.device != y.device:
        raise RuntimeError("flowconductor_amd: image on %s, rows on %s" % (image.device, y.device))
    if evals is not None and (evals.dtype != torch.float32 or evals.device != y.device or evals.numel() != 1):
        raise ValueError("flowconductor_amd: evals must be one float32 word on the device of the rows")
    widths = (ctypes.c_int32 * max(1, len(hidden)))(*hidden)
    return y, image, hidden, widths


def cnf_field(t, inputs, image, d, hidden, layer_kind, activation, residual=False, scale_output=1.0, p0=1.0,
              evals=None):
    """``(dy [N, d], -div [N])`` of the ODE function at time ``t`` (a number, or a one-element float32 tensor on the
    rows' device, which the kernel reads itself), one launch.  ``evals``: a float32 device word that is incremented.
    No autograd."""
    _hip.require_no_grad(inputs)
    lib = _hip.load()
    y, image, hidden, widths = _cnf_operands(inputs, image, d, hidden, layer_kind, activation, evals)
    t_host, t_dev = 0.0, None
    if isinstance(t, torch.Tensor):
        if t.numel() != 1 or t.dtype != torch.float32 or t.device != y.device:
            raise ValueError("flowconductor_amd: t must be a number or one float32 element on the device of the rows")
        t_dev = t
    else:
        t_host = float(t)
    n = y.shape[0]
    dy = torch.empty_like(y)
    negdiv = torch.empty(n, dtype=torch.float32, device=y.device)
    _call("fc_cnf_field", lib.fc_cnf_field, y.device, _hip.ptr(y), _hip.ptr(image), _hip.ptr(dy), _hip.ptr(negdiv),
          _hip.ptr(evals), n, d, len(hidden) + 1, widths, layer_kind, activation, int(bool(residual)),
          float(scale_output), float(p0), image.numel(), t_host, _hip.ptr(t_dev), _hip.stream_ptr(y.device))
    return dy, negdiv


def cnf_integrate(inputs, logp, image, d, hidden, layer_kind, activation, t0, t1, steps, method, residual=False,
                  scale_output=1.0, p0=1.0, evals=None):
    """``(z(t1) [N, d], logp(t1) [N])`` from ``z(t0) = inputs`` and ``logp(t0) = logp`` (None: zeros) in ``steps`` equal
    steps of ``method`` (``CNF_EULER`` / ``CNF_MIDPOINT`` / ``CNF_RK4``, the classical tableau), every row on its own,
    one launch, no host sync.  ``evals``: a float32 device word the launch max-reduces ``steps * stages`` into."""
    _hip.require_no_grad(inputs, logp)
    lib = _hip.load()
    z, image, hidden, widths = _cnf_operands(inputs, image, d, hidden, layer_kind, activation, evals)
    n = z.shape[0]
    if method not in CNF_STAGES or int(steps) < 1:
        raise ValueError("flowconductor_amd: fc_cnf_integrate takes euler / midpoint / rk4 and at least one step")
    if logp is not None:
        logp = _hip.dev_f32(logp, "logp")
        if logp.numel() != n or logp.device != z.device:
            raise ValueError("flowconductor_amd: logp of %d entries for %d rows" % (logp.numel(), n))
    z_out = torch.empty_like(z)
    logp_out = torch.empty(n, dtype=torch.float32, device=z.device)
    _call("fc_cnf_integrate", lib.fc_cnf_integrate, z.device, _hip.ptr(z), _hip.ptr(logp), _hip.ptr(image),
          _hip.ptr(z_out), _hip.ptr(logp_out), _hip.ptr(evals), n, d, len(hidden) + 1, widths, layer_kind, activation,
          int(bool(residual)), float(scale_output), float(p0), image.numel(), float(t0), float(t1), int(steps),
          int(method), _hip.stream_ptr(z.device))
    return z_out, logp_out
