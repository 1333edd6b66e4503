"""Continuous normalizing flows: one ODE-function evaluation, or a whole fixed-step solve, per launch (eval mode), and
one evaluation, or a whole fixed-step solve, as an autograd node of one forward and one backward launch (training)."""
import ctypes

import torch

from flowconductor_amd import _hip
from ._core import _call, _prep_2d, once_differentiable


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


def _cnf_net(d, hidden):
    """``(d, layers, hidden widths as an int32 array)``, as every C entry point takes a net."""
    hidden = tuple(int(h) for h in hidden)
    return d, len(hidden) + 1, (ctypes.c_int32 * max(1, len(hidden)))(*hidden)


def _cnf_operands(rows, image, d, hidden, layer_kind, activation, residual, scale_output, p0, evals):
    """The checked rows and image, and the ten arguments from ``n`` to the image length that follow the pointers in
    every launching entry point."""
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
    tail = (y.shape[0],) + _cnf_net(d, hidden) + (layer_kind, activation, int(bool(residual)), float(scale_output),
                                                  float(p0), image.numel())
    return y, image, tail


def _cnf_outputs(y):
    """``(out [N, d], out1 [N])`` for the rows ``y``."""
    return torch.empty_like(y), torch.empty(y.shape[0], dtype=torch.float32, device=y.device)


def _cnf_time(t, y):
    if isinstance(t, torch.Tensor):
        if t.numel() != 1 or t.dtype != torch.float32 or t.device != y.device:
            raise ValueError("flowconductor_amd: t must be a number or one float32 element on the device of the rows")
        return 0.0, t
    return float(t), None


def _cnf_logp(logp, z):
    if logp is None:
        return None
    logp = _hip.dev_f32(logp, "logp")
    if logp.numel() != z.shape[0] or logp.device != z.device:
        raise ValueError("flowconductor_amd: logp of %d entries for %d rows" % (logp.numel(), z.shape[0]))
    return logp


def cnf_field(t, inputs, image, d, hidden, layer_kind, activation, residual=False, scale_output=1.0, p0=1.0,
              evals=None):
    """``(dy [N, d], -div [N])`` of the ODE function at time ``t`` (a number, or a one-element float32 tensor on the
    rows' device, which the kernel reads itself), one launch.  ``evals``: a float32 device word that is incremented.
    No autograd."""
    _hip.require_no_grad(inputs)
    lib = _hip.load()
    y, image, tail = _cnf_operands(inputs, image, d, hidden, layer_kind, activation, residual, scale_output, p0, evals)
    t_host, t_dev = _cnf_time(t, y)
    dy, negdiv = _cnf_outputs(y)
    _call("fc_cnf_field", lib.fc_cnf_field, y.device, _hip.ptr(y), _hip.ptr(image), _hip.ptr(dy), _hip.ptr(negdiv),
          _hip.ptr(evals), *tail, t_host, _hip.ptr(t_dev), _hip.stream_ptr(y.device))
    return dy, negdiv


def cnf_integrate(inputs, logp, image, d, hidden, layer_kind, activation, t0, t1, steps, method, residual=False,
                  scale_output=1.0, p0=1.0, evals=None):
    """``(z(t1) [N, d], logp(t1) [N])`` from ``z(t0) = inputs`` and ``logp(t0) = logp`` (None: zeros) in ``steps`` equal
    steps of ``method`` (``CNF_EULER`` / ``CNF_MIDPOINT`` / ``CNF_RK4``, the classical tableau), every row on its own,
    one launch, no host sync.  ``evals``: a float32 device word the launch max-reduces ``steps * stages`` into."""
    _hip.require_no_grad(inputs, logp)
    lib = _hip.load()
    z, image, tail = _cnf_operands(inputs, image, d, hidden, layer_kind, activation, residual, scale_output, p0, evals)
    if method not in CNF_STAGES or int(steps) < 1:
        raise ValueError("flowconductor_amd: fc_cnf_integrate takes euler / midpoint / rk4 and at least one step")
    logp = _cnf_logp(logp, z)
    z_out, logp_out = _cnf_outputs(z)
    _call("fc_cnf_integrate", lib.fc_cnf_integrate, z.device, _hip.ptr(z), _hip.ptr(logp), _hip.ptr(image),
          _hip.ptr(z_out), _hip.ptr(logp_out), _hip.ptr(evals), *tail, float(t0), float(t1), int(steps), int(method),
          _hip.stream_ptr(z.device))
    return z_out, logp_out


# ---- the adaptive solve: fc_cnf_dopri5 -------------------------------------------------------------------------------
CNF_DOPRI5_MAX_ATTEMPTS = 4096
# A stage state enters the net rounded to float32 (6e-8 relative): below this tolerance that rounding is of the size of
# the error the step controller is asked to resolve, and the call keeps the float32 host loop it had.
CNF_DOPRI5_MIN_TOL = 1e-6
# The dispatch (options ``cnf_dopri5_kernel=True``) takes the one-launch solve up to this many lanes ``N * G``: the
# largest power of two at which it measured faster than both the host loop over ``fc_cnf_field`` and the torch
# composition on both nets of tools/probe/bench_cnf_dopri5.py by more than the spread of the rounds (DESIGN.md,
# "dopri5 in one launch": at 2^17 lanes it was still ahead, within the composition's spread).  It is
# ``CNF_KERNEL_MAX_LANES`` as well, up to which ``ODEfunc`` takes the kernels at all.
CNF_DOPRI5_MAX_LANES = 1 << 16


def cnf_dopri5_fits(d, hidden, atol, rtol):
    """Whether ``fc_cnf_dopri5`` takes a net ``d -> hidden... -> d`` at these tolerances: the limits of the other CNF
    kernels, and both tolerances at least ``CNF_DOPRI5_MIN_TOL``."""
    return cnf_supported(d, hidden) and float(atol) >= CNF_DOPRI5_MIN_TOL and float(rtol) >= CNF_DOPRI5_MIN_TOL


def cnf_dopri5_rows_pay(n, d):
    """Whether ``cnf_dopri5_kernel=True`` sends a batch of ``n`` rows of ``d`` features to the one-launch solve."""
    return n * cnf_group_lanes(d) <= CNF_DOPRI5_MAX_LANES


def cnf_dopri5_attempts(max_num_steps):
    """``max_attempts`` of the kernel for the solver option ``max_num_steps`` (None: not set): clipped to
    ``CNF_DOPRI5_MAX_ATTEMPTS``; None for a bound below 1, which only the host loop can answer (it raises)."""
    if max_num_steps is None:
        return CNF_DOPRI5_MAX_ATTEMPTS
    limit = int(max_num_steps)
    return None if limit < 1 else min(limit, CNF_DOPRI5_MAX_ATTEMPTS)


def cnf_dopri5(inputs, logp, image, d, hidden, layer_kind, activation, t0, t1, atol, rtol, first_step=None,
               max_attempts=CNF_DOPRI5_MAX_ATTEMPTS, residual=False, scale_output=1.0, p0=1.0, evals=None):
    """``(z(t1) [N, d], logp(t1) [N], attempts [N] int32)`` from ``z(t0) = inputs`` and ``logp(t0) = logp`` (None:
    zeros) with the Dormand-Prince 5(4) pair, one launch, no host sync.  Every row on its own: its own time, step size,
    decisions and attempt count, judged by the RMS of its own ``d + 1`` scaled errors.  ``first_step`` (> 0) replaces
    the initial-step heuristic.  A row that has made ``max_attempts`` attempts without reaching ``t1``, or whose error
    estimate is not finite, or whose step no longer moves ``t``, returns NaN (the host loop raises instead).
    ``evals``: a float32 device word the launch max-reduces ``2 + 6 * attempts`` into (``1 + ...`` with
    ``first_step``)."""
    _hip.require_no_grad(inputs, logp)
    lib = _hip.load()
    z, image, tail = _cnf_operands(inputs, image, d, hidden, layer_kind, activation, residual, scale_output, p0, evals)
    if not 1 <= int(max_attempts) <= CNF_DOPRI5_MAX_ATTEMPTS:
        raise ValueError("flowconductor_amd: fc_cnf_dopri5 takes max_attempts in 1 .. %d" % CNF_DOPRI5_MAX_ATTEMPTS)
    atol, rtol = float(atol), float(rtol)
    if not (atol >= 0.0 and rtol >= 0.0 and atol + rtol > 0.0):
        raise ValueError("flowconductor_amd: fc_cnf_dopri5 takes atol, rtol >= 0, not both 0")
    step = 0.0 if first_step is None else float(first_step)
    if first_step is not None and not 0.0 < step < float("inf"):
        raise ValueError("flowconductor_amd: fc_cnf_dopri5 takes a positive finite first_step")
    logp = _cnf_logp(logp, z)
    z_out, logp_out = _cnf_outputs(z)
    attempts = torch.empty(z.shape[0], dtype=torch.int32, device=z.device)
    _call("fc_cnf_dopri5", lib.fc_cnf_dopri5, z.device, _hip.ptr(z), _hip.ptr(logp), _hip.ptr(image), _hip.ptr(z_out),
          _hip.ptr(logp_out), _hip.ptr(attempts), _hip.ptr(evals), *tail, float(t0), float(t1), atol, rtol, step,
          int(max_attempts), _hip.stream_ptr(z.device))
    return z_out, logp_out, attempts


# ---- training: fc_cnf_field_train / fc_cnf_field_backward ------------------------------------------------------------
CNF_TRAIN_MAX_HIDDEN_LAYERS = 3
CNF_BACKWARD_MAX_BLOCKS = 256      # the backward launch's grid cap: beyond it a block walks over several row tiles
CNF_DOUBLE_BACKWARD_MSG = (
    "flowconductor_amd: the CNF kernel route (options 'cnf_training') is once differentiable; for a gradient of a "
    "gradient (create_graph=True, the regularisers) run the solve with options.override(cnf_training=False), the torch "
    "composition")

# A row occupies 2 lanes under Hutchinson's estimator (the value stream and one tangent) and ``cnf_group_lanes(d)`` with
# the exact divergence.  The dispatch takes the training kernels up to this many lanes: the largest measured size at
# which a training step beat the composition in BOTH divergence modes (tools/probe/bench_cnf_training.py; DESIGN.md,
# "CNF training": every measured shape up to 2^14 lanes won, 1.8x to 2.8x; at 2^15 lanes D = 16 under Hutchinson lost).
CNF_TRAIN_MAX_LANES = 1 << 14


def cnf_train_supported(d, hidden):
    """Whether ``fc_cnf_field_train`` / ``fc_cnf_field_backward`` take a net ``d -> hidden... -> d``: the forward
    kernels' limits with at most three hidden layers (the backward keeps every layer's input of a lane in LDS)."""
    return cnf_supported(d, hidden) and len(hidden) <= CNF_TRAIN_MAX_HIDDEN_LAYERS


def cnf_train_lanes(n, d, hutchinson):
    """Lanes ``n`` rows of ``d`` features occupy in the training kernels."""
    return n * (2 if hutchinson else cnf_group_lanes(d))


def cnf_train_rows_pay(n, d, hutchinson):
    """Whether ``cnf_training=True`` sends a batch of ``n`` rows to the training kernels."""
    return cnf_train_lanes(n, d, hutchinson) <= CNF_TRAIN_MAX_LANES


def _cnf_train_operands(rows, e, image, d, hidden, layer_kind, activation, residual, scale_output, p0, evals):
    y, image, tail = _cnf_operands(rows, image, d, hidden, layer_kind, activation, residual, scale_output, p0, evals)
    if not cnf_train_supported(d, hidden):
        raise ValueError("flowconductor_amd: the CNF training kernels take at most %d hidden layers"
                         % CNF_TRAIN_MAX_HIDDEN_LAYERS)
    if e is not None:
        if not (isinstance(e, torch.Tensor) and e.dtype == torch.float32 and e.device == y.device
                and e.shape == y.shape and e.is_contiguous()):
            raise ValueError("flowconductor_amd: e must be contiguous float32 [N, D] on the device of the rows")
    return y, image, tail


def cnf_backward_rows(d, hidden, hutchinson):
    """Rows one block of ``fc_cnf_field_backward`` carries (its sums over rows are per block, then over blocks)."""
    rows = _hip.load().fc_cnf_field_backward_rows(*_cnf_net(d, hidden), int(bool(hutchinson)))
    if rows < 1:
        raise ValueError("flowconductor_amd: cnf_backward_rows: outside the kernel's limits")
    return rows


def cnf_field_train(t, inputs, e, image, d, hidden, layer_kind, activation, residual=False, scale_output=1.0, p0=1.0,
                    evals=None):
    """``(dy [N, d], -div [N])`` as ``cnf_field``, one launch: with ``e`` (float32 ``[N, d]``) the divergence is
    Hutchinson's estimate ``e^T (df/dy) e``, with None the exact one.  No autograd (``_CnfFieldFunction`` has it)."""
    _hip.require_no_grad(inputs)
    lib = _hip.load()
    y, image, tail = _cnf_train_operands(inputs, e, image, d, hidden, layer_kind, activation, residual, scale_output,
                                         p0, evals)
    t_host, t_dev = _cnf_time(t, y)
    dy, negdiv = _cnf_outputs(y)
    _call("fc_cnf_field_train", lib.fc_cnf_field_train, y.device, _hip.ptr(y), _hip.ptr(e), _hip.ptr(image), _hip.ptr(dy),
          _hip.ptr(negdiv), _hip.ptr(evals), *tail, t_host, _hip.ptr(t_dev), _hip.stream_ptr(y.device))
    return dy, negdiv


def cnf_field_backward(t, inputs, e, image, g_dy, g_negdiv, d, hidden, layer_kind, activation, residual=False,
                       scale_output=1.0, p0=1.0):
    """The raw ``fc_cnf_field_backward``: ``(g_y [N, d], g_image [image floats])`` of ``sum(g_dy * dy) + sum(g_negdiv *
    negdiv)`` for the outputs of ``cnf_field_train`` at the same arguments; ``g_image`` in the image's layout, summed
    over the rows in a fixed order (bitwise reproducible)."""
    lib = _hip.load()
    y, image, tail = _cnf_train_operands(inputs, e, image, d, hidden, layer_kind, activation, residual, scale_output,
                                         p0, None)
    t_host, t_dev = _cnf_time(t, y)
    n = y.shape[0]
    g_dy = _hip.dev_f32(g_dy, "g_dy")
    g_negdiv = _hip.dev_f32(g_negdiv, "g_negdiv")
    if g_dy.shape != y.shape or g_negdiv.numel() != n or g_dy.device != y.device or g_negdiv.device != y.device:
        raise ValueError("flowconductor_amd: cnf_field_backward: g_dy / g_negdiv do not belong to the rows")
    with torch.cuda.device(y.device):
        floats = lib.fc_cnf_field_backward_workspace(*tail[:4], int(e is not None))
    if floats < 0:
        raise ValueError("flowconductor_amd: cnf_field_backward: outside the kernel's limits")
    workspace = torch.empty(max(floats // 2, 1), dtype=torch.float64, device=y.device)
    g_y = torch.empty_like(y)
    g_image = torch.empty_like(image)
    _call("fc_cnf_field_backward", lib.fc_cnf_field_backward, y.device, _hip.ptr(y), _hip.ptr(e), _hip.ptr(image),
          _hip.ptr(g_dy), _hip.ptr(g_negdiv), _hip.ptr(g_y), _hip.ptr(g_image), _hip.ptr(workspace), *tail, t_host,
          _hip.ptr(t_dev), _hip.stream_ptr(y.device))
    return g_y, g_image


class _CnfFieldFunction(torch.autograd.Function):
    """``fc_cnf_field_train`` with ``fc_cnf_field_backward`` over ``(y, image)``: saves the inputs alone, the backward
    recomputes the forward in its kernel.  ``e`` and ``t`` get no gradient.  Once differentiable."""

    @staticmethod
    def forward(ctx, y, image, e, t, kw):
        dy, negdiv = cnf_field_train(t, y, e, image=image, **kw)
        ctx.kw = {k: v for k, v in kw.items() if k != "evals"}
        ctx.t = t
        ctx.save_for_backward(_prep_2d(y), image, e)
        return dy, negdiv

    @staticmethod
    @once_differentiable(CNF_DOUBLE_BACKWARD_MSG)
    def backward(ctx, g_dy, g_negdiv):
        y, image, e = ctx.saved_tensors
        g_y, g_image = cnf_field_backward(ctx.t, y, e, image, g_dy.contiguous(), g_negdiv.contiguous(), **ctx.kw)
        need = ctx.needs_input_grad
        return g_y if need[0] else None, g_image if need[1] else None, None, None, None


# ---- training: the whole fixed-step solve, fc_cnf_integrate_train / fc_cnf_integrate_backward ------------------------
# The tape of a solve is ``steps * stages * N * D`` floats.  A call whose tape would be larger than this keeps the
# per-evaluation route: a condition that keeps a long solve from allocating without bound, not a tuned number.
CNF_SOLVE_TRAIN_MAX_TAPE_BYTES = 1 << 30
CNF_SOLVE_DOUBLE_BACKWARD_MSG = (
    "flowconductor_amd: the one-launch CNF solve (options 'cnf_solve_training') is once differentiable; for a gradient "
    "of a gradient (create_graph=True, the regularisers) run the solve with "
    "options.override(cnf_solve_training=False, cnf_training=False), the torch composition")


def cnf_solve_train_fits(n, d, hidden, steps, method, hutchinson):
    """Whether ``fc_cnf_integrate_train`` / ``fc_cnf_integrate_backward`` take ``n`` rows of a net ``d -> hidden... ->
    d`` through ``steps`` steps of ``method``: ``cnf_train_supported`` (every such net fits the backward kernel's LDS in
    either divergence mode) and a tape of at most ``CNF_SOLVE_TRAIN_MAX_TAPE_BYTES``.  Allocates nothing."""
    del hutchinson      # the tape and the limits are those of both modes
    if method not in CNF_STAGES or int(steps) < 1 or int(n) < 0 or not cnf_train_supported(d, hidden):
        return False
    return 4 * int(steps) * CNF_STAGES[method] * int(n) * int(d) <= CNF_SOLVE_TRAIN_MAX_TAPE_BYTES


def cnf_solve_train_rows_pay(n, d, hutchinson):
    """Whether ``cnf_solve_training=True`` sends a batch of ``n`` rows to the one-launch solve: the limit of the
    per-evaluation nodes, whose arithmetic it shares, and the largest measured size at which it beat both other routes
    in both divergence modes (tools/probe/bench_cnf_solve_training.py; DESIGN.md, "CNF training: the whole solve")."""
    return cnf_train_lanes(n, d, hutchinson) <= CNF_TRAIN_MAX_LANES


def _cnf_fixed_steps(name, steps, method):
    if method not in CNF_STAGES or int(steps) < 1:
        raise ValueError("flowconductor_amd: %s takes euler / midpoint / rk4 and at least one step" % name)
    return int(steps), int(method)


def cnf_integrate_train(inputs, logp, e, image, d, hidden, layer_kind, activation, t0, t1, steps, method,
                        residual=False, scale_output=1.0, p0=1.0, evals=None, tape=False):
    """``cnf_integrate`` for training, one launch: with ``e`` (float32 ``[N, d]``) every evaluation's divergence is
    Hutchinson's estimate with that ``e``, with None the exact one.  ``tape=True`` returns ``(z(t1), logp(t1), tape)``,
    ``tape [steps * stages, N, d]`` the float32 stage inputs ``cnf_integrate_backward`` reads; without it ``(z(t1),
    logp(t1))``, bitwise ``cnf_integrate``'s when ``e`` is None.  No autograd (``_CnfSolveFunction`` has it)."""
    _hip.require_no_grad(inputs, logp)
    lib = _hip.load()
    z, image, tail = _cnf_train_operands(inputs, e, image, d, hidden, layer_kind, activation, residual, scale_output,
                                         p0, evals)
    steps, method = _cnf_fixed_steps("fc_cnf_integrate_train", steps, method)
    logp = _cnf_logp(logp, z)
    z_out, logp_out = _cnf_outputs(z)
    kept = None
    if tape:
        kept = torch.empty(steps * CNF_STAGES[method], z.shape[0], d, dtype=torch.float32, device=z.device)
    _call("fc_cnf_integrate_train", lib.fc_cnf_integrate_train, z.device, _hip.ptr(z), _hip.ptr(logp), _hip.ptr(e),
          _hip.ptr(image), _hip.ptr(z_out), _hip.ptr(logp_out), _hip.ptr(kept), _hip.ptr(evals), *tail, float(t0),
          float(t1), steps, method, _hip.stream_ptr(z.device))
    return (z_out, logp_out, kept) if tape else (z_out, logp_out)


def cnf_integrate_backward(tape, e, image, g_z_out, g_logp_out, d, hidden, layer_kind, activation, t0, t1, steps,
                           method, residual=False, scale_output=1.0, p0=1.0):
    """The raw ``fc_cnf_integrate_backward``: ``(g_z [N, d], g_image [image floats])`` of ``sum(g_z_out * z(t1)) +
    sum(g_logp_out * logp(t1))`` for the solve that wrote ``tape`` at the same arguments (the gradient with respect to
    ``logp(t0)`` is ``g_logp_out`` itself); ``g_image`` as ``cnf_field_backward`` gives it, bitwise reproducible."""
    lib = _hip.load()
    steps, method = _cnf_fixed_steps("fc_cnf_integrate_backward", steps, method)
    g_z_out = _hip.dev_f32(g_z_out, "g_z_out")
    z, image, tail = _cnf_train_operands(g_z_out, e, image, d, hidden, layer_kind, activation, residual, scale_output,
                                         p0, None)
    n = z.shape[0]
    g_logp_out = _hip.dev_f32(g_logp_out, "g_logp_out")
    if not (isinstance(tape, torch.Tensor) and tape.dtype == torch.float32 and tape.device == z.device
            and tape.shape == (steps * CNF_STAGES[method], n, d) and tape.is_contiguous()):
        raise ValueError("flowconductor_amd: cnf_integrate_backward: the tape must be contiguous float32 "
                         "[steps * stages, N, D] on the device of the rows")
    if g_logp_out.numel() != n or g_logp_out.device != z.device:
        raise ValueError("flowconductor_amd: cnf_integrate_backward: g_logp_out does not belong to the rows")
    with torch.cuda.device(z.device):
        floats = lib.fc_cnf_integrate_backward_workspace(*tail[:4], int(e is not None))
    if floats < 0:
        raise ValueError("flowconductor_amd: cnf_integrate_backward: outside the kernel's limits")
    workspace = torch.empty(max(floats // 2, 1), dtype=torch.float64, device=z.device)
    g_z = torch.empty_like(z)
    g_image = torch.empty_like(image)
    _call("fc_cnf_integrate_backward", lib.fc_cnf_integrate_backward, z.device, _hip.ptr(tape), _hip.ptr(e),
          _hip.ptr(image), _hip.ptr(z), _hip.ptr(g_logp_out), _hip.ptr(g_z), _hip.ptr(g_image), _hip.ptr(workspace),
          *tail, float(t0), float(t1), steps, method, _hip.stream_ptr(z.device))
    return g_z, g_image


class _CnfSolveFunction(torch.autograd.Function):
    """``fc_cnf_integrate_train`` with ``fc_cnf_integrate_backward`` over ``(z, logp, image)``: saves the tape, the
    image and ``e``; no activation is kept.  ``e`` gets no gradient.  Once differentiable."""

    @staticmethod
    def forward(ctx, z, logp, image, e, kw):
        z_t, logp_t, tape = cnf_integrate_train(z, logp, e, image=image, tape=True, **kw)
        ctx.kw = {k: v for k, v in kw.items() if k != "evals"}
        ctx.save_for_backward(tape, image, e)
        return z_t, logp_t.view(logp.shape)

    @staticmethod
    @once_differentiable(CNF_SOLVE_DOUBLE_BACKWARD_MSG)
    def backward(ctx, g_z_out, g_logp_out):
        tape, image, e = ctx.saved_tensors
        g_z, g_image = cnf_integrate_backward(tape, e, image, g_z_out.contiguous(), g_logp_out.contiguous(), **ctx.kw)
        need = ctx.needs_input_grad
        return g_z if need[0] else None, g_logp_out if need[1] else None, g_image if need[2] else None, None, None
