"""The package's own ODE solver for tuples of tensors (``torchdiffeq`` is not a dependency), in torch ops.

``odeint(func, y0, t, atol, rtol, method, options, adjoint_options)`` integrates ``dy/dt = func(t, y)`` from ``t[0]``
through every later entry of ``t`` and returns, per state tensor, the states at those times stacked along a new
first axis (``[len(t), ...]``).

* ``euler``, ``midpoint`` (the explicit midpoint rule) and ``rk4`` (the CLASSICAL fourth-order tableau, weights
  1/6, 1/3, 1/3, 1/6 -- not the 3/8 rule) take equal steps: ``ceil(|t[i+1] - t[i]| / options["step_size"])`` of them
  per interval, one without a step size.
* ``dopri5`` is the Dormand-Prince 5(4) pair with first-same-as-last, Hairer's initial step, and the elementary
  controller ``h <- h * clip(0.9 * err ** -0.2, 0.2, 10)`` (no PI term; after a rejected step the factor is capped at
  1).  ``err`` is the root mean square over EVERY element of every state tensor -- the batch is one system -- of
  ``(y5 - y4) / (atol + rtol * max(|y0|, |y1|))``; a step is accepted when ``err <= 1``.  The last step of an
  interval is shortened to end on it; there is no dense output.  ``options["max_num_steps"]`` (default 2 ** 31 - 1)
  bounds the attempts, ``options["first_step"]`` replaces the initial-step heuristic.

Gradients are plain autograd through the accepted steps (discretise-then-optimise): whatever ``func`` and the entries
of ``t`` carry a graph for is differentiated through the arithmetic of the steps; the step-size decisions are taken on
detached numbers.  There is no continuous adjoint; ``adjoint_options`` is accepted and ignored.  Nothing here claims
the step sequence of another library."""
import math

import torch

__all__ = ["odeint", "fixed_grid_steps", "FIXED_STEP_TABLEAUS", "DOPRI5"]

# (c, A rows, b) of the explicit fixed-step methods
FIXED_STEP_TABLEAUS = {
    "euler": ((0.0,), ((),), (1.0,)),
    "midpoint": ((0.0, 0.5), ((), (0.5,)), (0.0, 1.0)),
    "rk4": ((0.0, 0.5, 0.5, 1.0), ((), (0.5,), (0.0, 0.5), (0.0, 0.0, 1.0)), (1 / 6, 1 / 3, 1 / 3, 1 / 6)),
}

# Dormand-Prince 5(4): nodes, coefficients, the fifth-order weights (= the last row: first same as last) and the
# difference between the fifth- and the fourth-order weights
DOPRI5 = {
    "c": (0.0, 1 / 5, 3 / 10, 4 / 5, 8 / 9, 1.0, 1.0),
    "a": ((),
          (1 / 5,),
          (3 / 40, 9 / 40),
          (44 / 45, -56 / 15, 32 / 9),
          (19372 / 6561, -25360 / 2187, 64448 / 6561, -212 / 729),
          (9017 / 3168, -355 / 33, 46732 / 5247, 49 / 176, -5103 / 18656),
          (35 / 384, 0.0, 500 / 1113, 125 / 192, -2187 / 6784, 11 / 84)),
    "b": (35 / 384, 0.0, 500 / 1113, 125 / 192, -2187 / 6784, 11 / 84, 0.0),
    "e": (35 / 384 - 5179 / 57600, 0.0, 500 / 1113 - 7571 / 16695, 125 / 192 - 393 / 640,
          -2187 / 6784 + 92097 / 339200, 11 / 84 - 187 / 2100, -1 / 40),
}
SAFETY, MIN_FACTOR, MAX_FACTOR, ERROR_EXPONENT = 0.9, 0.2, 10.0, -1 / 5


def _number(t):
    """A time as a Python float (reading a device tensor waits for the device)."""
    return float(t.detach()) if isinstance(t, torch.Tensor) else float(t)


def _needs_graph(t):
    return isinstance(t, torch.Tensor) and t.requires_grad and torch.is_grad_enabled()


def _times(t):
    """The entries of ``t``: floats, or 0-dim tensors where an entry carries a graph."""
    if isinstance(t, torch.Tensor):
        if t.dim() != 1:
            raise ValueError("odeint: t must be one-dimensional")
        if _needs_graph(t):
            return [t[i] for i in range(t.shape[0])]
        return [float(v) for v in t.detach().tolist()]
    return [v if _needs_graph(v) else _number(v) for v in t]


def fixed_grid_steps(t0, t1, options):
    """Number of equal steps a fixed-step method takes from ``t0`` to ``t1``."""
    step_size = (options or {}).get("step_size")
    if step_size is None:
        return 1
    step_size = _number(step_size)
    if not step_size > 0:
        raise ValueError("odeint: step_size must be positive")
    return max(1, math.ceil(abs(_number(t1) - _number(t0)) / step_size - 1e-9))


def _axpy(y, h, coefficients, slopes):
    """``y + h * sum_j coefficients[j] * slopes[j]`` per state tensor (zero coefficients skipped)."""
    out = []
    for i, yi in enumerate(y):
        total = None
        for c, k in zip(coefficients, slopes):
            if c != 0.0:
                total = c * k[i] if total is None else total + c * k[i]
        out.append(yi if total is None else yi + h * total)
    return tuple(out)


def _rk_slopes(func, t, y, h, c, a, first=None):
    slopes = [tuple(func(t, y)) if first is None else first]
    for ci, row in zip(c[1:], a[1:]):
        slopes.append(tuple(func(t + ci * h, _axpy(y, h, row, slopes))))
    return slopes


def _fixed_step(func, y, t0, t1, method, options):
    c, a, b = FIXED_STEP_TABLEAUS[method]
    steps = fixed_grid_steps(t0, t1, options)
    h = (t1 - t0) / steps
    for i in range(steps):
        t = t0 + i * h
        y = _axpy(y, h, b, _rk_slopes(func, t, y, h, c, a))
    return y


def _rms(tensors):
    """Root mean square over every element of every tensor, as a Python float."""
    count = sum(v.numel() for v in tensors)
    total = sum(v.detach().double().square().sum() for v in tensors)
    return math.sqrt(float(total) / max(count, 1))


def _initial_step(func, t0, y0, f0, direction, atol, rtol):
    """Hairer, Norsett & Wanner, Solving ODEs I, II.4: a step from the sizes of y, y' and an Euler probe of y''."""
    scale = [atol + rtol * v.detach().abs() for v in y0]
    d0 = _rms([v.detach() / s for v, s in zip(y0, scale)])
    d1 = _rms([v.detach() / s for v, s in zip(f0, scale)])
    h0 = 1e-6 if d0 < 1e-5 or d1 < 1e-5 else 0.01 * d0 / d1
    with torch.no_grad():
        y1 = tuple(v + direction * h0 * f for v, f in zip(y0, f0))
        f1 = func(_number(t0) + direction * h0, y1)
    d2 = _rms([(a - b.detach()) / s for a, b, s in zip(f1, f0, scale)]) / h0
    top = max(d1, d2)
    h1 = max(1e-6, h0 * 1e-3) if top <= 1e-15 else (0.01 / top) ** (1 / 5)
    return min(100 * h0, h1)


class _Dopri5:
    """Carries the step size and the first-same-as-last slope across the intervals of one ``odeint`` call."""

    def __init__(self, func, y0, t0, atol, rtol, options):
        self.func, self.atol, self.rtol = func, atol, rtol
        self.max_num_steps = int(options.get("max_num_steps", 2 ** 31 - 1))
        self.first_step = options.get("first_step")
        self.h = None
        self.slope = tuple(func(t0, y0))
        self.attempts = 0

    def advance(self, y, t0, t1):
        span = _number(t1) - _number(t0)
        if span == 0.0:
            return y
        direction = 1.0 if span > 0 else -1.0
        if self.h is None:
            self.h = (_number(self.first_step) if self.first_step is not None
                      else _initial_step(self.func, t0, y, self.slope, direction, self.atol, self.rtol))
        t, done = t0, 0.0           # ``done``: the distance covered, a float
        while abs(span) - done > 1e-12 * max(1.0, abs(span)):
            self.attempts += 1
            if self.attempts > self.max_num_steps:
                raise RuntimeError("odeint: max_num_steps (%d) exceeded" % self.max_num_steps)
            last = self.h >= abs(span) - done
            h = (t1 - t) if last else direction * self.h        # a tensor only where t1 carries a graph
            slopes = _rk_slopes(self.func, t, y, h, DOPRI5["c"], DOPRI5["a"], first=self.slope)
            y_new = _axpy(y, h, DOPRI5["b"], slopes)
            slopes_end = slopes[-1]                              # evaluated at y_new: stage 7 uses the weights b
            error = _axpy(tuple(torch.zeros_like(v) for v in y), _number(h), DOPRI5["e"],
                          [tuple(k.detach() for k in s) for s in slopes])
            ratio = _rms([e / (self.atol + self.rtol * torch.maximum(a.detach().abs(), b.detach().abs()))
                          for e, a, b in zip(error, y, y_new)])
            if not math.isfinite(ratio):
                raise FloatingPointError("odeint: non-finite error estimate")
            factor = MAX_FACTOR if ratio == 0.0 else min(MAX_FACTOR, max(MIN_FACTOR, SAFETY * ratio ** ERROR_EXPONENT))
            if ratio <= 1.0:
                done = abs(span) if last else done + self.h
                t = t1 if last else t + h
                y, self.slope = y_new, slopes_end
                if not last or factor < 1.0:
                    self.h = self.h * factor
                else:                                            # a shortened last step says little about the next
                    self.h = max(self.h, abs(_number(h)) * factor)
            else:
                self.h = abs(_number(h)) * min(1.0, factor)
        return y


def odeint(func, y0, t, atol=1e-5, rtol=1e-5, method="dopri5", options=None, adjoint_options=None):
    del adjoint_options         # accepted for call compatibility: there is no adjoint here
    options = dict(options or {})
    single = isinstance(y0, torch.Tensor)
    y = (y0,) if single else tuple(y0)
    call = (lambda s, v: (func(s, v[0]),)) if single else func
    times = _times(t)
    if len(times) < 2:
        raise ValueError("odeint: t needs at least two entries")
    if method == "dopri5":
        solver = _Dopri5(call, y, times[0], float(atol), float(rtol), options)
    elif method not in FIXED_STEP_TABLEAUS:
        raise ValueError("odeint: unknown method %r (dopri5, euler, midpoint, rk4)" % (method,))
    states = [y]
    for t0, t1 in zip(times[:-1], times[1:]):
        y = solver.advance(y, t0, t1) if method == "dopri5" else _fixed_step(call, y, t0, t1, method, options)
        states.append(y)
    stacked = tuple(torch.stack([s[i] for s in states]) for i in range(len(y)))
    return stacked[0] if single else stacked
