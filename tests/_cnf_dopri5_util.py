"""Shared by tests/test_cnf_dopri5_host.py and tests/test_gpu_cnf_dopri5.py: the float64 reference of the per-row
Dormand-Prince solve (``fc_cnf_dopri5``), independent of the kernel and of the package's host loop.

``dopri5_rows`` is ``_Dopri5.advance`` of ``flowconductor_amd/CNF/odeint.py`` with the batch-wide error norm replaced
by the row's own: every row has its own time, step size, accept / reject decisions and attempt count.  It is
vectorised over rows with per-row masks; the field is ``row_field``: the net written out in float64 from a copy of the
``ODEfunc``'s parameters, with one time per row and nothing shared between rows.  A row that uses up
``max_attempts``, whose error ratio is not finite, or whose step no longer moves ``t`` stops and returns NaN, as in the
kernel.
"""
import torch

from flowconductor_amd.CNF.odeint import DOPRI5, ERROR_EXPONENT, MAX_FACTOR, MIN_FACTOR, SAFETY
from _cnf_util import make_cnf, make_func, rk_solve, scale_of, worst  # noqa: F401  (re-exported for the two test files)


TOL = 1e-5
ATTEMPT_ROWS = 8        # of 64: the kernel's attempts may differ from the rounded reference's in 1/8 of the rows ...
ATTEMPT_GAP = 2         # ... and nowhere by more than this


def mixed_rows(n, seed):
    """``[n, 2]`` rows, the first half of scale 0.1, the second of scale 6: easy and hard rows in one batch."""
    z = torch.randn(n, 2, generator=torch.Generator().manual_seed(seed))
    z[: n // 2] *= 0.1
    z[n // 2:] *= 6.0
    return z


def step_control_case():
    """D 2, 3 x 64, N 64: at ``TOL`` the rounded reference takes 4 attempts in every easy row and 3 in nearly every
    hard one (tests/test_cnf_dopri5_host.py checks it)."""
    return make_func(2, (64, 64, 64), seed=15, gain=2.0), mixed_rows(64, 150)


# (name, seed, gain, first_step): with three attempts allowed some rows finish and some do not.  Without a first step
# no row can finish in fewer than three attempts (the initial step is at most 100 * h0 and grows tenfold at most); with
# first_step = 1 a row whose one-step error passes finishes in one.
CAP_CASES = [("heuristic", 17, 3.0, None), ("first_step", 18, 2.0, 1.0)]
CAP = 3


def cap_case(seed, gain):
    return make_func(2, (64, 64, 64), seed=seed, gain=gain), mixed_rows(64, 170)


def _per_row(fn, x):
    """``fn(x)`` element-wise, every row of ``x`` padded to whole SIMD vectors first: the vector loop and the remainder
    loop of a library's transcendental functions may differ in the last bit, and which of them an element meets would
    otherwise depend on the size of the batch."""
    flat = x.reshape(x.shape[0], -1)
    padded = torch.nn.functional.pad(flat, (0, (-flat.shape[1]) % 16))
    return fn(padded)[:, :flat.shape[1]].reshape(x.shape)


def _activation(name, x):
    """``(f(x), f'(x))`` of a ``NONLINEARITIES`` entry in float64."""
    sigmoid = _per_row(torch.sigmoid, x)
    if name == "Tanh":
        tanh = _per_row(torch.tanh, x)
        return tanh, 1.0 - tanh * tanh
    if name == "ReLU":
        return torch.relu(x), (x > 0).to(x.dtype)
    if name == "Softplus":
        return _per_row(torch.nn.functional.softplus, x), sigmoid
    if name == "ELU":
        return (torch.where(x > 0, x, _per_row(torch.expm1, x)),
                torch.where(x > 0, torch.ones_like(x), _per_row(torch.exp, x)))
    if name == "SiLU":
        return x * sigmoid, sigmoid + x * sigmoid * (1.0 - sigmoid)
    if name == "Lambda":        # square
        return x * x, 2.0 * x
    assert name == "Identity", name
    return x, torch.ones_like(x)


def row_field(func):
    """``field(t [N], y [N, D]) -> (dy [N, D], -div [N])`` of ``func`` in float64 with ONE TIME PER ROW, written out
    from the parameters: the value and the D unit tangents of a row go through the layers as one ``[D + 1, width]``
    matrix, and the products with the weights are element-wise sums in a fixed order, so that what a row gives depends
    on nothing but the row.  For the five layer kinds of one form, ``(W x + b + w_t t) gate + w_b t``.
    tests/test_cnf_dopri5_host.py pins it to the package's float64 composition."""
    net = func.diffeq
    layers = []
    for layer in net.layers:
        kind = type(layer).__name__
        weight, bias = layer._layer.weight.detach().double().cpu(), layer._layer.bias.detach().double().cpu()
        zero = torch.zeros_like(bias)
        w_t = w_g = b_g = w_b = None
        if kind == "ConcatLinear":
            w_t, weight = weight[:, 0], weight[:, 1:]
        elif kind == "ConcatLinear_v2":
            w_b = layer._hyper_bias.weight.detach().double().cpu().reshape(-1)
        elif kind == "SquashLinear":
            w_g, b_g = layer._hyper.weight.detach().double().cpu().reshape(-1), layer._hyper.bias.detach().double().cpu()
        elif kind == "ConcatSquashLinear":
            w_g = layer._hyper_gate.weight.detach().double().cpu().reshape(-1)
            b_g = layer._hyper_gate.bias.detach().double().cpu()
            w_b = layer._hyper_bias.weight.detach().double().cpu().reshape(-1)
        else:
            assert kind == "IgnoreLinear", kind
        layers.append((weight.t().contiguous(), bias, zero if w_t is None else w_t, w_g, b_g,
                       zero if w_b is None else w_b))
    act = type(net.activation_fns[0]).__name__ if len(layers) > 1 else "Identity"
    scale, residual = float(net.scale_output), bool(func.residual)

    def field(t, y):
        n, d = y.shape
        t = t.reshape(n, 1).double()
        x = torch.cat([y.reshape(n, 1, d), torch.eye(d, dtype=torch.float64).expand(n, d, d)], dim=1)
        for index, (wt, bias, w_t, w_g, b_g, w_b) in enumerate(layers):
            lin = torch.zeros(n, d + 1, wt.shape[1], dtype=torch.float64)     # [N, D + 1, out]
            for k in range(wt.shape[0]):        # correctly rounded products and sums in a fixed order: a library
                lin += x[:, :, k, None] * wt[k]             # matrix product may choose its order by the batch size
            gate = _per_row(torch.sigmoid, w_g * t + b_g) if w_g is not None else torch.ones(n, wt.shape[1], dtype=torch.float64)
            value = (lin[:, 0] + bias + w_t * t) * gate + w_b * t
            tangents = lin[:, 1:] * gate[:, None, :]
            if index < len(layers) - 1:
                value, slope = _activation(act, value)
                tangents = tangents * slope[:, None, :]
            x = torch.cat([value[:, None, :], tangents], dim=1)
        dy = scale * x[:, 0]
        div = scale * torch.diagonal(x[:, 1:], dim1=1, dim2=2).sum(dim=1)
        if residual:
            dy, div = dy - y, div - d
        return dy, -div

    return field


def _combine(coefficients, slopes):
    """``sum_j coefficients[j] * slopes[j]`` in order, zero coefficients skipped (as ``odeint._axpy`` adds them)."""
    total = None
    for c, k in zip(coefficients, slopes):
        if c != 0.0:
            total = c * k if total is None else total + c * k
    return total


def _rms(v):
    return v.square().mean(dim=1).sqrt()


def dopri5_rows(func, z, t0, t1, atol, rtol, first_step=None, max_attempts=4096, round_stage_input=False):
    """``(z(t1) [N, D], delta logp [N], attempts [N] int64)`` in float64 on the CPU, every row on its own.

    ``round_stage_input=True`` rounds each stage state to float32 before the float64 net: the kernel's one rounding.
    ``dopri5_rows.last_evals`` holds the evaluations every row of the last call took part in."""
    evaluate = row_field(func)
    z0 = z.detach().double().cpu()
    n, d = z0.shape
    y = torch.cat([z0, torch.zeros(n, 1, dtype=torch.float64)], dim=1)
    counts = torch.zeros(n, dtype=torch.int64)

    def field(t_rows, state, mask):
        rows = state[:, :d]
        if round_stage_input:
            rows = rows.float().double()
        dy, negdiv = evaluate(t_rows, rows)
        counts.add_(mask.long())
        return torch.cat([dy, negdiv.reshape(-1, 1)], dim=1)

    t0, t1 = float(t0), float(t1)
    span = t1 - t0
    aspan, direction = abs(span), (1.0 if span > 0 else -1.0)
    reach = 1e-12 * max(1.0, aspan)
    t = torch.full((n,), t0, dtype=torch.float64)
    done = torch.zeros(n, dtype=torch.float64)
    attempts = torch.zeros(n, dtype=torch.int64)
    failed = torch.zeros(n, dtype=torch.bool)
    active = torch.full((n,), aspan > reach)
    dopri5_rows.last_evals = counts
    if not bool(active.any()):
        return y[:, :d], y[:, d], attempts

    k1 = field(t, y, active)
    if first_step is None:      # Hairer, Norsett & Wanner II.4 in the row's own scaled norm
        scale = atol + rtol * y.abs()
        d0, d1 = _rms(y / scale), _rms(k1 / scale)
        h0 = torch.where((d0 < 1e-5) | (d1 < 1e-5), torch.full_like(d0, 1e-6), 0.01 * d0 / d1)
        dh = direction * h0
        f1 = field(t + dh, y + dh[:, None] * k1, active)
        d2 = _rms((f1 - k1) / scale) / h0
        top = torch.maximum(d1, d2)
        h1 = torch.where(top <= 1e-15, torch.clamp(h0 * 1e-3, min=1e-6), _per_row(lambda v: v ** (1 / 5), 0.01 / top))
        hmag = torch.minimum(100 * h0, h1)
    else:
        hmag = torch.full((n,), float(first_step), dtype=torch.float64)

    while bool(active.any()):
        capped = active & (attempts >= max_attempts)
        failed |= capped
        active = active & ~capped
        attempts = attempts + active.long()
        last = hmag >= aspan - done
        h = torch.where(last, t1 - t, direction * hmag)
        stuck = active & ~last & (t + h == t)
        failed |= stuck
        active = active & ~stuck
        if not bool(active.any()):
            break
        slopes = [k1]
        for stage in range(1, 7):
            y_new = y + h[:, None] * _combine(DOPRI5["a"][stage], slopes)
            slopes.append(field(t + DOPRI5["c"][stage] * h, y_new, active))
        error = h[:, None] * _combine(DOPRI5["e"], slopes)
        ratio = _rms(error / (atol + rtol * torch.maximum(y.abs(), y_new.abs())))
        bad = active & ~torch.isfinite(ratio)
        failed |= bad
        active = active & ~bad
        factor = torch.where(ratio == 0.0, torch.full_like(ratio, MAX_FACTOR),
                             torch.clamp(SAFETY * _per_row(lambda v: v ** ERROR_EXPONENT, ratio), MIN_FACTOR, MAX_FACTOR))
        accept = active & (ratio <= 1.0)
        reject = active & ~(ratio <= 1.0)
        grown = torch.where(~last | (factor < 1.0), hmag * factor, torch.maximum(hmag, h.abs() * factor))
        shrunk = h.abs() * torch.clamp(factor, max=1.0)
        done = torch.where(accept, torch.where(last, torch.full_like(done, aspan), done + hmag), done)
        t = torch.where(accept, torch.where(last, torch.full_like(t, t1), t + h), t)
        y = torch.where(accept[:, None], y_new, y)
        k1 = torch.where(accept[:, None], slopes[6], k1)
        hmag = torch.where(accept, grown, torch.where(reject, shrunk, hmag))
        active = active & (aspan - done > reach)

    y = torch.where(failed[:, None], torch.full_like(y, float("nan")), y)
    return y[:, :d], y[:, d], attempts
