"""What every kernel family shares: the exceptions, the device error word, argument preparation and the launch helper.

Device error word -> Python exceptions.  The reference raises synchronously inside each spline call (four host syncs
per layer on a GPU).  Here kernels OR bits into one device word; a stand-alone transform call reads it
right away, a CompositeTransform / Flow defers the read to once per cascade.  ``_state`` (the thread-local bookkeeping
of that word) and ``KernelTimer._active`` exist here and nowhere else.
"""
import contextlib
import functools
import threading

import torch

from flowconductor_amd import _hip
# the run-time caches, re-exported: call sites say ``ops.memo`` / ``ops.cache_key`` / ``ops.invalidate_hip_caches``
from flowconductor_amd.runtime_cache import (  # noqa: F401
    buffer_list, cache_key, cached, device_plan, drop_param_list, has_hooks, invalidate_hip_caches, memo,
    module_list, param_list, static_memo, structure_key)


class InverseNotAvailable(Exception):
    """Exception to be thrown when a transform does not have an inverse."""


class InputOutsideDomain(Exception):
    """Exception to be thrown when the input to a transform is not within its domain."""


_state = threading.local()


def _flags():
    if not hasattr(_state, "flags"):
        _state.flags = {}
        _state.depth = 0
        _state.dirty = set()
    return _state.flags


def _flag_for(device):
    flags = _flags()
    key = (device.type, device.index)
    t = flags.get(key)
    if t is None:
        t = torch.zeros(1, dtype=torch.int32, device=device)
        flags[key] = t
    return t


def _raise_for(bits):
    if bits & _hip.ERR_OUTSIDE_DOMAIN:
        raise InputOutsideDomain()
    if bits & _hip.ERR_DISCRIMINANT:
        raise AssertionError("rational-quadratic inverse: negative discriminant")
    if bits & _hip.ERR_NONFINITE:
        raise FloatingPointError("non-finite value inside a bijector kernel")
    if bits & _hip.ERR_NOT_LOWER_TRIANGULAR:
        raise AssertionError(MSG_NOT_LOWER_TRIANGULAR)
    if bits & _hip.ERR_DIAGONAL_NONPOSITIVE:
        raise AssertionError(MSG_DIAGONAL_NONPOSITIVE)
    if bits & _hip.ERR_NOT_SYMMETRIC:
        raise AssertionError(MSG_NOT_SYMMETRIC)
    if bits & _hip.ERR_NOT_POSITIVE_DEFINITE:
        raise AssertionError(MSG_NOT_POSITIVE_DEFINITE)
    if bits & _hip.ERR_CHOLESKY_FAILED:
        raise torch.linalg.LinAlgError(MSG_CHOLESKY_FAILED)


# the reference's messages (transforms/matrix/cholesky.py:37-49) and torch.linalg.cholesky's failure
MSG_NOT_SQUARE = "input tensor must be mini batch of square matrices"
MSG_NOT_LOWER_TRIANGULAR = "input tensor must be mini batch of lower triangular matrices"
MSG_DIAGONAL_NONPOSITIVE = "input tensor must be mini batch of lower triangular matrices with positive diagonal elements"
MSG_NOT_SYMMETRIC = "Input matrix is not symmetric."
MSG_NOT_POSITIVE_DEFINITE = ("Input matrix is not positive semi-definite in order to perform Cholesky "
                             "decomposition")
MSG_CHOLESKY_FAILED = ("linalg.cholesky: The factorization could not be completed because the input is not "
                       "positive-definite.")


def _check_now():
    flags = _flags()
    dirty, _state.dirty = _state.dirty, set()
    bits = 0
    for key in dirty:
        t = flags[key]
        bits |= int(t.item())
        if bits:
            t.zero_()
    if bits:
        _raise_for(bits)


@contextlib.contextmanager
def deferred_errors():
    """Read the device error word once when the outermost block exits."""
    _flags()
    _state.depth += 1
    try:
        yield
    except BaseException:
        _state.depth -= 1
        if _state.depth == 0:
            for key in _state.dirty:
                _state.flags[key].zero_()
            _state.dirty = set()
        raise
    else:
        _state.depth -= 1
        if _state.depth == 0:
            _check_now()


@contextlib.contextmanager
def capture_mode():
    """Inside a HIP-graph capture the error word cannot be read (no host sync): kernels still OR their bits into
    it, ``check_errors`` reads it after a replay."""
    _flags()
    _state.depth += 1
    try:
        yield
    finally:
        _state.depth -= 1
        _state.dirty = set()


def check_errors(device):
    """Read (and clear) the device error word of ``device`` now; raises the reference's exceptions."""
    _flags()
    _state.dirty.add((device.type, device.index))
    _flag_for(device)
    _check_now()


def _err_word(device, may_raise):
    """Device pointer for the kernel's error word (None when the op cannot raise)."""
    if not may_raise:
        return None
    _flags()
    _state.dirty.add((device.type, device.index))
    return _flag_for(device)


def _finish(may_raise):
    if may_raise and _state.depth == 0:
        _check_now()


def _as_cols(cols, device):
    if cols is None:
        return None
    if cols.dtype != torch.int32 or cols.device != device or not cols.is_contiguous():
        cols = cols.to(device=device, dtype=torch.int32).contiguous()
    return cols


def _prep_2d(inputs, name="inputs", align16=False):
    x = _hip.dev_f32(inputs, name)
    if x.dim() != 2:
        raise ValueError("%s must be [batch, features], got shape %s" % (name, tuple(x.shape)))
    return _aligned16(x) if align16 else x


def _aligned16(t):
    """The matrix-core kernels move rows as 16-byte pieces: a contiguous view that starts off a 16-byte boundary
    (``data[1:]`` with a feature count that is not a multiple of 4) is copied to a fresh allocation first."""
    return t if t.data_ptr() % 16 == 0 else t.clone()


LAD_STORE, LAD_ACCUMULATE, LAD_STORE_NEG, LAD_ACCUMULATE_NEG = 0, 1, 2, 3


class KernelTimer:
    """Times every launch of one C-ABI entry point with HIP events recorded on the stream the
    kernel is launched on (the current torch stream).  Used by bench.py for ``roofline``."""

    _active = []

    def __init__(self, name):
        self.name = name
        self.pairs = []

    def __enter__(self):
        KernelTimer._active.append(self)
        return self

    def __exit__(self, *exc):
        KernelTimer._active.remove(self)
        return False

    def durations_ms(self):
        """Per-launch durations; call after the stream has been synchronised."""
        return [a.elapsed_time(b) for a, b in self.pairs]


def _call(name, fn, device, *args):
    """Launch C-ABI entry ``fn`` (asynchronous), bracketing it with events for active timers."""
    if device.index is not None and device.index != torch.cuda.current_device():
        # the launchers size grids and set kernel attributes for the CURRENT device: make it the tensors' device
        with torch.cuda.device(device):
            return _call(name, fn, device, *args)
    timers = [t for t in KernelTimer._active if t.name == name]
    if timers:
        start = torch.cuda.Event(enable_timing=True)
        end = torch.cuda.Event(enable_timing=True)
        start.record(torch.cuda.current_stream(device))
    code = fn(*args)
    if timers:
        end.record(torch.cuda.current_stream(device))
        for t in timers:
            t.pairs.append((start, end))
    _hip.check(code, name)


def once_differentiable(message):
    """Decorator for the ``backward`` of an autograd node whose gradient is a kernel autograd cannot see into: a backward
    that is itself being recorded (``create_graph=True``) raises ``RuntimeError(message)`` before anything runs, every
    other one runs under ``torch.autograd.function.once_differentiable``."""
    def wrap(backward_once):
        once = torch.autograd.function.once_differentiable(backward_once)

        @functools.wraps(backward_once)
        def backward(ctx, *grads):
            if torch.is_grad_enabled():
                raise RuntimeError(message)
            return once(ctx, *grads)
        return backward
    return wrap


def rq_param_count(num_bins, tails):
    """Parameters per transformed dim of an RQ spline: K widths, K heights and the K - 1 inner derivatives with linear
    tails (3K - 1), all K + 1 derivatives otherwise (3K + 1)."""
    return 3 * num_bins - 1 if tails == "linear" else 3 * num_bins + 1


def _logabsdet_target(logabsdet_accum, n, device):
    """``(lad, flags)`` of a kernel that stores its logabsdet [N] or adds it onto a running total: a fresh tensor and 0, or
    the checked ``logabsdet_accum`` and 1 (``FC_RQ_ACCUMULATE_LOGABSDET`` / ``LAD_ACCUMULATE``)."""
    if logabsdet_accum is None:
        return torch.empty(n, dtype=torch.float32, device=device), 0
    lad = logabsdet_accum
    if lad.dtype != torch.float32 or lad.shape != (n,) or not lad.is_contiguous() or lad.device != device:
        raise ValueError("logabsdet_accum must be a contiguous float32 [N] tensor on the inputs' device")
    return lad, 1


def _pad_to(t, shape):
    """``t`` zero-padded at the end of every dim up to ``shape`` (returns ``t`` itself when nothing is missing)."""
    if tuple(t.shape) == tuple(shape):
        return t.contiguous()
    out = t.new_zeros(shape)
    out[tuple(slice(0, k) for k in t.shape)] = t
    return out
