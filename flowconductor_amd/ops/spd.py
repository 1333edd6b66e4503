"""Flows on SPD matrices (transforms/matrix/)."""
import torch

from flowconductor_amd import _hip
from ._core import _call, _err_word, _finish


SPD_MAX_DIM = 128   # FC_SPD_MAX_DIM: larger matrices take the reference's torch composition (transforms/matrix/)


def _matrices(inputs, name="inputs"):
    x = _hip.dev_f32(inputs, name)
    if x.dim() != 3 or x.shape[1] != x.shape[2]:
        raise ValueError("flowconductor_amd: %s must be [B, m, m], got %s" % (name, tuple(x.shape)))
    return x


def _tril_pack_nograd(x, m, mode):
    lib = _hip.load()
    n = x.shape[0]
    y = (torch.empty(n, m, m, dtype=torch.float32, device=x.device) if mode == 0
         else torch.empty(n, m * (m + 1) // 2, dtype=torch.float32, device=x.device))
    _call("fc_tril_pack", lib.fc_tril_pack, x.device, _hip.ptr(x), _hip.ptr(y), n, m, mode,
          _hip.stream_ptr(x.device))
    return y


class _TrilPackFunction(torch.autograd.Function):
    """Lower-triangle fill (mode 0) or gather (mode 1); the backward is the other mode of the same kernel."""

    @staticmethod
    def forward(ctx, x, m, mode):
        ctx.m, ctx.mode = m, mode
        return _tril_pack_nograd(x, m, mode)

    @staticmethod
    def backward(ctx, grad):
        return _tril_pack_nograd(_hip.dev_f32(grad, "grad"), ctx.m, 1 - ctx.mode), None, None


def fill_triangular(inputs, m):
    """``[B, m(m+1)/2] -> [B, m, m]``: the entries in ``np.tril_indices(m)`` order, zeros above the diagonal
    (bit-exact, permutations.py:97-106)."""
    x = _hip.dev_f32(inputs, "inputs")
    if x.dim() != 2 or x.shape[1] != m * (m + 1) // 2:
        raise ValueError("flowconductor_amd: fill_triangular expects [B, %d], got %s" % (m * (m + 1) // 2,
                                                                                         tuple(x.shape)))
    if torch.is_grad_enabled() and inputs.requires_grad:
        return _TrilPackFunction.apply(x, m, 0)
    return _tril_pack_nograd(x, m, 0)


def tril_gather(inputs):
    """``[B, m, m] -> [B, m(m+1)/2]``: the lower triangle in ``np.tril_indices(m)`` order (bit-exact)."""
    x = _matrices(inputs)
    m = x.shape[1]
    if torch.is_grad_enabled() and inputs.requires_grad:
        return _TrilPackFunction.apply(x, m, 1)
    return _tril_pack_nograd(x, m, 1)


def _diag_extract_nograd(x):
    lib = _hip.load()
    n, m = x.shape[0], x.shape[1]
    d = torch.empty(n, m, dtype=torch.float32, device=x.device)
    _call("fc_matrix_diag", lib.fc_matrix_diag, x.device, _hip.ptr(x), _hip.ptr(d), None, n, m, 0,
          _hip.stream_ptr(x.device))
    return d


def _diag_replace_nograd(x, diag, n, m, device):
    """A copy of ``x`` (zeros when ``x`` is None) with its diagonal replaced by ``diag``."""
    lib = _hip.load()
    y = torch.empty(n, m, m, dtype=torch.float32, device=device)
    _call("fc_matrix_diag", lib.fc_matrix_diag, device, _hip.ptr(x), _hip.ptr(diag), _hip.ptr(y), n, m, 1,
          _hip.stream_ptr(device))
    return y


class _DiagExtractFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        ctx.m = x.shape[1]
        return _diag_extract_nograd(x)

    @staticmethod
    def backward(ctx, grad):
        g = _hip.dev_f32(grad, "grad")
        return _diag_replace_nograd(None, g, g.shape[0], ctx.m, g.device)


class _DiagReplaceFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, diag):
        return _diag_replace_nograd(x, diag, x.shape[0], x.shape[1], x.device)

    @staticmethod
    def backward(ctx, grad):
        g = _hip.dev_f32(grad, "grad")
        n, m = g.shape[0], g.shape[1]
        grad_x = grad_diag = None
        if ctx.needs_input_grad[0]:
            grad_x = _diag_replace_nograd(g, torch.zeros(n, m, dtype=torch.float32, device=g.device), n, m, g.device)
        if ctx.needs_input_grad[1]:
            grad_diag = _diag_extract_nograd(g)
        return grad_x, grad_diag


def matrix_diagonal(inputs):
    """``torch.diagonal(inputs, dim1=-2, dim2=-1)`` of ``[B, m, m]`` as a contiguous ``[B, m]`` (bit-exact)."""
    x = _matrices(inputs)
    if torch.is_grad_enabled() and inputs.requires_grad:
        return _DiagExtractFunction.apply(x)
    return _diag_extract_nograd(x)


def matrix_replace_diagonal(inputs, diag):
    """``torch.diagonal_scatter(inputs, diag, dim1=-2, dim2=-1)`` (bit-exact)."""
    x = _matrices(inputs)
    d = _hip.dev_f32(diag, "diag")
    if d.shape != x.shape[:2]:
        raise ValueError("flowconductor_amd: diagonal of shape %s for matrices %s" % (tuple(d.shape), tuple(x.shape)))
    if torch.is_grad_enabled() and (inputs.requires_grad or diag.requires_grad):
        return _DiagReplaceFunction.apply(x, d)
    return _diag_replace_nograd(x, d, x.shape[0], x.shape[1], x.device)


def _cholesky_outer_nograd(x, checkargs):
    lib = _hip.load()
    n, m = x.shape[0], x.shape[1]
    y = torch.empty_like(x)
    lad = torch.empty(n, dtype=torch.float32, device=x.device)
    err = _err_word(x.device, checkargs)
    _call("fc_cholesky_outer", lib.fc_cholesky_outer, x.device, _hip.ptr(x), _hip.ptr(y), _hip.ptr(lad),
          _hip.ptr(err), n, m, 1 if checkargs else 0, _hip.stream_ptr(x.device))
    _finish(checkargs)
    return y, lad


class _CholeskyOuterFunction(torch.autograd.Function):
    """``L -> (0.5 (L L^T + (L L^T)^T), logabsdet)`` with the HIP backward ``fc_cholesky_outer_backward``."""

    @staticmethod
    def forward(ctx, x, checkargs):
        y, lad = _cholesky_outer_nograd(x, checkargs)
        ctx.save_for_backward(x)
        return y, lad

    @staticmethod
    def backward(ctx, grad_y, grad_lad):
        (x,) = ctx.saved_tensors
        lib = _hip.load()
        n, m = x.shape[0], x.shape[1]
        gy = _hip.dev_f32(grad_y, "grad") if grad_y is not None else None
        gl = _hip.dev_f32(grad_lad, "grad") if grad_lad is not None else None
        gx = torch.empty_like(x)
        _call("fc_cholesky_outer_backward", lib.fc_cholesky_outer_backward, x.device, _hip.ptr(x), _hip.ptr(gy),
              _hip.ptr(gl), _hip.ptr(gx), n, m, _hip.stream_ptr(x.device))
        return gx, None


def cholesky_outer(inputs, checkargs=True):
    """``CholeskyOuterProduct.forward`` (matrix/cholesky.py:18-25) for ``[B, m, m]``, ``m <= SPD_MAX_DIM``; with
    ``checkargs`` the reference's lower-triangular / positive-diagonal assertions come from the device error word."""
    x = _matrices(inputs)
    if x.shape[1] > SPD_MAX_DIM:
        raise ValueError("flowconductor_amd: cholesky_outer takes m <= %d" % SPD_MAX_DIM)
    if torch.is_grad_enabled() and inputs.requires_grad:
        return _CholeskyOuterFunction.apply(x, bool(checkargs))
    return _cholesky_outer_nograd(x, bool(checkargs))


def cholesky(inputs, eps, checkargs=True):
    """``CholeskyOuterProduct.inverse`` (matrix/cholesky.py:27-35): ``L = chol(A + eps I)`` and
    ``-(m log 2 + sum_i (m - i) log L_ii)``; no autograd (the transform takes torch's path when a gradient is due).
    A failed pivot raises the reference's assertion (``checkargs``) or ``torch.linalg.LinAlgError``."""
    lib = _hip.load()
    x = _matrices(inputs)
    _hip.require_no_grad(inputs)
    n, m = x.shape[0], x.shape[1]
    if m > SPD_MAX_DIM:
        raise ValueError("flowconductor_amd: cholesky takes m <= %d" % SPD_MAX_DIM)
    y = torch.empty_like(x)
    lad = torch.empty(n, dtype=torch.float32, device=x.device)
    err = _err_word(x.device, True)
    _call("fc_cholesky", lib.fc_cholesky, x.device, _hip.ptr(x), _hip.ptr(y), _hip.ptr(lad), _hip.ptr(err), n, m,
          float(eps), 1 if checkargs else 0, _hip.stream_ptr(x.device))
    _finish(True)
    return y, lad
