"""Row-per-wavefront bijectors with dense parameters: Householder, planar, the linear family (dense, LU, upper, per-sample,
Householder-diagonal-Householder) and Sylvester with its matrix-core products.
"""
import torch

from flowconductor_amd import _hip
from ._core import _aligned16, _call, _prep_2d


class _LULinearFunction(torch.autograd.Function):
    """``y = L (U x) + b`` / ``y = U^-1 L^-1 (x - b)`` by the HIP kernel; gradients by library GEMMs and triangular
    solves on the device (lu.py:56-91 under autograd)."""

    @staticmethod
    def forward(ctx, inputs, lower, upper, bias, inverse):
        with torch.no_grad():
            outputs = linear(inputs, upper, lower, bias, mode=LINEAR_LU_INVERSE if inverse else LINEAR_LU_FORWARD)
        ctx.save_for_backward(inputs, lower, upper, outputs)
        ctx.inverse = inverse
        return outputs

    @staticmethod
    def backward(ctx, gy):
        x, lower, upper, y = ctx.saved_tensors
        if not ctx.inverse:
            ux = x @ upper.T
            g_ux = gy @ lower
            return g_ux @ upper, gy.T @ ux, g_ux.T @ x, gy.sum(0), None
        # y = W^-1 (x - b), W = L U:  gz = W^-T gy;  dW = -gz^T y;  dL = dW U^T, dU = L^T dW
        t = torch.linalg.solve_triangular(upper.T, gy.T, upper=False)
        gz = torch.linalg.solve_triangular(lower.T, t, upper=True, unitriangular=True).T
        gw = -(gz.T @ y)
        return gz, gw @ upper.T, lower.T @ gw, -gz.sum(0), None


def lu_linear_autograd(inputs, lower, upper, bias, inverse=False):
    """LU-parameterised linear map with an autograd node (training / differentiable sampling)."""
    return _LULinearFunction.apply(_prep_2d(inputs), lower, upper, bias, inverse)


class _DenseLinearFunction(torch.autograd.Function):
    """``y = W x + b`` / ``y = W^-1 (x - b)`` by the ``fc_linear`` kernel; gradients by library GEMMs on the device
    (``NaiveLinear`` under autograd, linear.py:159-190).  The inverse direction is handed ``W^-1`` (no graph of its own): with
    ``gz = gy W^-1`` the gradients are ``gx = gz``, ``dW = -gz^T y``, ``db = -sum gz``."""

    @staticmethod
    def forward(ctx, inputs, weight, bias, weight_inverse):
        ctx.inverse = weight_inverse is not None
        with torch.no_grad():
            if ctx.inverse:
                outputs = linear(inputs, weight_inverse, bias=bias, mode=LINEAR_DENSE_SHIFTED)
                ctx.save_for_backward(outputs, weight_inverse)
            else:
                outputs = linear(inputs, weight, bias=bias, mode=LINEAR_DENSE)
                ctx.save_for_backward(inputs, weight)
        return outputs

    @staticmethod
    def backward(ctx, gy):
        saved, matrix = ctx.saved_tensors
        if not ctx.inverse:
            return gy @ matrix, gy.T @ saved, gy.sum(0), None
        gz = gy @ matrix
        return gz, -(gz.T @ saved), -gz.sum(0), None


def dense_linear_autograd(inputs, weight, bias, weight_inverse=None):
    """Dense linear map with an autograd node (training / differentiable sampling); with ``weight_inverse`` (``W^-1`` as a
    tensor without a graph) the inverse direction, whose gradients still reach ``weight`` and ``bias``."""
    return _DenseLinearFunction.apply(_prep_2d(inputs), weight, bias, weight_inverse)


class _UpperLinearFunction(torch.autograd.Function):
    """``y = R x`` / ``y = R^-1 x`` with an upper-triangular ``R`` by the ``fc_linear`` kernel (the inverse is its back
    substitution: ``LINEAR_LU_INVERSE`` with a unit lower factor); gradients by library GEMMs and one triangular solve
    (qr.py:45-82 under autograd)."""

    @staticmethod
    def forward(ctx, inputs, upper, inverse):
        with torch.no_grad():
            outputs = upper_linear(inputs, upper, inverse=inverse)
        ctx.save_for_backward(outputs if inverse else inputs, upper)
        ctx.inverse = inverse
        return outputs

    @staticmethod
    def backward(ctx, gy):
        saved, upper = ctx.saved_tensors
        if not ctx.inverse:
            return gy @ upper, gy.T @ saved, None
        # y = R^-1 x:  gx = R^-T gy;  dR = -gx^T y
        gx = torch.linalg.solve_triangular(upper.T, gy.T, upper=False).T
        return gx, -(gx.T @ saved), None


def upper_linear(inputs, upper, bias=None, inverse=False):
    """``R x + bias`` or the back substitution ``R^-1 (x - bias)`` for an upper-triangular ``R`` (``fc_linear``)."""
    if not inverse:
        return linear(inputs, upper, bias=bias, mode=LINEAR_DENSE)
    eye = torch.eye(upper.shape[0], dtype=torch.float32, device=inputs.device)
    return linear(inputs, upper, eye, bias, mode=LINEAR_LU_INVERSE)


def upper_linear_autograd(inputs, upper, inverse=False):
    """Upper-triangular linear map with an autograd node (training / differentiable sampling)."""
    return _UpperLinearFunction.apply(_prep_2d(inputs), upper, inverse)


MAX_ROW_FEATURES = 512


def _rows(inputs, name="inputs", align16=False):
    x = _prep_2d(inputs, name, align16)
    if x.shape[1] > MAX_ROW_FEATURES:
        raise ValueError("flowconductor_amd: %d features exceed the %d supported by the row kernels"
                         % (x.shape[1], MAX_ROW_FEATURES))
    return x


def _param(t, device, name):
    """A parameter operand (module-owned or produced per sample by a hyper-network) as a device f32 tensor.  These
    kernels have no backward: a parameter that still carries a graph is refused rather than silently detached."""
    if isinstance(t, torch.Tensor):
        _hip.require_no_grad(t)
    return _hip.dev_f32(torch.as_tensor(t).detach().to(device), name)


def _check_q_vectors(q, x):
    """``q`` [K, D] shared or [N, K, D] per sample against the rows ``x``; True when per-sample."""
    n, d = x.shape
    per_sample = q.dim() == 3
    if q.shape[-1] != d or (per_sample and q.shape[0] != n) or q.dim() not in (2, 3):
        raise ValueError("q_vectors of shape %s do not match inputs %s" % (tuple(q.shape), tuple(x.shape)))
    return per_sample


def _check_planar_parameters(wv, uv, bv, x, per_sample):
    n, d = x.shape
    rows = n if per_sample else 1
    if wv.numel() != rows * d or uv.numel() != rows * d or bv.numel() != rows:
        raise ValueError("planar parameters do not match %d features" % d)


def _check_matrices(m, x):
    n, d = x.shape
    if m.numel() != n * d * d:
        raise ValueError("matrices must be [%d, %d, %d]" % (n, d, d))


def householder(inputs, q_vectors, reverse=False):
    """Apply K Householder reflections (reference orthogonal.py:144-194).

    ``q_vectors``: ``[K, D]`` shared across the batch or ``[N, K, D]`` per sample."""
    lib = _hip.load()
    x = _rows(inputs)
    _hip.require_no_grad(inputs, q_vectors)
    q = _param(q_vectors, x.device, "q_vectors")
    n, d = x.shape
    per_sample = _check_q_vectors(q, x)
    y = torch.empty_like(x)
    _call("fc_householder", lib.fc_householder, x.device, _hip.ptr(x), _hip.ptr(y), _hip.ptr(q), n, d,
          q.shape[-2], 1 if per_sample else 0, 1 if reverse else 0, _hip.stream_ptr(x.device))
    return y


def planar(inputs, w, u_hat, b, per_sample=False):
    """Planar flow forward + logabsdet (reference no_analytic_inv/planar.py:30-49; with ``per_sample``
    the [N, D] / [N] parameters of ConditionalPlanarTransform, conditional.py:824-838)."""
    lib = _hip.load()
    x = _rows(inputs)
    _hip.require_no_grad(inputs)
    n, d = x.shape
    wv = _param(w, x.device, "w").reshape(-1)
    uv = _param(u_hat, x.device, "u").reshape(-1)
    bv = _param(b, x.device, "b").reshape(-1)
    _check_planar_parameters(wv, uv, bv, x, per_sample)
    y = torch.empty_like(x)
    lad = torch.empty(n, dtype=torch.float32, device=x.device)
    _call("fc_planar", lib.fc_planar, x.device, _hip.ptr(x), _hip.ptr(y), _hip.ptr(lad), _hip.ptr(wv),
          _hip.ptr(uv), _hip.ptr(bv), n, d, 1 if per_sample else 0, _hip.stream_ptr(x.device))
    return y, lad


PER_SAMPLE_DENSE, PER_SAMPLE_DENSE_T, PER_SAMPLE_LU_FORWARD, PER_SAMPLE_LU_INVERSE = 0, 1, 2, 3


def linear_per_sample(inputs, matrices, mode=PER_SAMPLE_DENSE, offdiag_scale=1.0, eps=0.0, want_logabsdet=False):
    """Per-sample ``[N, D, D]`` matrices applied to the rows of ``inputs`` (reference
    conditional.py:275-401): dense ``M x`` / ``M^T x`` or the LU forms built from raw hyper-network
    output on the fly.  Returns ``outputs`` or ``(outputs, logabsdet)``."""
    lib = _hip.load()
    x = _rows(inputs)
    m = _hip.dev_f32(matrices, "matrices")
    _hip.require_no_grad(inputs, matrices)
    n, d = x.shape
    _check_matrices(m, x)
    y = torch.empty_like(x)
    lad = torch.empty(n, dtype=torch.float32, device=x.device) if want_logabsdet else None
    _call("fc_linear_per_sample", lib.fc_linear_per_sample, x.device, _hip.ptr(x), _hip.ptr(y), _hip.ptr(lad),
          _hip.ptr(m), n, d, mode, float(offdiag_scale), float(eps), _hip.stream_ptr(x.device))
    return (y, lad) if want_logabsdet else y


class _LinearPerSampleFunction(torch.autograd.Function):
    """``linear_per_sample`` with its HIP backward kernel (``fc_linear_per_sample_backward``): gradients for the rows,
    the per-sample matrices (written once per row: no reduction) and a 0-dim ``offdiag_scale`` tensor (the sum of the
    kernel's per-row terms).  Saves the inputs -- for the LU inverse the OUTPUT -- and the matrices."""

    @staticmethod
    def forward(ctx, inputs, matrices, offdiag_scale, mode, eps):
        sp = float(offdiag_scale.detach()) if isinstance(offdiag_scale, torch.Tensor) else float(offdiag_scale)
        with torch.no_grad():
            outputs, logabsdet = linear_per_sample(inputs, matrices.detach(), mode=mode, offdiag_scale=sp, eps=eps,
                                                   want_logabsdet=True)
        ctx.save_for_backward(outputs if mode == PER_SAMPLE_LU_INVERSE else inputs, matrices)
        ctx.mode, ctx.sp, ctx.eps = mode, sp, eps
        ctx.sp_like = offdiag_scale if isinstance(offdiag_scale, torch.Tensor) and offdiag_scale.requires_grad else None
        if mode < PER_SAMPLE_LU_FORWARD:
            ctx.mark_non_differentiable(logabsdet)      # the dense forms have no log-determinant of their own (zeros)
        return outputs, logabsdet

    @staticmethod
    @torch.autograd.function.once_differentiable      # no double backward: create_graph=True raises instead of going silent
    def backward(ctx, grad_outputs, grad_logabsdet):
        saved, matrices = ctx.saved_tensors
        lib = _hip.load()
        x = _hip.dev_f32(saved, "inputs")
        m = _hip.dev_f32(matrices, "matrices")
        n, d = x.shape
        gy = _hip.dev_f32(grad_outputs.contiguous() if grad_outputs is not None else torch.zeros_like(x), "grad_outputs")
        lu = ctx.mode >= PER_SAMPLE_LU_FORWARD
        gl = _hip.dev_f32(grad_logabsdet.contiguous(), "grad_logabsdet") if lu and grad_logabsdet is not None else None
        gx = torch.empty_like(x)
        gm = torch.empty_like(m)
        gsp = torch.empty(n, dtype=torch.float32, device=x.device) if lu and ctx.sp_like is not None else None
        _call("fc_linear_per_sample_backward", lib.fc_linear_per_sample_backward, x.device, _hip.ptr(x), _hip.ptr(gy),
              _hip.ptr(gl), _hip.ptr(m), _hip.ptr(gx), _hip.ptr(gm), _hip.ptr(gsp), n, d, ctx.mode, ctx.sp, float(ctx.eps),
              _hip.stream_ptr(x.device))
        g_scale = None
        if ctx.sp_like is not None:
            g_scale = gsp.sum().to(ctx.sp_like.dtype).view_as(ctx.sp_like) if lu else torch.zeros_like(ctx.sp_like)
        return gx, gm, g_scale, None, None


def linear_per_sample_autograd(inputs, matrices, mode=PER_SAMPLE_DENSE, offdiag_scale=1.0, eps=0.0, want_logabsdet=False):
    """``linear_per_sample`` behind ``_LinearPerSampleFunction`` when a gradient is needed (``offdiag_scale`` may be a
    0-dim tensor with a graph; the kernel receives its float value); otherwise exactly ``linear_per_sample``."""
    scale_grad = isinstance(offdiag_scale, torch.Tensor) and offdiag_scale.requires_grad
    if torch.is_grad_enabled() and (inputs.requires_grad or matrices.requires_grad or scale_grad):
        x = _rows(inputs)
        m = _hip.dev_f32(matrices, "matrices")
        _check_matrices(m, x)
        if scale_grad:
            offdiag_scale = _hip.dev_f32(offdiag_scale, "offdiag_scale")
        outputs, logabsdet = _LinearPerSampleFunction.apply(x, m, offdiag_scale, mode, eps)
        return (outputs, logabsdet) if want_logabsdet else outputs
    return linear_per_sample(inputs, matrices, mode=mode, offdiag_scale=float(offdiag_scale), eps=eps,
                             want_logabsdet=want_logabsdet)


LINEAR_DENSE, LINEAR_LU_FORWARD, LINEAR_LU_INVERSE, LINEAR_DENSE_SHIFTED = 0, 1, 2, 3


def linear(inputs, a, b=None, bias=None, mode=LINEAR_DENSE):
    """Dense [D, D] maps on rows: ``A x + bias``; ``B (A x) + bias``; ``A^-1 B^-1 (x - bias)``; ``A (x - bias)``
    (reference linear.py:45-76, lu.py:56-91).  ``a``/``b`` are given untransposed."""
    lib = _hip.load()
    x = _rows(inputs)
    _hip.require_no_grad(inputs)
    n, d = x.shape
    at = _param(a, x.device, "weight").t().contiguous()
    bt = _param(b, x.device, "weight").t().contiguous() if b is not None else None
    if at.shape != (d, d) or (bt is not None and bt.shape != (d, d)):
        raise ValueError("weights must be [%d, %d]" % (d, d))
    bv = _param(bias, x.device, "bias").reshape(-1) if bias is not None else None
    y = torch.empty_like(x)
    _call("fc_linear", lib.fc_linear, x.device, _hip.ptr(x), _hip.ptr(y), _hip.ptr(at), _hip.ptr(bt),
          _hip.ptr(bv), n, d, mode, _hip.stream_ptr(x.device))
    return y


def _householder_backward(outputs, grad_outputs, q, reverse):
    """(grad_inputs, grad_q) of ``householder`` from its saved OUTPUT.  Shared q [K, D]: ``fc_householder_backward`` adds
    the batch's sum into a zeroed grad_q; per-sample q [N, K, D]: ``fc_householder_backward_per_sample`` writes every
    element of grad_q once."""
    lib = _hip.load()
    n, d = outputs.shape
    per_sample = q.dim() == 3
    entry = "fc_householder_backward_per_sample" if per_sample else "fc_householder_backward"
    gx = torch.empty_like(outputs)
    gq = torch.empty_like(q) if per_sample else torch.zeros_like(q)
    _call(entry, getattr(lib, entry), outputs.device, _hip.ptr(outputs), _hip.ptr(grad_outputs), _hip.ptr(q), _hip.ptr(gx),
          _hip.ptr(gq), n, d, q.shape[-2], 1 if reverse else 0, _hip.stream_ptr(outputs.device))
    return gx, gq


class _HouseholderFunction(torch.autograd.Function):
    """``householder`` with batch-shared q-vectors and its HIP backward kernel (``fc_householder_backward``: the
    reflections are involutions, so the saved OUTPUT is walked back to every intermediate)."""

    @staticmethod
    def forward(ctx, inputs, q_vectors, reverse):
        with torch.no_grad():
            outputs = householder(inputs, q_vectors, reverse=reverse)
        ctx.save_for_backward(outputs, q_vectors)
        ctx.reverse = reverse
        return outputs

    @staticmethod
    def backward(ctx, grad_outputs):
        outputs, q_vectors = ctx.saved_tensors
        gx, gq = _householder_backward(_hip.dev_f32(outputs, "outputs"), _hip.dev_f32(grad_outputs, "grad_outputs"),
                                       _hip.dev_f32(q_vectors.detach(), "q_vectors"), ctx.reverse)
        return gx, gq, None


class _HouseholderPerSampleFunction(torch.autograd.Function):
    """``householder`` with per-sample q-vectors ``[N, K, D]`` and its HIP backward kernel
    (``fc_householder_backward_per_sample``: the saved OUTPUT is walked back through the involutions with each row's own
    q block; the q gradient is written per row and reflection)."""

    @staticmethod
    def forward(ctx, inputs, q_vectors, reverse):
        with torch.no_grad():
            outputs = householder(inputs, q_vectors.detach(), reverse=reverse)
        ctx.save_for_backward(outputs, q_vectors)
        ctx.reverse = reverse
        return outputs

    @staticmethod
    @torch.autograd.function.once_differentiable      # no double backward: create_graph=True raises instead of going silent
    def backward(ctx, grad_outputs):
        outputs, q_vectors = ctx.saved_tensors
        gx, gq = _householder_backward(_hip.dev_f32(outputs, "outputs"),
                                       _hip.dev_f32(grad_outputs.contiguous(), "grad_outputs"),
                                       _hip.dev_f32(q_vectors, "q_vectors"), ctx.reverse)
        return gx, gq, None


def householder_autograd(inputs, q_vectors, reverse=False):
    """``householder`` -> (outputs, zeros); under autograd the shared-q form sits behind ``_HouseholderFunction`` and the
    per-sample form ``[N, K, D]`` behind ``_HouseholderPerSampleFunction``."""
    if torch.is_grad_enabled() and (inputs.requires_grad or q_vectors.requires_grad):
        if q_vectors.dim() == 2:
            x = _prep_2d(inputs)
            return _HouseholderFunction.apply(x, q_vectors, bool(reverse)), x.new_zeros(x.shape[0])
        if q_vectors.dim() == 3:
            x = _rows(inputs)
            q = _hip.dev_f32(q_vectors, "q_vectors")
            _check_q_vectors(q, x)
            return _HouseholderPerSampleFunction.apply(x, q, bool(reverse)), x.new_zeros(x.shape[0])
    return householder(inputs, q_vectors, reverse=reverse), inputs.new_zeros(inputs.shape[0])


HDH_MAX_REFLECTIONS = 4096      # ka + kb of fc_hdh_linear: the table of 2 / |q|^2 factors lives in LDS


def _hdh_operands(device, d, q_a, q_b, scale, pre, post):
    """(q_a, q_b, scale, pre, post) of ``fc_hdh_linear`` as device f32 tensors; an absent or empty sequence becomes
    ``None`` (a NULL pointer with a count of 0)."""
    qs = []
    for q, name in ((q_a, "q_a"), (q_b, "q_b")):
        if q is not None and q.shape[0] > 0:
            q = _hip.dev_f32(q.detach().to(device), name)
            if q.dim() != 2 or q.shape[1] != d:
                raise ValueError("%s of shape %s does not match %d features" % (name, tuple(q.shape), d))
        else:
            q = None
        qs.append(q)
    if sum(q.shape[0] for q in qs if q is not None) > HDH_MAX_REFLECTIONS:
        raise ValueError("flowconductor_amd: more than %d reflections in one fc_hdh_linear call" % HDH_MAX_REFLECTIONS)
    vecs = []
    for v, name in ((scale, "scale"), (pre, "pre"), (post, "post")):
        if v is not None:
            v = _hip.dev_f32(v.detach().to(device).reshape(-1), name)
            if v.numel() != d:
                raise ValueError("%s must have %d entries" % (name, d))
        vecs.append(v)
    if vecs[0] is None:
        raise ValueError("scale is required")
    return qs[0], qs[1], vecs[0], vecs[1], vecs[2]


def hdh_linear(inputs, q_a, q_b, scale, pre=None, post=None, reverse_a=False, reverse_b=False):
    """``post + H_b(scale * H_a(inputs - pre))`` in one launch (``fc_hdh_linear``): ``H_a`` / ``H_b`` the Householder
    sequences ``q_a [Ka, D]`` / ``q_b [Kb, D]`` (``None`` or empty: no reflection), each in index order or reversed;
    ``scale`` [D]; ``pre`` / ``post`` [D] or ``None``.  Both directions of ``SVDLinear`` (reference svd.py:56-95)."""
    lib = _hip.load()
    x = _rows(inputs)
    _hip.require_no_grad(inputs, q_a, q_b, scale, pre, post)
    n, d = x.shape
    qa, qb, sc, pr, po = _hdh_operands(x.device, d, q_a, q_b, scale, pre, post)
    y = torch.empty_like(x)
    _call("fc_hdh_linear", lib.fc_hdh_linear, x.device, _hip.ptr(x), _hip.ptr(y), _hip.ptr(qa), _hip.ptr(qb), _hip.ptr(sc),
          _hip.ptr(pr), _hip.ptr(po), n, d, 0 if qa is None else qa.shape[0], 0 if qb is None else qb.shape[0],
          1 if reverse_a else 0, 1 if reverse_b else 0, _hip.stream_ptr(x.device))
    return y


class _HDHLinearFunction(torch.autograd.Function):
    """``hdh_linear`` with its HIP backward kernel (``fc_hdh_linear_backward``): one node and one saved [N, D] tensor, the
    OUTPUT -- every stage of the map is invertible, so the kernel recovers the intermediates by walking back."""

    @staticmethod
    def forward(ctx, inputs, q_a, q_b, scale, pre, post, reverse_a, reverse_b):
        with torch.no_grad():
            outputs = hdh_linear(inputs, q_a, q_b, scale, pre, post, reverse_a, reverse_b)
        ctx.save_for_backward(outputs, q_a, q_b, scale, post)
        ctx.has_pre, ctx.reverse = pre is not None, (reverse_a, reverse_b)
        return outputs

    @staticmethod
    def backward(ctx, grad_outputs):
        outputs, q_a, q_b, scale, post = ctx.saved_tensors
        lib = _hip.load()
        y = _hip.dev_f32(outputs, "outputs")
        gy = _hip.dev_f32(grad_outputs, "grad_outputs")
        n, d = y.shape
        qa, qb, sc, _, po = _hdh_operands(y.device, d, q_a, q_b, scale, None, post)
        ka, kb = (0 if q is None else q.shape[0] for q in (qa, qb))
        gx = torch.empty_like(y)
        gpar = torch.zeros(ka + kb + 3, d, dtype=torch.float32, device=y.device)    # gq_a | gq_b | gscale | gpre | gpost
        gqa, gqb, gsc, gpr, gpo = gpar[:ka], gpar[ka:ka + kb], gpar[ka + kb], gpar[ka + kb + 1], gpar[ka + kb + 2]
        _call("fc_hdh_linear_backward", lib.fc_hdh_linear_backward, y.device, _hip.ptr(y), _hip.ptr(gy), _hip.ptr(qa),
              _hip.ptr(qb), _hip.ptr(sc), _hip.ptr(po), _hip.ptr(gx), _hip.ptr(gqa) if ka else None,
              _hip.ptr(gqb) if kb else None, _hip.ptr(gsc), _hip.ptr(gpr) if ctx.has_pre else None,
              _hip.ptr(gpo) if post is not None else None, n, d, ka, kb, 1 if ctx.reverse[0] else 0,
              1 if ctx.reverse[1] else 0, _hip.stream_ptr(y.device))
        return (gx, None if q_a is None else gqa.view_as(q_a), None if q_b is None else gqb.view_as(q_b), gsc.view_as(scale),
                gpr if ctx.has_pre else None, None if post is None else gpo.view_as(post), None, None)


def hdh_linear_autograd(inputs, q_a, q_b, scale, pre=None, post=None, reverse_a=False, reverse_b=False):
    """``hdh_linear``; under autograd one ``_HDHLinearFunction`` node (one launch forward, one backward)."""
    operands = (inputs, q_a, q_b, scale, pre, post)
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in operands):
        return _HDHLinearFunction.apply(_prep_2d(inputs), q_a, q_b, scale, pre, post, bool(reverse_a), bool(reverse_b))
    return hdh_linear(inputs, q_a, q_b, scale, pre, post, reverse_a, reverse_b)


def _planar_backward(x, grad_outputs, grad_logabsdet, wv, uv, bv, per_sample):
    """(gx, gw, gu, gb) of ``planar`` for device f32 operands.  Shared parameters [D] / [1]: ``fc_planar_backward`` adds
    the batch's sums into one zeroed buffer; per-sample [N, D] / [N]: ``fc_planar_backward_per_sample`` writes every
    element once."""
    lib = _hip.load()
    n, d = x.shape
    gy = _hip.dev_f32(grad_outputs if grad_outputs is not None else torch.zeros_like(x), "grad_outputs")
    gl = None if grad_logabsdet is None else _hip.dev_f32(grad_logabsdet, "grad_logabsdet")
    gx = torch.empty_like(x)
    if per_sample:
        entry = "fc_planar_backward_per_sample"
        gw, gu, gb = torch.empty_like(wv), torch.empty_like(uv), torch.empty_like(bv)
    else:
        entry = "fc_planar_backward"
        gpar = torch.zeros(2 * d + 1, dtype=torch.float32, device=x.device)      # gw | gu | gb, one zero fill
        gw, gu, gb = gpar[:d], gpar[d:2 * d], gpar[2 * d:]
    _call(entry, getattr(lib, entry), x.device, _hip.ptr(x), _hip.ptr(gy), _hip.ptr(gl), _hip.ptr(wv), _hip.ptr(uv),
          _hip.ptr(bv), _hip.ptr(gx), _hip.ptr(gw), _hip.ptr(gu), _hip.ptr(gb), n, d, _hip.stream_ptr(x.device))
    return gx, gw, gu, gb


class _PlanarFunction(torch.autograd.Function):
    """Shared-parameter ``planar`` with its HIP backward kernel (``fc_planar_backward``)."""

    @staticmethod
    def forward(ctx, inputs, w, u_hat, b):
        with torch.no_grad():
            outputs, logabsdet = planar(inputs, w, u_hat, b)
        ctx.save_for_backward(inputs, w, u_hat, b)
        return outputs, logabsdet

    @staticmethod
    def backward(ctx, grad_outputs, grad_logabsdet):
        inputs, w, u_hat, b = ctx.saved_tensors
        wv, uv, bv = (_hip.dev_f32(t.detach().reshape(-1), name) for t, name in ((w, "w"), (u_hat, "u"), (b, "b")))
        gx, gw, gu, gb = _planar_backward(_hip.dev_f32(inputs.detach(), "inputs"), grad_outputs, grad_logabsdet, wv, uv, bv,
                                          False)
        return gx, gw.view_as(w), gu.view_as(u_hat), gb.view_as(b)


class _PlanarPerSampleFunction(torch.autograd.Function):
    """``planar(per_sample=True)`` with its HIP backward kernel (``fc_planar_backward_per_sample``): ``w``, ``u_hat``
    ``[N, D]`` and ``b`` ``[N]`` per row, their gradients written per row."""

    @staticmethod
    def forward(ctx, inputs, w, u_hat, b):
        with torch.no_grad():
            outputs, logabsdet = planar(inputs, w.detach(), u_hat.detach(), b.detach(), per_sample=True)
        ctx.save_for_backward(inputs, w, u_hat, b)
        return outputs, logabsdet

    @staticmethod
    @torch.autograd.function.once_differentiable      # no double backward: create_graph=True raises instead of going silent
    def backward(ctx, grad_outputs, grad_logabsdet):
        x, wv, uv, bv = ctx.saved_tensors
        return _planar_backward(x, grad_outputs, grad_logabsdet, wv, uv, bv, True)


def planar_autograd(inputs, w, u_hat, b, per_sample=False):
    """Planar flow (no_analytic_inv/planar.py:30-49) with an autograd node when needed: shared parameters, or with
    ``per_sample`` the [N, D] / [N] parameters of ConditionalPlanarTransform (conditional.py:824-838)."""
    if torch.is_grad_enabled() and any(t.requires_grad for t in (inputs, w, u_hat, b)):
        if not per_sample:
            return _PlanarFunction.apply(_prep_2d(inputs), w, u_hat, b)
        x = _rows(inputs)
        n, d = x.shape
        wv, uv, bv = (_hip.dev_f32(t, name) for t, name in ((w, "w"), (u_hat, "u"), (b, "b")))
        _check_planar_parameters(wv, uv, bv, x, True)
        return _PlanarPerSampleFunction.apply(x, wv.reshape(n, d), uv.reshape(n, d), bv.reshape(n))
    return planar(inputs, w, u_hat, b, per_sample=per_sample)


class _SylvesterFunction(torch.autograd.Function):
    """Shared-parameter ``sylvester`` (no_analytic_inv/planar.py:144-166) with an explicit backward: the two Householder
    sequences through ``fc_householder`` / ``fc_householder_backward``, the products with R1 / R2 as library GEMMs, the
    tanh / log-determinant middle in ``fc_sylvester_mid_backward``."""

    @staticmethod
    def forward(ctx, inputs, q_vectors, r1, r2, bias):
        with torch.no_grad():
            outputs, logabsdet = sylvester(inputs, q_vectors, r1, r2, bias)
        ctx.save_for_backward(inputs, q_vectors, r1, r2, bias)
        return outputs, logabsdet

    @staticmethod
    def backward(ctx, grad_outputs, grad_logabsdet):
        inputs, q_vectors, r1, r2, bias = ctx.saved_tensors
        lib = _hip.load()
        with torch.no_grad():
            x = _hip.dev_f32(inputs.detach(), "inputs")
            q = _hip.dev_f32(q_vectors.detach(), "q_vectors")
            r1d, r2d, bd = r1.detach().float(), r2.detach().float(), bias.detach().float().reshape(-1)
            n, d = x.shape
            gy = _hip.dev_f32(grad_outputs if grad_outputs is not None else torch.zeros_like(x), "grad_outputs")
            gl = None if grad_logabsdet is None else _hip.dev_f32(grad_logabsdet, "grad_logabsdet")
            qtz = householder(x, q, reverse=True)                               # Q^T z
            pre = torch.addmm(bd, qtz, r1d.t())
            act = torch.tanh(pre)
            out = householder(act @ r2d.t(), q, reverse=False)                  # Q R2 act (saved output of that sequence)
            g_mid, gq_a = _householder_backward(out, gy, q, False)
            g_r2 = g_mid.t() @ act
            g_act = (g_mid @ r2d).contiguous()
            rd = (torch.diagonal(r1d) * torch.diagonal(r2d)).contiguous()
            sums = torch.zeros(2, d, dtype=torch.float32, device=x.device)        # g_bias | g_rd, one zero fill
            _call("fc_sylvester_mid_backward", lib.fc_sylvester_mid_backward, x.device, _hip.ptr(pre), _hip.ptr(g_act),
                  _hip.ptr(gl), _hip.ptr(rd), _hip.ptr(sums[0]), _hip.ptr(sums[1]), n, d, _hip.stream_ptr(x.device))
            g_pre = g_act
            g_r1 = g_pre.t() @ qtz
            g_x2, gq_b = _householder_backward(qtz, (g_pre @ r1d).contiguous(), q, True)
            g_r1.diagonal().add_(sums[1] * torch.diagonal(r2d))
            g_r2.diagonal().add_(sums[1] * torch.diagonal(r1d))
            return gy + g_x2, gq_a + gq_b, g_r1, g_r2, sums[0].view_as(bias)


def _sylvester_per_sample_composed(inputs, q_vectors, r1, r2, bias):
    """Per-sample Sylvester flow under autograd, composed of the per-sample nodes (no kernel of its own): the two
    Householder sequences and the two products with R1 / R2 (``PER_SAMPLE_DENSE``, which reads the zero triangle of the
    upper-triangular matrices too) on their HIP kernels, tanh and the log-determinant as torch ops on [N, D]."""
    qtz, _ = householder_autograd(inputs, q_vectors, reverse=True)                      # Q^T z
    act = torch.tanh(linear_per_sample_autograd(qtz, r1, mode=PER_SAMPLE_DENSE) + bias)
    rot, _ = householder_autograd(linear_per_sample_autograd(act, r2, mode=PER_SAMPLE_DENSE), q_vectors)
    rdiag = torch.diagonal(r1, dim1=-2, dim2=-1) * torch.diagonal(r2, dim1=-2, dim2=-1)
    return inputs + rot, torch.log(1 + (1 - act ** 2) * rdiag).sum(-1)


def sylvester_autograd(inputs, q_vectors, r1, r2, bias):
    """Sylvester flow (no_analytic_inv/planar.py:144-166) with autograd when needed: one node for shared parameters, the
    per-sample nodes composed for per-sample ones (``r1`` [N, D, D])."""
    if torch.is_grad_enabled() and any(t.requires_grad for t in (inputs, q_vectors, r1, r2, bias)):
        if r1.dim() == 3:
            return _sylvester_per_sample_composed(inputs, q_vectors, r1, r2, bias)
        return _SylvesterFunction.apply(_prep_2d(inputs), q_vectors, r1, r2, bias)
    return sylvester(inputs, q_vectors, r1, r2, bias)


def sylvester(inputs, q_vectors, r1, r2, bias):
    """Sylvester flow forward + logabsdet (reference no_analytic_inv/planar.py:144-166).

    Shared parameters: ``q [M, D]``, ``r1``/``r2`` ``[D, D]`` upper triangular, ``bias [D]``;
    per-sample: ``q [N, M, D]``, ``r1``/``r2`` ``[N, D, D]``, ``bias [N, D]``.

    The two forms read the matrices differently.  The shared form multiplies by EVERY entry of ``r1`` / ``r2`` (as
    ``pack_sylvester`` and ``sylvester_mm`` do), so the caller must pass matrices whose strict lower triangle is zero; an
    entry there enters the outputs, while the log-determinant is still that of the diagonal.  The per-sample form reads
    the upper triangle of every matrix only: whatever a hyper-network leaves below the diagonal is never fetched."""
    lib = _hip.load()
    x = _rows(inputs)
    _hip.require_no_grad(inputs)
    n, d = x.shape
    q = _param(q_vectors, x.device, "q_vectors")
    r1 = _param(r1, x.device, "R1")
    r2 = _param(r2, x.device, "R2")
    bv = _param(bias, x.device, "bias")
    per_sample = r1.dim() == 3
    if per_sample != (q.dim() == 3) or per_sample != (bv.dim() == 2):
        raise ValueError("q, R1, R2 and bias must all be shared or all be per-sample")
    rdiag = (torch.diagonal(r1, dim1=-2, dim2=-1) * torch.diagonal(r2, dim1=-2, dim2=-1)).contiguous()
    if per_sample:
        # [N, D, D] row-major exactly as the hyper-network emits them: the kernel reads each row's upper part once
        # (a transposed copy would cost two more passes over 2 x N x D x D floats)
        r1t, r2t = r1.contiguous(), r2.contiguous()
    else:
        r1t = r1.transpose(-1, -2).contiguous()
        r2t = r2.transpose(-1, -2).contiguous()
    y = torch.empty_like(x)
    lad = torch.empty(n, dtype=torch.float32, device=x.device)
    _call("fc_sylvester", lib.fc_sylvester, x.device, _hip.ptr(x), _hip.ptr(y), _hip.ptr(lad), _hip.ptr(q),
          _hip.ptr(r1t), _hip.ptr(r2t), _hip.ptr(bv), _hip.ptr(rdiag), n, d, q.shape[-2],
          1 if per_sample else 0, _hip.stream_ptr(x.device))
    return y, lad


SYLVESTER_INVERSE_MAX_FEATURES = 128      # fc_sylvester_inverse keeps 2 * D * 256 bytes of LDS per wavefront


def sylvester_inverse_supported(n, d):
    """Shapes of the Sylvester back-substitution kernel (shared parameters only)."""
    return 1 <= d <= SYLVESTER_INVERSE_MAX_FEATURES and n >= 0


def _rotate(x, q, reverse, matrix):
    """``householder(x, q, reverse)``; with ``matrix`` (the reflections folded into a dense [D, D] weight) the rows that
    fill whole 16-row tiles go through the matrix cores instead."""
    n, d = x.shape
    if matrix is None or not sylvester_mm_supported(n, d):
        return householder(x, q, reverse=reverse)
    body = n - n % SYLVESTER_MM_ROWS
    out = dense_mm(x[:body], matrix)
    if body < n:
        out = torch.cat((out, householder(x[body:], q, reverse=reverse)))
    return out


def sylvester_inverse(inputs, q_vectors, r1, r2, bias, q_matrices=None):
    """Inverse of ``sylvester`` with shared parameters -> ``(z, logabsdet)`` (the reference has none).

    Three steps: ``c = Q^T y`` (the reflections in reverse order), the back substitution ``fc_sylvester_inverse`` of
    ``c = v + R2 tanh(R1 v + bias)`` in those coordinates, ``z = Q v`` (the reflections in index order).  ``q_matrices``:
    optional ``(weight of Q^T, weight of Q)`` for ``dense_mm`` (``householder_matrix(q, reverse).T`` as float32), used
    where ``sylvester_mm_supported`` holds.  At most ``SYLVESTER_INVERSE_MAX_FEATURES`` features."""
    lib = _hip.load()
    y = _rows(inputs)
    _hip.require_no_grad(inputs)
    n, d = y.shape
    if not sylvester_inverse_supported(n, d):
        raise ValueError("fc_sylvester_inverse: %d features exceed the %d supported" % (d, SYLVESTER_INVERSE_MAX_FEATURES))
    q = _param(q_vectors, y.device, "q_vectors")
    r1 = _param(r1, y.device, "R1")
    r2 = _param(r2, y.device, "R2")
    bv = _param(bias, y.device, "bias").reshape(-1)
    if q.dim() != 2 or q.shape[1] != d or r1.shape != (d, d) or r2.shape != (d, d) or bv.numel() != d:
        raise ValueError("sylvester_inverse takes shared parameters: q [M, %d], R1 / R2 [%d, %d], bias [%d]" % (d, d, d, d))
    lad = torch.empty(n, dtype=torch.float32, device=y.device)
    if n == 0:
        return torch.empty_like(y), lad
    m_rev, m_fwd = q_matrices if q_matrices is not None else (None, None)
    r1t, r2t = r1.t().contiguous(), r2.t().contiguous()
    c = _rotate(y, q, True, m_rev)
    v = torch.empty_like(c)
    _call("fc_sylvester_inverse", lib.fc_sylvester_inverse, y.device, _hip.ptr(c), _hip.ptr(v), _hip.ptr(lad),
          _hip.ptr(r1t), _hip.ptr(r2t), _hip.ptr(bv), n, d, _hip.stream_ptr(y.device))
    return _rotate(v, q, False, m_fwd), lad


SYLVESTER_MM_ROWS = 16


def sylvester_mm_supported(n, d):
    """Shapes of the matrix-core Sylvester kernel (shared parameters only)."""
    return d % 32 == 0 and d <= 128 and n >= SYLVESTER_MM_ROWS


def dense_mm(inputs, weight, bias=None, pre=None):
    """``inputs @ weight.T + bias`` -- or ``(inputs - pre) @ weight.T + bias`` -- for a batch-independent [D, D]
    ``weight`` on the matrix cores (rows a multiple of 16, D % 32 == 0, D <= 128): f32-GEMM accuracy by split-f16
    products.  The shift is subtracted in f32 inside the kernel, before the product."""
    lib = _hip.load()
    x = _rows(inputs, align16=True)
    _hip.require_no_grad(inputs)
    n, d = x.shape
    if n % SYLVESTER_MM_ROWS != 0 or not sylvester_mm_supported(n, d):
        raise ValueError("fc_dense_mm: unsupported shape %s" % (tuple(x.shape),))
    w = _aligned16(_param(weight, x.device, "weight"))
    if w.shape != (d, d):
        raise ValueError("weight must be [%d, %d]" % (d, d))
    bv = _param(bias, x.device, "bias").reshape(-1) if bias is not None else None
    y = torch.empty_like(x)
    if pre is None:
        _call("fc_dense_mm", lib.fc_dense_mm, x.device, _hip.ptr(x), _hip.ptr(y), _hip.ptr(w), _hip.ptr(bv), n, d,
              _hip.stream_ptr(x.device))
        return y
    pv = _param(pre, x.device, "pre").reshape(-1)
    if pv.numel() != d or (bv is not None and bv.numel() != d):
        raise ValueError("pre / bias must have %d entries" % d)
    _call("fc_dense_mm_shifted", lib.fc_dense_mm_shifted, x.device, _hip.ptr(x), _hip.ptr(y), _hip.ptr(w),
          _hip.ptr(pv), _hip.ptr(bv), n, d, _hip.stream_ptr(x.device))
    return y


def sylvester_mm(inputs, w1, w2, bias, rdiag):
    """Sylvester flow forward + logabsdet with shared parameters as two matrix-core products (rows a multiple of 16)."""
    lib = _hip.load()
    x = _rows(inputs, align16=True)
    _hip.require_no_grad(inputs)
    n, d = x.shape
    if n % SYLVESTER_MM_ROWS != 0 or not sylvester_mm_supported(n, d):
        raise ValueError("fc_sylvester_mm: unsupported shape %s" % (tuple(x.shape),))
    bv = _param(bias, x.device, "bias")
    w1, w2 = _aligned16(_hip.dev_f32(w1, "w1")), _aligned16(_hip.dev_f32(w2, "w2"))
    y = torch.empty_like(x)
    lad = torch.empty(n, dtype=torch.float32, device=x.device)
    _call("fc_sylvester_mm", lib.fc_sylvester_mm, x.device, _hip.ptr(x), _hip.ptr(y), _hip.ptr(lad), _hip.ptr(w1),
          _hip.ptr(w2), _hip.ptr(bv), _hip.ptr(rdiag), n, d, _hip.stream_ptr(x.device))
    return y, lad
