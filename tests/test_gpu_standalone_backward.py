"""The four stand-alone backward entries against float64 autograd, slice by slice and on every launch path
(tests/_standalone_backward_util.py; its truth is checked without a GPU in tests/test_standalone_backward_host.py):

rq      ``fc_rq_spline_backward`` at operator level (``ops.rq_spline_backward``: misaligned buffers, no grad_logabsdet): every
        instantiation (K = 4, 8, 16 compiled in, 5, 10, 32 at run time, both tail modes) on the wave kernel and below its
        threshold; the wave kernel plus leftover rows, its scalar strip, G = 1, 2, 64, the three fall-backs to the generic
        kernel, a second grid-stride trip of either kernel, the edges of the interval and of the activations; one case through
        ``ops.rq_spline_autograd``;
spline  ``fc_piecewise_spline_backward`` under ``ops.piecewise_spline_autograd``: every (kind, tails) at K = 3, a middle value
        and the largest supported one at (d, d_t, n) = (5, 3, 400); at the middle K also (4, 4, 257) with all columns,
        (3, 1, 130), and the rows on the ends of the interval and beyond the tails; a second grid-stride trip;
sos     ``fc_sum_of_sigmoids_backward`` under ``ops.sum_of_sigmoids_autograd``: the LDS-tile kernel up to S = 159 (whole and
        partly filled groups, its 160 KB tile, a second trip), the direct kernel from S = 160, no grad_logabsdet, a
        log_scale_postact, saturated rows;
affine  ``fc_affine_backward`` under ``ops.affine_coupling``: seven activations x (column subset, all columns, d_t = 1), the
        rows at which an activation changes branch, a second grid-stride trip.

Every case first asserts with the route predictors that it lies on the path it is named for, and prints its figures
(``pytest -s``) before it asserts: the worst err / bound and the worst err / floor per kind of slice."""
import pytest
import torch

import _standalone_backward_util as U
import _tile_util
from flowconductor_amd import ops
from flowconductor_amd.ops import sigmoids as sigmoid_ops

pytestmark = pytest.mark.gpu


def _cus(device):
    return torch.cuda.get_device_properties(device).multi_processor_count


def _inputs(cs, device):
    """(x [n, d], params [n, d_t P], cols, gy [n, d], gl [n] or None) on the device, the distinct rows repeated there."""
    idx = None if cs.idx is None else cs.idx.to(device)

    def rows(t):
        if t is None:
            return None
        t = t.to(device)
        return t if idx is None else t[idx].contiguous()

    cols = None if cs.cols is None else cs.cols.to(device)
    return rows(cs.x), rows(cs.params), cols, rows(cs.gy), rows(cs.gl)


def _backward_through(fn, x, params, gy, gl):
    xg, pg = x.requires_grad_(True), params.requires_grad_(True)
    y, lad = fn(xg, pg)
    total = (y * gy).sum()
    if gl is not None:
        total = total + (lad * gl).sum()
    total.backward()
    return xg.grad, pg.grad


def _launch(cs, device, cus):
    """(gx [n, d], gp [n, d_t P]) of the entry's HIP backward kernel, after the route assertion."""
    spec = cs.spec
    x, params, cols, gy, gl = _inputs(cs, device)
    if spec.variant == "mis_x":
        x, gy = _tile_util.misaligned(x, device), _tile_util.misaligned(gy, device)
    elif spec.variant == "mis_p":
        params = _tile_util.misaligned(params, device)
    aligned_rows = x.data_ptr() % 16 == 0 and gy.data_ptr() % 16 == 0
    reached = U.branches(spec, cus, aligned_rows, params.data_ptr() % 16 == 0)
    missing = [b for b in spec.named if b not in reached]
    assert not missing, (cs.id, missing, sorted(reached))
    assert reached == U.branches(U.SPECS[cs.id]), (cs.id, sorted(reached))      # the table the host file checks, on this device
    if cs.entry == "rq":
        kw = U.rq_kwargs(spec)
        if spec.variant == "autograd":
            gx, gp = _backward_through(lambda a, b: ops.rq_spline_autograd(a, b, cols, **kw), x, params, gy, gl)
            return gx, gp
        return ops.rq_spline_backward(x, params, cols, gy, gl, **kw)
    if cs.entry == "spline":
        kw = U.spline_kwargs(spec)
        return _backward_through(lambda a, b: ops.piecewise_spline_autograd(a, b, cols, **kw), x, params, gy, gl)
    if cs.entry == "sos":
        s, log_post = cs.cfg["s"], cs.cfg.get("log_post", 0.0)
        if spec.variant == "gl_none":
            # autograd hands a custom node zeros for an unused output: the operator itself, with no grad_logabsdet
            return sigmoid_ops.sum_of_sigmoids_backward(x, params, gy, None, s, log_post)
        if spec.variant == "postact":
            return _backward_through(lambda a, b: sigmoid_ops._SoSFunction.apply(a, b, s, 0.0, log_post), x, params, gy, gl)
        return _backward_through(lambda a, b: ops.sum_of_sigmoids_autograd(a, b, s), x, params, gy, gl)
    code = U.AFFINE_ACTS[cs.cfg["act"]]
    return _backward_through(lambda a, b: ops.affine_coupling(a, b, cols, activation=code), x, params, gy, gl)


def _run(cid, device):
    """Launch case ``cid`` and compare it slice by slice; returns (case, gx [R, d], gp [R, d_t P]) of the distinct rows on the
    CPU."""
    cus = _cus(device)
    cs = U.with_cus(U.case(cid), cus)
    gx, gp = _launch(cs, device, cus)
    torch.cuda.synchronize(device)
    r = cs.distinct
    gp = gp.reshape(cs.n, -1)
    assert gx.shape == (cs.n, cs.d) and gp.shape == (cs.n, cs.params.shape[1])
    if cs.idx is not None:          # every row equals the first appearance of its source row, bit for bit
        idx = cs.idx.to(device)
        assert torch.equal(gx, gx[:r][idx]) and torch.equal(gp, gp[:r][idx]), cid
    gx, gp = gx[:r].cpu(), gp[:r].cpu()
    ident = U.identity_columns(cs)
    assert torch.equal(gx[:, ident], cs.gy[:, ident]), cid
    failures = []
    for kind, res in U.check(cs, gx[:, U.tcols(cs)], gp):
        print("standalone-backward %s %s %s: err/bound %.3f err/floor %.2f (%s)"
              % (cs.entry, cid, kind, res.worst, res.worst_floor, res.detail))
        if not res.ok:
            failures.append((kind, res.detail))
    assert not failures, (cid, failures)
    return cs, gx, gp


def _outside_rows_are_the_identity(cs, gx, gp):
    if cs.cfg["tails"]:
        rows = [U.ROW_ABOVE, U.ROW_BELOW]
        assert torch.equal(gx[rows], cs.gy[rows]) and float(gp[rows].abs().max()) == 0.0


# ---- rq ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cid", U.ids("rq", "plain", "-d12-dt8-n51"))
def test_rq_every_instantiation(cid, device):
    _run(cid, device)


_RQ_ROUTES = [i for i in U.ids("rq") if "-d12-dt8-n51" not in i and U.SPECS[i].variant not in ("edges", "autograd")]


@pytest.mark.parametrize("cid", _RQ_ROUTES)
def test_rq_launch_routes(cid, device):
    _run(cid, device)


@pytest.mark.parametrize("cid", U.ids("rq", "edges"))
def test_rq_edges(cid, device):
    """Rows on the ends of the interval (gl = 0: gp = 0 in exact arithmetic, gx = gy d_end), beyond the tails (the identity,
    exactly), a derivative logit above the softplus threshold, a saturated width softmax, all logits equal."""
    cs, gx, gp = _run(cid, device)
    _outside_rows_are_the_identity(cs, gx, gp)


def test_rq_through_the_autograd_node(device):
    _run("rq-K8-tails-autograd", device)


# ---- piecewise splines ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cid", U.ids("spline", "plain"))
def test_piecewise_splines(cid, device):
    _run(cid, device)


@pytest.mark.parametrize("cid", U.ids("spline", "edges"))
def test_piecewise_spline_edges(cid, device):
    cs, gx, gp = _run(cid, device)
    _outside_rows_are_the_identity(cs, gx, gp)


@pytest.mark.parametrize("name", list(U.KNOT_CASES))
def test_piecewise_spline_gradients_at_the_knots(name, device):
    """x on the float32 rounding of every interior knot and on its four float32 neighbours on either side -- the elements
    every case above leaves out.  Each element's (gx, gp) must be the float64 gradient of the bin on the left of the knot or
    of the bin on the right (``U.check_knots``: taken at x -+ 2^-16 of the interval); no element is left out."""
    cs = U.knot_case(name)
    kw = U.spline_kwargs(cs.spec)
    gx, gp = _backward_through(lambda a, b: ops.piecewise_spline_autograd(a, b, None, **kw), cs.x.to(device),
                               cs.params.to(device), cs.gy.to(device), cs.gl.to(device))
    torch.cuda.synchronize(device)
    ok, worst, detail = U.check_knots(name, gx.cpu(), gp.reshape(cs.n, -1).cpu())
    print("standalone-backward spline %s at the knots: err/bound %.3f (%s)" % (cs.id, worst, detail))
    assert ok, (cs.id, detail)


# ---- sum of sigmoids -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cid", U.ids("sos"))
def test_sum_of_sigmoids(cid, device):
    _run(cid, device)


# ---- affine family -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cid", U.ids("affine"))
def test_affine_family(cid, device):
    cs, gx, gp = _run(cid, device)
    if cs.spec.variant == "edges" and cs.cfg["act"] == "softplus_clamp3":
        # softplus + 1e-3 above 3: the clamp passes no gradient to the raw scale
        scale_grad = gp[:, cs.d_t:]
        assert float(scale_grad[[U.AFFINE_ROW_ABOVE20, U.AFFINE_ROW_CLAMPED]].abs().max()) == 0.0
