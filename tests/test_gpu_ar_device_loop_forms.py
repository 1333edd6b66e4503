"""The one-kernel inverse of the sum-of-sigmoids and sibling-spline autoregressive layers (fc_made_inverse_sos,
fc_made_inverse_spline) against the oracle's D full passes (autoregressive.py:44-53) in float32 and float64 and against
this package's own host loop (options ar_device_loop = False)."""
import copy

import pytest
import torch

from _util import maxdiff
from flowconductor_amd import options
from oracle import torch_oracle as O

pytestmark = pytest.mark.gpu

ENTRIES = ("fc_made_inverse_sos", "fc_made_inverse_spline")

# (kind, bins / sigmoids, D, hidden, blocks, N, seed): every parameter-tile count (P = 8 .. 91), both k-step counts of the
# initial layer, 1-3 blocks, batches that are not whole 16-row blocks.  The seeds are part of the fixtures: on other seeds the
# quadratic K = 6 and cubic K = 6 shapes are ill-conditioned in the reference's own float32 (2e-2 from float64).
CASES = [
    ("sos", 6, 6, 64, 2, 1000, 70), ("sos", 30, 8, 64, 2, 200, 72), ("sos", 10, 40, 50, 2, 333, 90),
    ("sos", 3, 5, 24, 1, 77, 29), ("sos", 15, 7, 32, 3, 160, 39), ("sos", 30, 64, 64, 2, 96, 128),
    ("linear", 8, 6, 64, 2, 1000, 70), ("linear", 20, 33, 24, 2, 200, 57),
    ("quadratic_tails", 6, 6, 64, 2, 1000, 2), ("quadratic", 10, 5, 24, 2, 77, 1), ("quadratic_tails", 20, 33, 24, 2, 200, 2),
    ("cubic", 6, 6, 64, 2, 1000, 4), ("cubic", 10, 9, 16, 1, 50, 2)]
PER_DIM = {"sos": lambda k: 3 * k + 1, "linear": lambda k: k, "quadratic_tails": lambda k: 2 * k - 1,
           "quadratic": lambda k: 2 * k + 1, "cubic": lambda k: 2 * k + 2}


def _entry(kind):
    return ENTRIES[0] if kind == "sos" else ENTRIES[1]


def _build(kind, k, features, hidden, blocks, seed, **kw):
    from flowconductor_amd import transforms as T

    torch.manual_seed(seed)
    kw = dict(num_blocks=blocks, **kw)
    if kind == "sos":
        t = T.MaskedSumOfSigmoidsTransform(features, hidden, n_sigmoids=k, **kw)
    elif kind == "linear":
        t = T.MaskedPiecewiseLinearAutoregressiveTransform(k, features, hidden, **kw)
    elif kind == "quadratic_tails":
        t = T.MaskedPiecewiseQuadraticAutoregressiveTransform(k, features, hidden, tails="linear", tail_bound=3.0, **kw)
    elif kind == "quadratic":
        t = T.MaskedPiecewiseQuadraticAutoregressiveTransform(k, features, hidden, **kw)
    else:
        t = T.MaskedPiecewiseCubicAutoregressiveTransform(k, features, hidden, **kw)
    t = t.eval()
    with torch.no_grad():
        for p in t.parameters():
            p.mul_(1.5)
    return t


def _inputs(kind, n, features):
    """The inputs of tests/test_gpu_ar_inverse.py::_inputs."""
    g = torch.Generator().manual_seed(5)
    if kind == "sos":
        return torch.randn(n, features, generator=g) * 0.6
    if kind == "quadratic_tails":
        return torch.randn(n, features, generator=g) * 1.2
    return torch.rand(n, features, generator=g) * 0.98 + 0.01


_REFS = {}


def _references(key, t, x, context=None):
    """Oracle inverse in float32 and float64 (computed once per fixture), the project's bounds for this kernel family, and
    the conditions on the fixture itself: an ill-conditioned one makes both bounds vacuous."""
    if key not in _REFS:
        with torch.no_grad():
            y32, lad32 = O.transform_apply(t, x.clone(), context, inverse=True)
            y64, lad64 = O.transform_apply(copy.deepcopy(t).double(), x.double(), None if context is None else context.double(),
                                           inverse=True)
        _REFS[key] = (y32, lad32, y64, lad64)
    y32, lad32, y64, lad64 = _REFS[key]
    assert float(y64.abs().max()) <= 100, "fixture: the float64 inverse leaves the usable range"
    assert maxdiff(y32, y64) <= 2e-4 * max(1.0, float(y64.abs().max())), "fixture: the float32 oracle is itself far off"
    tol_y = 1e-4 * max(1.0, float(y32.abs().max())) + 4 * maxdiff(y32, y64)
    tol_l = 1e-3 * max(1.0, float(lad32.abs().max()) / 10) + 4 * maxdiff(lad32, lad64)
    return y64, lad64, tol_y, tol_l


def _timed_inverse(t, x, context=None):
    """``t.inverse`` and the launches of the two new entries and of fc_made_inverse it issued."""
    from flowconductor_amd import ops

    with ops.KernelTimer(ENTRIES[0]) as sos, ops.KernelTimer(ENTRIES[1]) as spline, ops.KernelTimer("fc_made_inverse") as old:
        y, lad = t.inverse(x, context)
    return y, lad, {ENTRIES[0]: len(sos.pairs), ENTRIES[1]: len(spline.pairs), "fc_made_inverse": len(old.pairs)}


@pytest.mark.parametrize("kind,k,features,hidden,blocks,n,seed", CASES)
def test_device_loop_forms_match_the_reference_scheme(kind, k, features, hidden, blocks, n, seed, device):
    from flowconductor_amd import ops

    t = _build(kind, k, features, hidden, blocks, seed)
    x = _inputs(kind, n, features)
    ref_y64, ref_lad64, tol_y, tol_l = _references((kind, k, features, hidden, blocks, n, seed), t, x)
    t = t.to(device)
    xd = x.to(device)
    assert t._device_loop_form()[1] == PER_DIM[kind](k)
    assert ops.made_inverse_form_fits(features, blocks, PER_DIM[kind](k))
    with torch.no_grad():
        assert t._device_loop_ok(xd, None)
        y, lad, launches = _timed_inverse(t, xd)
        other = ENTRIES[1] if kind == "sos" else ENTRIES[0]
        assert launches == {_entry(kind): 1, other: 0, "fc_made_inverse": 0}
        with options.override(ar_device_loop=False):
            assert not t._device_loop_ok(xd, None)
            y_host, lad_host, host_launches = _timed_inverse(t, xd)
        assert not any(host_launches.values())
        z, lad_fwd = t.forward(y)
    errors = {"y vs float64": maxdiff(y, ref_y64) / tol_y, "lad vs float64": maxdiff(lad, ref_lad64) / tol_l,
              "y vs host loop": maxdiff(y, y_host) / tol_y, "lad vs host loop": maxdiff(lad, lad_host) / tol_l,
              "round trip y": maxdiff(z, x) / (2 * tol_y),
              "round trip lad": maxdiff(lad + lad_fwd, torch.zeros_like(lad)) / (2 * tol_l)}
    worst = max(errors, key=errors.get)
    print("device loop %s k=%d D=%d H=%d blocks=%d N=%d: worst error / bound %.3f (%s), tol_y %.3g tol_l %.3g"
          % (kind, k, features, hidden, blocks, n, errors[worst], worst, tol_y, tol_l))
    assert errors[worst] <= 1.0, errors


def test_rows_do_not_depend_on_the_batch(device):
    """S = 30: the first 77 rows of a 1000-row call equal a 77-row call bitwise (each wave works on its own 16 rows); N = 1
    and N = 17 run; a call repeats itself bitwise.  Every call here is far below 256 rows per CU, so only the
    one-block-per-wave form runs: the two-blocks-per-wave form against the same rows on the one-block form is
    tests/test_gpu_ar_sampler_rows.py::test_rows_of_the_two_block_route_against_float64."""
    t = _build("sos", 30, 8, 64, 2, 72).to(device)
    x = _inputs("sos", 1000, 8).to(device)
    with torch.no_grad():
        y, lad, launches = _timed_inverse(t, x)
        assert launches[ENTRIES[0]] == 1
        y2, lad2, _ = _timed_inverse(t, x)
        assert torch.equal(y, y2) and torch.equal(lad, lad2)
        for n in (77, 17, 1):
            y_n, lad_n, launches = _timed_inverse(t, x[:n].contiguous())
            assert launches[ENTRIES[0]] == 1 and y_n.shape == (n, 8) and lad_n.shape == (n,)
            assert torch.equal(y_n, y[:n]) and torch.equal(lad_n, lad[:n])


@pytest.mark.parametrize("kind,k,features,hidden,blocks", [("sos", 30, 8, 64, 2), ("cubic", 10, 33, 40, 3)])
def test_prefix_passes_equal_whole_passes(kind, k, features, hidden, blocks, device):
    """units_needed against the same kernel computing all 64 units in every pass (the bounds of
    test_device_loop_prefix_passes_equal_whole_passes)."""
    from flowconductor_amd import ops

    t = _build(kind, k, features, hidden, blocks, features).to(device)
    form, per_dim, kw = t._device_loop_form()
    z = _inputs(kind, 1024 + 16, features).to(device)
    with torch.no_grad():
        packed = ops.pack_made_inverse(t.autoregressive_net, features, per_dim)
        need = packed[-1]
        assert int(need[0]) == 0 and int(need.max()) <= hidden and bool((need[1:] >= need[:-1]).all())
        with ops.KernelTimer(_entry(kind)) as timer:
            y, lad = ops.made_inverse(z, packed, blocks, per_dim, form, kw)
            whole = packed[:-1] + (torch.full_like(need, 64),)
            y_all, lad_all = ops.made_inverse(z, whole, blocks, per_dim, form, kw)
        assert len(timer.pairs) == 2
        y_t, lad_t = t.inverse(z)
    assert maxdiff(y, y_all) <= 2e-6 * max(1.0, float(y_all.abs().max()))
    assert maxdiff(lad, lad_all) <= 2e-5 * max(1.0, float(lad_all.abs().max()) / 10)
    assert maxdiff(y, y_t) <= 1e-6 and maxdiff(lad, lad_t) <= 1e-5      # (the transform's own call: same kernel, same pack)


# (name, kind, k, D, hidden, blocks, N, seed, constructor arguments): shapes and conditioners the entries do not take
ASIDE = [
    ("tanh", "sos", 6, 6, 32, 2, 77, 70, dict(activation=torch.tanh)),
    ("feed_forward_blocks", "cubic", 6, 6, 32, 2, 77, 4, dict(use_residual_blocks=False, random_mask=True)),
    ("d65", "linear", 8, 65, 64, 1, 32, 70, {}),
    ("lds", "sos", 30, 40, 64, 3, 32, 72, {}),
    ("s33", "sos", 33, 5, 32, 2, 48, 72, {})]


@pytest.mark.parametrize("name,kind,k,features,hidden,blocks,n,seed,kw", ASIDE, ids=[c[0] for c in ASIDE])
def test_shapes_outside_the_kernel_keep_the_host_loop(name, kind, k, features, hidden, blocks, n, seed, kw, device):
    t = _build(kind, k, features, hidden, blocks, seed, **kw)
    x = _inputs(kind, n, features)
    ref_y64, ref_lad64, tol_y, tol_l = _references(("aside", name), t, x)
    t = t.to(device)
    with torch.no_grad():
        assert not t._device_loop_ok(x.to(device), None)
        y, lad, launches = _timed_inverse(t, x.to(device))
    assert not any(launches.values())
    assert maxdiff(y, ref_y64) <= tol_y and maxdiff(lad, ref_lad64) <= tol_l


def test_options_autograd_and_float64_keep_the_host_loop(device):
    from flowconductor_amd import ops

    t = _build("sos", 6, 6, 64, 2, 70)
    x = _inputs("sos", 77, 6)
    ref_y64, ref_lad64, tol_y, tol_l = _references(("aside", "routes"), t, x)
    t = t.to(device)
    xd = x.to(device)
    # autograd on (the parameters require gradients)
    assert not t._device_loop_ok(xd, None)
    y, lad, launches = _timed_inverse(t, xd)
    assert not any(launches.values()) and y.requires_grad
    assert maxdiff(y, ref_y64) <= tol_y and maxdiff(lad, ref_lad64) <= tol_l
    with torch.no_grad():
        assert t._device_loop_ok(xd, None)
        for off in (dict(ar_device_loop=False), dict(fused_hidden=False)):
            with options.override(**off):
                assert not t._device_loop_ok(xd, None)
                y, lad, launches = _timed_inverse(t, xd)
            assert not any(launches.values())
            assert maxdiff(y, ref_y64) <= tol_y and maxdiff(lad, ref_lad64) <= tol_l
        # float64 rows: not the kernel's.  The host loop hands them to the float32 conditioner's first masked linear layer,
        # where PyTorch refuses the mixed product (as on the parent, and on the CPU): nothing of the new entries is launched
        assert not t._device_loop_ok(xd.double(), None)
        with ops.KernelTimer(ENTRIES[0]) as sos, ops.KernelTimer(ENTRIES[1]) as spline:
            with pytest.raises(RuntimeError, match="dtype"):
                t.inverse(xd.double())
        assert not sos.pairs and not spline.pairs


def test_very_large_sum_of_sigmoids_batches_keep_the_host_loop(device):
    """Beyond rows x sigmoids = 30 x 2^16 the host loop is the faster route; the splines have no such limit.
    (The route's predicate only: the host loop itself is covered above.)"""
    t = _build("sos", 30, 8, 64, 2, 72).to(device)
    c = _build("cubic", 10, 9, 16, 1, 2).to(device)
    with torch.no_grad():
        assert t._device_loop_ok(torch.zeros(1 << 16, 8, device=device), None)
        assert not t._device_loop_ok(torch.zeros((1 << 16) + 1, 8, device=device), None)
        assert c._device_loop_ok(torch.zeros(1 << 18, 9, device=device), None)


@pytest.mark.parametrize("kind,k", [("sos", 6), ("cubic", 6)])
def test_a_context_keeps_the_host_loop(kind, k, device):
    """A MADE with context layers, called with a context: these forms have no conditional device loop."""
    t = _build(kind, k, 6, 32, 2, 4, context_features=3)
    x = _inputs(kind, 77, 6)
    c = torch.randn(77, 3, generator=torch.Generator().manual_seed(6))
    ref_y64, ref_lad64, tol_y, tol_l = _references(("aside", "context", kind), t, x, c)
    t = t.to(device)
    with torch.no_grad():
        assert not t._device_loop_ok(x.to(device), c.to(device))
        assert not t._device_loop_ok(x.to(device), None)          # (a net with context layers called without one)
        y, lad, launches = _timed_inverse(t, x.to(device), c.to(device))
    assert not any(launches.values())
    assert maxdiff(y, ref_y64) <= tol_y and maxdiff(lad, ref_lad64) <= tol_l


def test_outside_the_box_raises_like_the_host_loop(device):
    """A piecewise-linear layer lives on [0, 1]: an input of 1.5 sets the kernel's error word, which raises what the host
    loop raises (no device fault is involved)."""
    from flowconductor_amd import transforms as T

    t = _build("linear", 8, 6, 64, 2, 70).to(device)
    x = _inputs("linear", 64, 6)
    x[5, 3] = 1.5
    xd = x.to(device)
    with torch.no_grad():
        assert t._device_loop_ok(xd, None)
        with pytest.raises(T.InputOutsideDomain) as on_device:
            t.inverse(xd)
        with options.override(ar_device_loop=False), pytest.raises(T.InputOutsideDomain) as on_host:
            t.inverse(xd)
    assert on_device.type is on_host.type


def test_flow_samples_with_one_launch_per_layer(device):
    from flowconductor_amd import distributions, flows, ops, transforms as T

    torch.manual_seed(11)
    layers = []
    for _ in range(3):
        layers += [T.MaskedSumOfSigmoidsTransform(8, 64), T.ReversePermutation(8)]
    flow = flows.Flow(T.CompositeTransform(layers), distributions.StandardNormal([8])).eval()
    # one layer's bound on the log-determinant, from that layer's oracle on standard-normal rows
    layer = copy.deepcopy(layers[0])
    _, _, _, tol_l = _references(("flow", "layer"), layer, torch.randn(256, 8, generator=torch.Generator().manual_seed(5)))
    flow = flow.to(device)
    with torch.no_grad():
        with ops.KernelTimer(ENTRIES[0]) as timer:
            samples = flow.sample(1000)
        assert len(timer.pairs) == 3 and samples.shape == (1000, 8)
        with ops.KernelTimer(ENTRIES[0]) as timer:
            samples, log_prob = flow.sample_and_log_prob(1000)
        assert len(timer.pairs) == 3
        again = flow.log_prob(samples)
    assert bool(torch.isfinite(samples).all())
    assert maxdiff(log_prob, again) <= 3 * tol_l
