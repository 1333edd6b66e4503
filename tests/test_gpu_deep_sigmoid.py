"""DeepSigmoid / MaskedDeepSigmoidTransform on the GPU: the HIP forward, inverse and backward kernels against the reference's
fixtures and the float64 restatement (tests/_deep_sigmoid_util.py).

Forward margins are the project's golden margin, 4 x the float32 noise floor max|reference float32 - reference float64| that
each fixture records (ordinary rows and the rows pushed to +-50 separately).  Gradient tolerances are those of
tests/test_gpu_backward.py: 1e-4 of the gradient's scale + 8 x what float32 autograd on the restatement loses against
float64."""
import copy
import io
import pickle

import pytest
import torch

import _deep_sigmoid_util as U
import flowconductor_amd.transforms as T
from flowconductor_amd import distributions, flows, ops, options

pytestmark = pytest.mark.gpu

# fc_tile.h, per-sample rows of the [6 x 24] fixture: rowlen = 144, so plan_tile starts from 256 / 6 -> 40 samples per
# tile (25 KiB: over the 24 KiB growth target, under the 40 KiB soft limit), a full 256-thread block, 1440 float4 of
# parameters (<= 8 x 256) and 60 of inputs per tile; launch_tile takes the persistent prefetching variant from 64 full tiles:
# 64 x 40 rows + a leftover tile of 17.
PREFETCH_ROWS = 64 * 40 + 17


def _context(z, device, rows=None):
    return U.tensor(z, "context")[:rows].to(device) if "context" in z.files else None


def _forward(name, module, z, device, rows=None, x=None, dsparams=None):
    x = (U.tensor(z, "x")[:rows] if x is None else x).to(device)
    with torch.no_grad(), ops.KernelTimer("fc_deep_sigmoid") as timer:
        if name == U.PER_SAMPLE:
            dsparams = (U.tensor(z, "dsparams")[:rows] if dsparams is None else dsparams).to(device)
            y, lad = module.forward_given_params(x, dsparams)
        else:
            y, lad = module(x, _context(z, device, rows))
    assert len(timer.pairs) == 1, "fc_deep_sigmoid did not run"
    return y, lad


def _check_against_fixture(name, z, y, lad, rows):
    far = min(int(z["far_rows"]), rows)
    for got, key, tag in ((y, "y64", "y"), (lad, "lad64", "lad")):
        diff = U.row_maxdiff(got, U.tensor(z, key)[:rows])
        print("%s N=%d %s: body %.3g (floor %.3g) far %.3g (floor %.3g)" % (
            name, rows, tag, float(diff[far:].max()) if rows > far else 0.0, float(z["floor_%s_body" % tag]),
            float(diff[:far].max()) if far else 0.0, float(z["floor_%s_far" % tag])))
        if rows > far:
            assert float(diff[far:].max()) <= 4 * float(z["floor_%s_body" % tag]), (name, rows, key)
        if far:
            assert float(diff[:far].max()) <= 4 * float(z["floor_%s_far" % tag]), (name, rows, key)


@pytest.mark.parametrize("name", U.FIXTURES)
def test_forward_against_the_fixtures(device, name):
    z = U.fixture(name)
    module = U.build(name).to(device)
    for rows in (1, 63, 257):
        y, lad = _forward(name, module, z, device, rows)
        _check_against_fixture(name, z, y, lad, rows)


def test_forward_persistent_variant_with_a_leftover_tile(device):
    name = U.PER_SAMPLE
    z = U.fixture(name)
    module = U.build(name).to(device)
    idx = torch.arange(PREFETCH_ROWS) % 257
    x, dsparams = U.tensor(z, "x")[idx], U.tensor(z, "dsparams")[idx]
    y, lad = _forward(name, module, z, device, x=x, dsparams=dsparams)
    fn, _ = U.model(name, module)
    with torch.no_grad():
        y64, lad64 = fn(x, None, dsparams)
    far = idx < int(z["far_rows"])
    for got, ref, tag in ((y, y64, "y"), (lad, lad64, "lad")):
        diff = U.row_maxdiff(got, ref)
        assert float(diff[~far].max()) <= 4 * float(z["floor_%s_body" % tag]), tag
        assert float(diff[far].max()) <= 4 * float(z["floor_%s_far" % tag]), tag
    # the tiles of the persistent kernel and the leftover tile compute the same rows bit for bit
    assert torch.equal(y[:257], y[257:514]) and torch.equal(lad[:257], lad[257:514])
    assert torch.equal(y[PREFETCH_ROWS - 17:], y[(PREFETCH_ROWS - 17) % 257:][:17])


def test_shared_and_per_sample_modes_agree(device):
    name = "ds_f5_s30_m0"
    z = U.fixture(name)
    module = U.build(name).to(device)
    x = U.tensor(z, "x").to(device)
    with torch.no_grad():
        y, lad = module(x)
        y_ps, lad_ps = module.forward_given_params(x, module.dsparams[None].expand(x.shape[0], -1, -1).contiguous())
        back, lad_inv = module.inverse(y[8:])
        back_ps, lad_inv_ps = module.inverse_given_params(y[8:], module.dsparams[None].expand(249, -1, -1).contiguous())
    assert torch.equal(y, y_ps) and torch.equal(lad, lad_ps)
    assert torch.equal(back, back_ps) and torch.equal(lad_inv, lad_inv_ps)


def test_columns_and_logabsdet_modes(device):
    name = U.PER_SAMPLE
    z = U.fixture(name)
    x = U.tensor(z, "x").to(device)
    raw = U.tensor(z, "dsparams").to(device)
    full_y, _ = ops.deep_sigmoid(x, raw, 8)
    cols = torch.tensor([4, 1, 2], dtype=torch.int32, device=device)
    sub = raw[:, [4, 1, 2]].contiguous()
    y, lad = ops.deep_sigmoid(x, sub, 8, cols=cols)
    assert torch.equal(y[:, [0, 3, 5]], x[:, [0, 3, 5]])             # identity columns pass through
    assert torch.equal(y[:, [4, 1, 2]], full_y[:, [4, 1, 2]])
    with torch.no_grad():
        ref = U.restate(x[:, [4, 1, 2]].cpu(), sub.cpu(), 8, 0.0, 1e-4)[1].sum(-1)
    diff = U.row_maxdiff(lad, ref)
    assert float(diff[8:].max()) <= 4 * float(z["floor_lad_body"]) and float(diff[:8].max()) <= 4 * float(z["floor_lad_far"])
    base = torch.randn(x.shape[0], device=device)
    _, neg = ops.deep_sigmoid(x, sub, 8, cols=cols, lad_mode=ops.LAD_STORE_NEG)
    assert torch.equal(neg, -lad)
    acc = base.clone()
    ops.deep_sigmoid(x, sub, 8, cols=cols, lad_mode=ops.LAD_ACCUMULATE, logabsdet=acc)
    assert torch.equal(acc, base + lad)
    acc = base.clone()
    ops.deep_sigmoid(x, sub, 8, cols=cols, lad_mode=ops.LAD_ACCUMULATE_NEG, logabsdet=acc)
    assert torch.equal(acc, base - lad)


@pytest.mark.parametrize("name", ["ds_f7_s1_m0", "ds_f7_s4_m0", "ds_f5_s30_m0", "ds_f3_s4_m25", "ds_f70_s4_m0", U.PER_SAMPLE])
def test_inverse_against_the_float64_model(device, name):
    z = U.fixture(name)
    module = U.build(name).to(device)
    y = U.tensor(z, "y32_inv")
    dsparams = U.tensor(z, "dsparams")[:y.shape[0]] if name == U.PER_SAMPLE else None
    with torch.no_grad(), ops.KernelTimer("fc_deep_sigmoid") as timer:
        if dsparams is None:
            back, lad_inv = module.inverse(y.to(device))
        else:
            back, lad_inv = module.inverse_given_params(y.to(device), dsparams.to(device))
    assert len(timer.pairs) == 1
    fn, _ = U.model(name, module)
    with torch.no_grad():
        y64, lad64 = fn(back.cpu(), None, dsparams)
    print("%s: |f64(x^) - y| %.3g (floor %.3g), |lad_inv + lad64| %.3g (floor %.3g), |x^ - x| %.3g" % (
        name, U.maxdiff(y64, y), float(z["floor_y_inv"]), U.maxdiff(lad_inv, -lad64), float(z["floor_lad_inv"]),
        U.maxdiff(back, U.tensor(z, "x_inv"))))
    assert U.maxdiff(y64, y) <= 4 * float(z["floor_y_inv"])
    assert U.maxdiff(lad_inv, -lad64) <= 4 * float(z["floor_lad_inv"])


def test_inverse_outside_the_range_raises(device):
    module = U.build("ds_f7_s4_m0").to(device)
    bound = ops.deep_sigmoid_bound(module.eps)
    inside = torch.zeros(16, 7, device=device)
    for bad in (12.0, -12.0, bound, -bound):
        y = inside.clone()
        y[5, 3] = bad
        with pytest.raises(T.InputOutsideDomain):
            with torch.no_grad():
                module.inverse(y)
    with torch.no_grad():
        back, _ = module.inverse(inside)       # the error word was cleared: the next call is clean
    assert bool(torch.isfinite(back).all())


@pytest.mark.parametrize("name", ["made_d5_h32_s30_ctx0", "made_d33_h16_s4_ctx0"])
def test_made_layer_inverse(device, name):
    z = U.fixture(name)
    module = U.build(name).to(device)
    fn, _ = U.model(name, module)
    x = U.tensor(z, "x").to(device)
    with torch.no_grad():
        y, lad = module(x)
        assert module._device_loop_form() is None
        for mode in ("auto", "force"):
            with options.override(ar_incremental=mode):
                assert module._incremental_ok(y) == (mode == "force")
                with ops.KernelTimer("fc_deep_sigmoid") as timer:
                    back, lad_inv = module.inverse(y)
            assert len(timer.pairs) == x.shape[1]
            y64, lad64 = fn(back.cpu())
            print("%s %s: |f64(x^) - y| %.3g (floor %.3g) |lad| %.3g (floor %.3g)" % (
                name, mode, U.maxdiff(y64, y), float(z["floor_y_body"]), U.maxdiff(lad_inv, -lad64), float(z["floor_lad_body"])))
            assert U.maxdiff(y64, y) <= 4 * float(z["floor_y_body"]), mode
            assert U.maxdiff(lad_inv, -lad64) <= 4 * float(z["floor_lad_body"]), mode


def test_flow_samples_with_their_density(device):
    name = "made_d5_h32_s30_ctx0"
    z = U.fixture(name)
    flow = flows.Flow(U.build(name), distributions.StandardNormal([5])).to(device).eval()
    torch.manual_seed(3)
    with torch.no_grad():
        samples, log_prob = flow.sample_and_log_prob(64)
        again = flow.log_prob(samples)
    assert samples.shape == (64, 5) and bool(torch.isfinite(samples).all())
    print("sample_and_log_prob vs log_prob: %.3g" % U.maxdiff(log_prob, again))
    assert U.maxdiff(log_prob, again) <= 4 * float(z["floor_y_body"]) * 5


def _tolerance(ref, f32):
    return 1e-4 * float(ref.abs().max()) + 8 * U.maxdiff(f32, ref)


def _restatement_grads(name, module, x, gy, gl, dtype, context=None, dsparams=None):
    fn, twin = U.model(name, module, dtype)
    # (fresh leaves: ``.to`` of the same dtype returns the caller's tensor itself)
    xr = x.detach().clone().to(dtype).requires_grad_(True)
    pr = None if dsparams is None else dsparams.detach().clone().to(dtype).requires_grad_(True)
    y, lad = fn(xr, context, pr)
    ((y * gy.to(dtype)).sum() + (lad * gl.to(dtype)).sum()).backward()
    return xr.grad, (None if pr is None else pr.grad), {k: p.grad for k, p in twin.named_parameters()}


def test_backward_per_sample(device):
    name = U.PER_SAMPLE
    z = U.fixture(name)
    module = U.build(name).to(device)
    x, dsparams, gy, gl = (U.tensor(z, k) for k in ("x", "dsparams", "gy", "gl"))
    f32_gx, f32_gp, _ = _restatement_grads(name, module, x, gy, gl, torch.float32, dsparams=dsparams)
    xd, pd = x.to(device).requires_grad_(True), dsparams.to(device).requires_grad_(True)
    with ops.KernelTimer("fc_deep_sigmoid_backward") as timer:
        y, lad = module.forward_given_params(xd, pd)
        ((y * gy.to(device)).sum() + (lad * gl.to(device)).sum()).backward()
    assert len(timer.pairs) == 1
    for got, key, f32 in ((xd.grad, "grad_x64", f32_gx), (pd.grad, "grad_dsparams64", f32_gp)):
        ref = U.tensor(z, key)
        print("%s %s: %.3g (tolerance %.3g)" % (name, key, U.maxdiff(got, ref), _tolerance(ref, f32)))
        assert U.maxdiff(got, ref) <= _tolerance(ref, f32), key


@pytest.mark.parametrize("name", U.DS_FIXTURES)
def test_backward_shared(device, name):
    z = U.fixture(name)
    module = U.build(name).to(device).train()
    x, gy, gl = (U.tensor(z, k) for k in ("x", "gy", "gl"))
    f32_gx, _, f32_gp = _restatement_grads(name, module, x, gy, gl, torch.float32)
    grads = []
    for _ in range(2):
        module.zero_grad(set_to_none=True)
        xd = x.to(device).requires_grad_(True)
        with ops.KernelTimer("fc_deep_sigmoid_backward") as timer:
            y, lad = module(xd)
            assert type(y.grad_fn).__name__ == "_DeepSigmoidFunctionBackward"
            saved = y.grad_fn.saved_tensors if hasattr(y.grad_fn, "saved_tensors") else ()
            assert all(t.numel() < x.shape[0] * module.dsparams.numel() for t in saved)     # no [N, F, 3S] tensor
            ((y * gy.to(device)).sum() + (lad * gl.to(device)).sum()).backward()
        assert len(timer.pairs) == 1
        assert module.dsparams.grad.shape == module.dsparams.shape
        grads.append((xd.grad.clone(), module.dsparams.grad.clone()))
    assert torch.equal(grads[0][0], grads[1][0]) and torch.equal(grads[0][1], grads[1][1])    # no atomics: bit-identical
    for got, ref, f32 in ((grads[0][0], U.tensor(z, "grad_x64"), f32_gx),
                          (grads[0][1], U.tensor(z, "grad64::dsparams"), f32_gp["dsparams"])):
        print("%s: %.3g (tolerance %.3g)" % (name, U.maxdiff(got, ref), _tolerance(ref, f32)))
        assert U.maxdiff(got, ref) <= _tolerance(ref, f32)


def test_backward_made_layer_in_train_mode(device):
    name = "made_d6_h24_s8_ctx3"
    z = U.fixture(name)
    module = U.build(name).to(device).train()
    x, context, gy, gl = (U.tensor(z, k) for k in ("x", "context", "gy", "gl"))
    f32_gx, _, f32_gp = _restatement_grads(name, module, x, gy, gl, torch.float32, context=context)
    xd = x.to(device).requires_grad_(True)
    with ops.KernelTimer("fc_deep_sigmoid_backward") as timer:
        y, lad = module(xd, context.to(device))
        ((y * gy.to(device)).sum() + (lad * gl.to(device)).sum()).backward()
    assert len(timer.pairs) == 1
    assert U.maxdiff(xd.grad, U.tensor(z, "grad_x64")) <= _tolerance(U.tensor(z, "grad_x64"), f32_gx)
    for pname, p in module.named_parameters():
        ref = U.tensor(z, "grad64::" + pname)
        assert p.grad is not None and U.maxdiff(p.grad, ref) <= _tolerance(ref, f32_gp[pname]), pname


@pytest.mark.parametrize("name", ["ds_f7_s4_m0", U.PER_SAMPLE])
def test_backward_through_the_inverse(device, name):
    z = U.fixture(name)
    module = U.build(name).to(device).train()
    y, gx, gl = U.tensor(z, "y32_inv"), U.tensor(z, "gy")[:128], U.tensor(z, "gl")[:128]
    dsparams = U.tensor(z, "dsparams")[:128] if name == U.PER_SAMPLE else None
    yd = y.to(device).requires_grad_(True)
    pd = module.dsparams if dsparams is None else dsparams.to(device).requires_grad_(True)
    back, lad = module.inverse_given_params(yd, pd)
    ((back * gx.to(device)).sum() + (lad * gl.to(device)).sum()).backward()

    def implicit(dtype):
        """x = x0 - (f(x0; p) - y) / f'(x0) at the root x0 the kernel found, logabsdet = -logabsdet_f(x; p)."""
        fn, twin = U.model(name, module, dtype)
        x0 = back.detach().cpu().to(dtype).requires_grad_(True)
        yr = y.detach().clone().to(dtype).requires_grad_(True)
        pr = twin.dsparams if dsparams is None else dsparams.detach().clone().to(dtype).requires_grad_(True)
        f0, _ = fn(x0, None, pr)
        slope, = torch.autograd.grad(f0.sum(), x0, retain_graph=True)
        x = x0.detach() - (f0 - yr) / slope.detach()
        _, lad_r = fn(x, None, pr)
        ((x * gx.to(dtype)).sum() + (-lad_r * gl.to(dtype)).sum()).backward()
        return yr.grad, pr.grad

    ref_gy, ref_gp = implicit(torch.float64)
    f32_gy, f32_gp = implicit(torch.float32)
    for got, ref, f32 in ((yd.grad, ref_gy, f32_gy), (pd.grad, ref_gp, f32_gp)):
        print("%s inverse gradient: %.3g (tolerance %.3g)" % (name, U.maxdiff(got, ref), _tolerance(ref, f32)))
        assert U.maxdiff(got, ref) <= _tolerance(ref, f32)


def test_fallbacks_take_the_composition(device):
    name = "ds_f7_s4_m0"
    z = U.fixture(name)
    module = U.build(name).to(device)
    x = U.tensor(z, "x")[8:104].to(device)
    with torch.no_grad():
        y, lad = module(x)
        with ops.KernelTimer("fc_deep_sigmoid") as timer:
            y3, lad3 = module(x.reshape(8, 12, 7))
            y64, lad64 = copy.deepcopy(module).double()(x.double())
        assert len(timer.pairs) == 0
    assert y3.shape == (8, 12, 7) and lad3.shape == (8, 12) and y64.dtype == torch.float64
    floor_y, floor_lad = float(z["floor_y_body"]), float(z["floor_lad_body"])
    assert U.maxdiff(y3.reshape(96, 7), y) <= 4 * floor_y and U.maxdiff(y64, y) <= 4 * floor_y
    # ([N, A, F] inputs: the reference sums over the last dim only)
    assert U.maxdiff(lad64, lad) <= 4 * floor_lad
    assert U.maxdiff(lad3.sum(-1), lad.reshape(8, 12).sum(-1)) <= 4 * 12 * floor_lad
    # rows beyond the tile kernels' LDS plan: S = 3200 at 4 features is the smallest (tests/test_deep_sigmoid_host.py)
    assert not ops.deep_sigmoid_fits(4, 4, 3200)
    torch.manual_seed(5)
    wide = T.DeepSigmoid(4, n_sigmoids=3200)
    with torch.no_grad():
        wide.dsparams.add_(torch.randn(wide.dsparams.shape))
    xw = 3 * torch.randn(16, 4)
    fn, _ = U.model("ds_wide", wide)
    with torch.no_grad():
        ref_y, ref_lad = fn(xw)
        cpu_y, cpu_lad = wide(xw)
        with ops.KernelTimer("fc_deep_sigmoid") as timer:
            got_y, got_lad = wide.to(device)(xw.to(device))
        assert len(timer.pairs) == 0
    # the same float32 ops on the device: within 4 x what they lose on the CPU
    assert U.maxdiff(got_y, ref_y) <= 4 * U.maxdiff(cpu_y, ref_y)
    assert U.maxdiff(got_lad, ref_lad) <= 4 * U.maxdiff(cpu_lad, ref_lad)


@pytest.mark.parametrize("name", ["ds_f7_s4_m0", "made_d6_h24_s8_ctx3"])
def test_serialisation_after_a_gpu_call(device, name):
    z = U.fixture(name)
    module = U.build(name).to(device)
    x, context = U.tensor(z, "x").to(device), _context(z, device)
    with torch.no_grad():
        y, lad = module(x, context)
        buffer = io.BytesIO()
        torch.save(module, buffer)
        buffer.seek(0)
        for twin in (copy.deepcopy(module), pickle.loads(pickle.dumps(module)), torch.load(buffer, weights_only=False)):
            y2, lad2 = twin(x, context)
            assert torch.equal(y2, y) and torch.equal(lad2, lad)
            back, _ = twin.inverse(y, context)
            assert U.maxdiff(back, x) <= 1e-3
