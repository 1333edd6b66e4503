"""DeepSigmoid / MaskedDeepSigmoidTransform off the GPU: the float64 restatement against the reference's fixtures, reference
checkpoints, API names and defaults, the torch composition (forward and numerical inverse) and the C ABI of the new entries."""
import inspect
import os
import re

import pytest
import torch
import torch.nn.functional as F

import _deep_sigmoid_util as U
import flowconductor_amd.transforms as T
from flowconductor_amd import _hip, ops
from flowconductor_amd.transforms.adaptive_sigmoids import DeepSigmoid, DeepSigmoidModule
from flowconductor_amd.transforms.autoregressive import MaskedDeepSigmoidTransform

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fixtures_are_all_there():
    assert len(U.DS_FIXTURES) == 5 and len(U.MADE_FIXTURES) == 3 and U.PER_SAMPLE in U.FIXTURES


def _call(name, fn, z, x_key="x"):
    x = U.tensor(z, x_key)
    context = U.tensor(z, "context") if "context" in z.files else None
    dsparams = U.tensor(z, "dsparams")[:x.shape[0]] if name == U.PER_SAMPLE else None
    return fn(x, context, dsparams)


@pytest.mark.parametrize("name", U.FIXTURES)
def test_float64_restatement_matches_the_reference(name):
    z = U.fixture(name)
    fn, _ = U.model(name, U.build(name))
    keys = [("x", "y64", "lad64")] + ([("x_inv", "y64_inv", "lad64_inv")] if "x_inv" in z.files else [])
    for x_key, y_key, lad_key in keys:
        with torch.no_grad():
            y, lad = _call(name, fn, z, x_key)
        for got, ref in ((y, U.tensor(z, y_key)), (lad, U.tensor(z, lad_key))):
            assert bool(((got - ref).abs() <= 1e-12 * ref.abs().clamp(min=1.0)).all()), (name, y_key, U.maxdiff(got, ref))


@pytest.mark.parametrize("name", U.FIXTURES)
def test_reference_state_dicts_load_strictly(name):
    z = U.fixture(name)
    module = U.build(name, load=False)
    assert set(module.state_dict()) == set(U.state(z))
    module.load_state_dict(U.state(z), strict=True)
    for k, v in module.state_dict().items():
        assert torch.equal(v, U.state(z)[k]), k


def test_constructor_defaults_and_attribute_names():
    p = inspect.signature(DeepSigmoidModule.__init__).parameters
    assert list(p)[1:] == ["n_sigmoids", "mollify", "eps", "num_inverse_iterations", "lim"]
    assert [p[k].default for k in list(p)[1:]] == [4, 0., 1e-4, 100, 10]
    p = inspect.signature(MaskedDeepSigmoidTransform.__init__).parameters
    assert list(p)[1:] == ["features", "hidden_features", "n_sigmoids", "context_features", "num_blocks",
                           "use_residual_blocks", "random_mask", "activation", "dropout_probability", "use_batch_norm"]
    assert (p["n_sigmoids"].default, p["context_features"].default, p["num_blocks"].default, p["use_residual_blocks"].default,
            p["random_mask"].default, p["activation"].default, p["dropout_probability"].default,
            p["use_batch_norm"].default) == (30, None, 2, True, False, F.relu, 0.0, False)
    assert T.DeepSigmoid is DeepSigmoid and T.MaskedDeepSigmoidTransform is MaskedDeepSigmoidTransform
    torch.manual_seed(0)
    ds = DeepSigmoid(3)
    assert (ds.features, ds.n_sigmoids, ds.eps, ds._mollify, ds.num_inverse_iterations, ds.lim) == (3, 4, 1e-4, 0., 100, 10)
    assert ds.dsparams.shape == (3, 12) and ds.dsparams.requires_grad
    # the reference's initialisation: -2, 0, 1 plus small noise
    assert U.maxdiff(ds.dsparams[:, :4], torch.full((3, 4), -2.0)) < 1e-4
    assert U.maxdiff(ds.dsparams[:, 4:8], torch.zeros(3, 4)) < 1e-4
    assert U.maxdiff(ds.dsparams[:, 8:], torch.ones(3, 4)) < 1e-2
    raw = torch.arange(24.).reshape(2, 12)
    assert torch.equal(ds.raw_scales(raw), raw[:, :4]) and torch.equal(ds.raw_shifts(raw), raw[:, 4:8])
    assert torch.equal(ds.raw_weights(raw), raw[:, 8:])
    a, b = DeepSigmoid(3, mollify=0.25).mollify(torch.tensor(2.0), torch.tensor(4.0))
    assert float(a) == 1.75 and float(b) == 3.0
    layer = MaskedDeepSigmoidTransform(4, 8)
    assert (layer.features, layer.n_sigmoids) == (4, 30)
    assert layer.autoregressive_net.final_layer.out_features == 4 * 90
    module = layer.deep_sigmoid_module
    assert isinstance(module, MaskedDeepSigmoidTransform.DeepSigmoidMadeModule) and isinstance(module, DeepSigmoidModule)
    assert (module.eps, module.n_sigmoids, module.num_inverse_iterations, module.lim) == (3e-5, 30, 50, 10)
    assert layer._device_loop_form() is None
    with pytest.raises(NotImplementedError, match="Do not directly use this class."):
        module.forward(torch.zeros(2, 4))


@pytest.mark.parametrize("name", U.FIXTURES)
def test_cpu_composition_reproduces_the_reference(name):
    z = U.fixture(name)
    module = U.build(name)
    far = int(z["far_rows"])
    with torch.no_grad():
        if name == U.PER_SAMPLE:
            y, lad = module.forward_given_params(U.tensor(z, "x"), U.tensor(z, "dsparams"))
        else:
            y, lad = module(U.tensor(z, "x"), U.tensor(z, "context") if "context" in z.files else None)
    for got, key, tag in ((y, "y32", "y"), (lad, "lad32", "lad")):
        diff = U.row_maxdiff(got, U.tensor(z, key))
        assert float(diff[far:].max()) <= 4 * float(z["floor_%s_body" % tag]), (name, key)
        if far:
            assert float(diff[:far].max()) <= 4 * float(z["floor_%s_far" % tag]), (name, key)


def test_composition_handles_other_ranks_and_dtypes():
    name = "ds_f7_s4_m0"
    z = U.fixture(name)
    module = U.build(name)
    x = U.tensor(z, "x")[8:104]
    with torch.no_grad():
        y2, lad2 = module(x)
        y3, lad3 = module(x.reshape(8, 12, 7))
        y64, lad64 = module.double()(x.double())
    assert y3.shape == (8, 12, 7) and lad3.shape == (8, 12)
    assert torch.equal(y3.reshape(96, 7), y2) and torch.equal(lad3.reshape(96), lad2)
    assert y64.dtype == torch.float64 and U.maxdiff(y64, U.tensor(z, "y64")[8:104]) <= 1e-12 * 10


def test_mismatched_parameter_batches_raise():
    module = U.build(U.PER_SAMPLE)
    z = U.fixture(U.PER_SAMPLE)
    x, dsparams = U.tensor(z, "x")[:16], U.tensor(z, "dsparams")
    with pytest.raises(ValueError, match="batch"):
        module.forward_given_params(x, dsparams[:15])
    with pytest.raises(ValueError, match="batch"):
        module.inverse_given_params(x, dsparams[:17])
    with pytest.raises(ValueError):
        module.forward_given_params(x, dsparams[:16, :5])


@pytest.mark.parametrize("name", ["ds_f7_s1_m0", "ds_f3_s4_m25", U.PER_SAMPLE])
def test_cpu_numerical_inverse(name):
    """The composition's inverse (bisection + Newton in torch ops) in float64: it returns the recorded inputs."""
    z = U.fixture(name)
    module = U.build(name).double()
    x, y = U.tensor(z, "x_inv").double(), U.tensor(z, "y64_inv")
    dsparams = U.tensor(z, "dsparams")[:x.shape[0]].double() if name == U.PER_SAMPLE else module.dsparams
    with torch.no_grad():
        back, lad = module.inverse_given_params(y, dsparams)
    assert U.maxdiff(back, x) <= 1e-9
    assert U.maxdiff(lad, -U.tensor(z, "lad64_inv")) <= 1e-9
    bound = ops.deep_sigmoid_bound(module.eps)
    for bad in (12.0, -12.0, bound):
        with pytest.raises(T.InputOutsideDomain):
            module.inverse_given_params(torch.full_like(y, bad), dsparams)


def test_made_layer_inverts_on_the_cpu():
    name = "made_d5_h32_s30_ctx0"
    module = U.build(name).double()
    x = U.tensor(U.fixture(name), "x")[:32].double()
    with torch.no_grad():
        y, lad = module(x)
        back, lad_inv = module.inverse(y)
    assert U.maxdiff(back, x) <= 1e-8 and U.maxdiff(lad_inv, -lad) <= 1e-8


def test_tile_plan_limit_mirrors_the_kernel_header():
    """``ops.deep_sigmoid_fits`` restates ``plan_tile`` of csrc/fc_tile.h at one sample per tile; the smallest S that no
    longer fits at 4 features is what the GPU fallback test uses."""
    text = open(os.path.join(ROOT, "flowconductor_amd", "csrc", "fc_tile.h")).read()
    assert re.search(r"kLdsHard\s*=\s*150\s*\*\s*1024", text)
    assert ops.deep_sigmoid_fits(4, 4, 3199) and not ops.deep_sigmoid_fits(4, 4, 3200)
    assert ops.deep_sigmoid_fits(8, 8, 30) and ops.deep_sigmoid_fits(70, 70, 4)


@pytest.mark.parametrize("name", ["fc_deep_sigmoid", "fc_deep_sigmoid_backward", "fc_deep_sigmoid_backward_rows"])
def test_entries_are_declared_bound_and_exported(name):
    import ctypes

    assert name in _hip.SIGNATURES
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "flowcon_hip.h")).read(), flags=re.S)
    decl = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, header)
    assert decl is not None
    assert len(decl.group(1).split(",")) == len(_hip.SIGNATURES[name])
    assert hasattr(ctypes.CDLL(_hip.LIB_PATH), name)


def test_shared_gradient_workspace_rows():
    lib = _hip.load()
    assert lib.fc_deep_sigmoid_backward_rows(257, 7, 4) == 2          # ceil(ceil(257 / 64) / 4) workgroups
    assert lib.fc_deep_sigmoid_backward_rows(1 << 18, 8, 30) == 512   # the fixed cap
    assert lib.fc_deep_sigmoid_backward_rows(64, 4, 3200) == 0        # five rows do not fit 64 KiB of LDS
    assert abs(ops.deep_sigmoid_bound(1e-4) - 9.90344) < 1e-4


def test_cpu_inverse_carries_implicit_function_gradients():
    """Gradients through the composition's inverse in float64: dx/dy = 1 / f'(x) with the slope itself, not the log-det's
    exp (which carries the reference's -2 eps per element: a relative 2e-4 that this test would see)."""
    name = "ds_f7_s4_m0"
    z = U.fixture(name)
    module = U.build(name).double()
    y = U.tensor(z, "y64_inv").clone().requires_grad_(True)
    back, lad = module.inverse(y)
    gy, = torch.autograd.grad(back.sum(), y, retain_graph=True)
    x0 = back.detach().clone().requires_grad_(True)
    fn, twin = U.model(name, module)
    slope, = torch.autograd.grad(fn(x0)[0].sum(), x0)
    assert U.maxdiff(gy * slope, torch.ones_like(gy)) <= 1e-9
    lad.sum().backward()
    assert module.dsparams.grad is not None and bool(torch.isfinite(module.dsparams.grad).all())
