"""RadialTransform / UnitVector / NaiveLinear off the GPU: API, reference checkpoints, the CPU restatements against the
reference's fixtures, the dense forms of NaiveLinear and the C ABI of the row-norm entries."""
import copy
import ctypes
import inspect
import os
import pickle
import re

import pytest
import torch

import _rownorm_util as U
from flowconductor_amd import _hip, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["fc_radial", "fc_radial_backward", "fc_unit_vector", "fc_unit_vector_backward"]


def test_exports_and_constructor_arguments():
    import flowconductor_amd.transforms as T
    from flowconductor_amd.transforms import no_analytic_inv
    from flowconductor_amd.transforms.linear import Linear
    from flowconductor_amd.utils import torchutils

    radial = inspect.signature(T.RadialTransform.__init__).parameters
    assert list(radial)[1:] == ["features", "z_0"] and radial["features"].default == 2 and radial["z_0"].default is None
    assert no_analytic_inv.RadialTransform is T.RadialTransform
    assert list(inspect.signature(T.UnitVector.__init__).parameters)[1:] == ["features"]
    naive = inspect.signature(T.NaiveLinear.__init__).parameters
    assert list(naive)[1:] == ["features", "orthogonal_initialization", "using_cache"]
    assert (naive["orthogonal_initialization"].default, naive["using_cache"].default) == (True, False)
    assert issubclass(T.NaiveLinear, Linear)
    assert T.RadialTransform._HIP_AUTOGRAD and T.UnitVector._HIP_AUTOGRAD and T.NaiveLinear._HIP_AUTOGRAD
    for name in ("radial", "radial_autograd", "_RadialFunction", "unit_vector", "unit_vector_autograd", "_UnitVectorFunction",
                 "dense_linear_autograd", "_DenseLinearFunction"):
        assert hasattr(ops, name), name
    assert callable(torchutils.batch_JTJ_logabsdet)

    torch.manual_seed(0)
    r = T.RadialTransform(4)
    assert list(r.state_dict()) == U.STATE_KEYS["radial"]
    assert r.beta.shape == (1,) and r.alpha.shape == (1,) and r.z_0.shape == (1, 4)
    assert r.d.dtype == torch.int64 and int(r.d) == 4
    assert -1.25 - 1e-6 <= r.beta.item() <= -0.75 + 1e-6 and abs(r.alpha.item()) <= 0.25 + 1e-6
    u = T.UnitVector(3)
    assert list(u.state_dict()) == U.STATE_KEYS["unit_vector"] and u.dim_Rd == 3
    assert isinstance(u.dim_sphere, torch.nn.Parameter) and u.dim_sphere.dtype == torch.float32 and u.dim_sphere.item() == 4.0
    n = T.NaiveLinear(6)
    assert list(n.state_dict()) == U.STATE_KEYS["naive_linear"]
    with torch.no_grad():
        assert float((n._weight @ n._weight.T - torch.eye(6)).abs().max()) <= 1e-5      # orthogonal initialisation
        assert float(n.bias.abs().max()) == 0.0
    m = T.NaiveLinear(16, orthogonal_initialization=False)
    assert 0 < float(m._weight.abs().max()) <= 0.25


@pytest.mark.parametrize("name", U.FIXTURES)
def test_reference_checkpoint_loads_strictly(name):
    t, kind, d = U.fixture(name)
    module = U.build(name)
    assert list(module.state_dict()) == U.STATE_KEYS[kind]
    for key, value in U.state_dict(name).items():
        assert torch.equal(module.state_dict()[key], value)
    assert os.path.getsize(os.path.join(U.GOLDEN, name + ".npz")) <= 1 << 20
    assert t["x"].shape == (257, d) and t["y32"].dtype == torch.float32 and t["grad_x64"].shape == (257, d)
    if kind == "radial":
        row = int(t["edge_row"])
        assert torch.equal(t["x"][row], t["sd::z_0"][0]) and "xinv32" not in t
    if kind == "unit_vector":
        assert float((1 - t["y64"][:, -1]).min()) >= 0.05
    if name == "naive_linear_d64":
        assert float(t["sd::bias"].abs().max()) > 100      # the bias that must come off first


@pytest.mark.parametrize("name", U.FIXTURES)
def test_float32_restatement_reproduces_the_fixture(name):
    """The util's float32 evaluation against the reference's float32 and float64 values: 1e-5 scale + 4 x floor."""
    t, kind, d = U.fixture(name)
    y, lad = U.restate(name, t["x"], torch.float32)
    for got, ref32, ref64, floor, what in ((y, t["y32"], t["y64"], t["floor_fwd_y"], "y"),
                                           (lad, t["lad32"], t["lad64"], t["floor_fwd_lad"], "lad")):
        bound = U.bound(ref64.abs().max(), floor)
        err32, err64 = float((got.double() - ref32.double()).abs().max()), float((got.double() - ref64).abs().max())
        print(name, what, "err32 %.3g err64 %.3g bound %.3g" % (err32, err64, bound))
        assert err32 <= bound and err64 <= bound, (name, what)
    if kind != "radial":
        x, ladinv = U.restate(name, t["y32"], torch.float32, inverse=True)
        assert float((x.double() - t["xinv64"]).abs().max()) <= U.bound(t["xinv64"].abs().max(), t["floor_inv_x"])
        assert float((ladinv.double() - t["ladinv64"]).abs().max()) <= U.bound(t["ladinv64"].abs().max(), t["floor_inv_lad"])


@pytest.mark.parametrize("name", U.RADIAL)
def test_closed_form_radial_inverse_undoes_the_reference_forward(name):
    """float64: the util's closed-form inverse of the reference's float64 outputs is the fixture's x to 1e-12, with the
    negated logabsdet."""
    t, _, _ = U.fixture(name)
    x, lad = U.restate(name, t["y64"], torch.float64, inverse=True)
    assert float((x - t["x"].double()).abs().max()) <= 1e-12
    assert float((lad + t["lad64"]).abs().max()) <= 1e-12


@pytest.mark.parametrize("d", [1, 3, 20])
def test_batch_jtj_logabsdet_is_the_unit_vector_logabsdet(d):
    from flowconductor_amd.utils import torchutils

    torch.manual_seed(d)
    x = torch.randn(9, d, dtype=torch.float64, requires_grad=True)
    y, lad = U.unit_forward(x)
    assert y.shape == (9, d + 1) and float((y.pow(2).sum(-1) - 1).abs().max()) <= 1e-14
    assert float((torchutils.batch_JTJ_logabsdet(x, y) - lad).abs().max()) <= 1e-12


@pytest.mark.parametrize("name", ENTRIES)
def test_entries_are_declared_bound_and_exported(name):
    assert name in _hip.SIGNATURES
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "flowcon_hip.h")).read(), flags=re.S)
    decl = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, header)
    assert decl is not None, "%s is not declared in include/flowcon_hip.h" % name
    assert len(decl.group(1).split(",")) == len(_hip.SIGNATURES[name])
    assert hasattr(ctypes.CDLL(_hip.LIB_PATH), name), "libflowcon_hip.so does not export %s" % name


@pytest.mark.parametrize("name", U.NAIVE)
def test_naive_linear_dense_forms_on_the_cpu(name):
    """Uncached (``weight`` / ``weight_inverse`` / ``logabsdet`` and the torch composition) and cached (the ``Linear`` cache
    slots) dense forms on CPU tensors against ``x @ W.T + b`` and its inverse: 4 x the fixture's floor."""
    t, _, d = U.fixture(name)
    module = U.build(name, using_cache=True)
    eye = torch.eye(d, dtype=torch.float64)
    with torch.no_grad():
        module._check_forward_cache()
        module._check_inverse_cache()
        cached = (module.cache.weight, module.cache.inverse, module.cache.logabsdet)
        uncached = (module.weight(), module.weight_inverse(), module.logabsdet())
        for w, w_inv, lad in (cached, uncached, (module.weight(),) + tuple(module.weight_inverse_and_logabsdet())):
            assert w.dtype == torch.float32 and w_inv.dtype == torch.float32 and w_inv.device == module._weight.device
            y = t["x"] @ w.T + module.bias
            x_back = (t["y32"] - module.bias) @ w_inv.T
            assert float((y.double() - t["y64"]).abs().max()) <= 4 * float(t["floor_fwd_y"])
            assert float((x_back.double() - t["xinv64"]).abs().max()) <= 4 * float(t["floor_inv_x"])
            # (the float64 value rounded once to float32 is off by up to half a unit in the last place)
            assert float((lad.double() - t["lad64"][0]).abs()) <= 4 * float(t["floor_fwd_lad"]) + 2.0 ** -24 * float(t["lad64"][0].abs())
            assert float((w.double() @ w_inv.double() - eye).abs().max()) <= 1e-5
        y = module._composition(t["x"], False)
        x_back = module._composition(t["y32"], True)
        assert float((y.double() - t["y64"]).abs().max()) <= 4 * float(t["floor_fwd_y"])
        assert float((x_back.double() - t["xinv64"]).abs().max()) <= 4 * float(t["floor_inv_x"])
    # with a graph the dense forms are differentiable: against float64 autograd through torch.linalg.inv
    (module.weight_inverse() * t["gy"][:d, :d]).sum().backward()
    w64 = t["sd::_weight"].double().requires_grad_(True)
    (torch.linalg.inv(w64) * t["gy"][:d, :d].double()).sum().backward()
    scale = float(w64.grad.abs().max())
    assert float((module._weight.grad.double() - w64.grad).abs().max()) <= 1e-4 * scale + 1e-5


def test_train_invalidates_the_linear_cache_and_the_memo_follows_the_parameters():
    module = U.build("naive_linear_d5", using_cache=True)
    with torch.no_grad():
        module._check_inverse_cache()
        assert module.cache.inverse is not None and module.cache.logabsdet is not None
        module.train()
        assert module.cache.weight is None and module.cache.inverse is None and module.cache.logabsdet is None
        module.eval()
        first = module.weight_inverse()
        assert module.weight_inverse() is first                     # memoised: one factorisation
        module._weight.mul_(2.0)                                    # an in-place update bumps the version
        second = module.weight_inverse()
        assert second is not first and float((second * 2 - first).abs().max()) <= 1e-6


def test_copies_of_a_naive_linear_that_has_run_carry_parameters_only():
    module = U.build("naive_linear_d5")
    with torch.no_grad():
        module.weight_inverse_and_logabsdet()
    assert module.__dict__["_fc_cache"]
    for clone in (copy.deepcopy(module), pickle.loads(pickle.dumps(module))):
        assert not clone.__dict__.get("_fc_cache")
        assert list(clone.state_dict()) == U.STATE_KEYS["naive_linear"]
        assert torch.equal(clone._weight, module._weight) and torch.equal(clone.bias, module.bias)


def test_value_errors():
    import flowconductor_amd.transforms as T

    with pytest.raises(ValueError):
        T.UnitVector(ops.MAX_ROW_FEATURES)                 # features + 1 > 512
    T.UnitVector(ops.MAX_ROW_FEATURES - 1)
    with pytest.raises(ValueError):
        T.UnitVector(3).forward(torch.zeros(2, 4))
    with pytest.raises(ValueError):
        T.UnitVector(3).inverse(torch.zeros(2, 3))
    with pytest.raises(ValueError):
        T.RadialTransform(4, z_0=torch.zeros(4))           # no leading batch dimension of 1
    with pytest.raises(ValueError):
        T.RadialTransform(4, z_0=torch.zeros(2, 2))
    with pytest.raises(ValueError):
        T.RadialTransform(1024, z_0=torch.zeros(1, 32, 32))      # more than 512 values per row
    with pytest.raises(ValueError):
        T.RadialTransform(4).forward(torch.zeros(2, 5))
    assert T.RadialTransform(32, z_0=torch.zeros(1, 2, 4, 4)).z_0.shape == (1, 2, 4, 4)
