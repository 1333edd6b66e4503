"""MADEMoG / MixtureOfGaussiansMADE off the GPU: API, reference checkpoints, the torch composition of the density against
the reference's fixtures, the C ABI of the new entries and the host-loop sampler."""
import ctypes
import inspect
import os
import re

import pytest
import torch
import torch.nn.functional as F

import _mog_util as M
from flowconductor_amd import _hip, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["fc_mog_log_prob", "fc_mog_log_prob_backward", "fc_made_mog_sample", "fc_made_mog_sample_context"]


def test_imports_and_constructor_defaults():
    from flowconductor_amd.distributions import MADEMoG
    from flowconductor_amd.nn.nde import MixtureOfGaussiansMADE
    from flowconductor_amd.transforms.made import MADE

    made = inspect.signature(MixtureOfGaussiansMADE.__init__).parameters
    assert list(made)[1:] == ["features", "hidden_features", "context_features", "num_blocks", "num_mixture_components",
                              "use_residual_blocks", "random_mask", "activation", "dropout_probability", "use_batch_norm",
                              "epsilon", "custom_initialization"]
    assert (made["num_mixture_components"].default, made["epsilon"].default, made["custom_initialization"].default,
            made["num_blocks"].default, made["context_features"].default) == (5, 1e-2, True, 2, None)
    dist = inspect.signature(MADEMoG.__init__).parameters
    assert list(dist)[1:] == ["features", "hidden_features", "context_features", "num_blocks", "num_mixture_components",
                              "use_residual_blocks", "random_mask", "activation", "dropout_probability", "use_batch_norm",
                              "custom_initialization"]
    assert (dist["num_blocks"].default, dist["num_mixture_components"].default, dist["custom_initialization"].default,
            dist["context_features"].default) == (2, 1, False, inspect.Parameter.empty)
    assert issubclass(MixtureOfGaussiansMADE, MADE)
    with pytest.raises(ValueError, match="Residual blocks can't be used with random masks."):
        MixtureOfGaussiansMADE(3, 8, random_mask=True)
    net = MixtureOfGaussiansMADE(3, 8, num_mixture_components=4)
    assert net.final_layer.out_features == 3 * 3 * 4 and net.epsilon == 1e-2
    assert isinstance(MADEMoG(3, 8, None)._made, MixtureOfGaussiansMADE)


def test_custom_initialisation_is_strided():
    """nn/nde/made.py:390-419: logit rows (::3) at the epsilon scale, ustd rows (2::3) around softplus^-1(1 - epsilon)."""
    from flowconductor_amd.nn.nde import MixtureOfGaussiansMADE

    torch.manual_seed(0)
    net = MixtureOfGaussiansMADE(6, 32, num_mixture_components=5)
    w, b = net.final_layer.weight.detach(), net.final_layer.bias.detach()
    assert float(w[::3].abs().max()) < 0.06 and float(b[::3].abs().max()) < 0.06 and float(w[2::3].abs().max()) < 0.06
    centre = float(torch.log(torch.exp(torch.tensor(1 - 1e-2)) - 1))
    assert float((b[2::3] - centre).abs().max()) < 0.06
    assert float(w[1::3].abs().max()) > 0.1            # the means keep nn.Linear's initialisation


@pytest.mark.parametrize("name", M.FIXTURES)
def test_reference_checkpoint_loads_and_cpu_density_matches(name):
    """strict load of the reference's state_dict; the torch composition on the CPU within 4 x the fixture's own float32
    noise floor of the float64 value, on the ordinary rows and on the rows at +-50 (finite)."""
    g, dims = M.fixture(name)
    dist = M.build(*dims, state=g)
    assert set(dist.state_dict()) == {k[4:] for k in g.files if k.startswith("sd::")}
    x = torch.from_numpy(g["x"])
    context = torch.from_numpy(g["context"]) if dims[3] else None
    with torch.no_grad():
        lp = dist.log_prob(x, context)
    assert lp.shape == (x.shape[0],) and torch.isfinite(lp).all()
    err = (lp.double() - torch.from_numpy(g["log_prob64"])).abs()
    print(name, "body %.3g (floor %.3g) far %.3g (floor %.3g)" % (err[M.FAR_ROWS:].max(), g["floor_body"],
                                                                   err[:M.FAR_ROWS].max(), g["floor_far"]))
    assert float(err[M.FAR_ROWS:].max()) <= 4 * float(g["floor_body"])
    assert float(err[:M.FAR_ROWS].max()) <= 4 * float(g["floor_far"])


def test_fixture_cases_are_the_issue_s():
    assert sorted(M.fixture(n)[1] for n in M.FIXTURES) == sorted(
        [(2, 4, 1, None, 2), (5, 32, 5, 3, 2), (8, 50, 10, 16, 2), (33, 24, 10, 5, 2), (64, 64, 16, 8, 1)])
    for name in M.FIXTURES:
        assert os.path.getsize(os.path.join(M.GOLDEN, "mog_%s.npz" % name)) <= 1 << 20


@pytest.mark.parametrize("name", ENTRIES)
def test_entries_are_declared_bound_and_exported(name):
    assert name in _hip.SIGNATURES
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "flowcon_hip.h")).read(), flags=re.S)
    decl = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, header)
    assert decl is not None, "%s is not declared in include/flowcon_hip.h" % name
    assert len(decl.group(1).split(",")) == len(_hip.SIGNATURES[name])
    assert hasattr(ctypes.CDLL(_hip.LIB_PATH), name), "libflowcon_hip.so does not export %s" % name
    assert _hip.ABI_VERSION == 3


@pytest.mark.parametrize("dims,n,seed", [((2, 4, 1, None, 2), 200, 1), ((5, 32, 5, 3, 2), 200, 2), ((33, 24, 10, 5, 2), 200, 3),
                                         ((64, 64, 16, 8, 1), 96, 4)])
def test_host_loop_sampler_matches_float64_restatement(dims, n, seed):
    """``_sample_from_noise`` on the CPU (the host loop) against the selection rule restated in float64 on the same noise.
    Rows with a near-tie between two components are left out (at most 5 %).  Bound: every pass computes its column from
    three masked products of <= 64 terms and a handful of transcendentals in float32 -- allow 64 eps of the draws' scale
    per pass -- and a column's error feeds every later pass, so the allowance grows linearly with D: 64 D eps."""
    dist = M.build(*dims)
    normal, uniform, context = M.noise(n, dims[0], dims[3], seed)
    x64, keep, logp64 = M.sample64(dist, normal, uniform, context)
    assert float(keep.float().mean()) >= 0.95, "the float64 restatement itself leaves out too many rows"
    x = dist._sample_from_noise(normal, uniform, context)
    assert x.shape == (n, dims[0]) and x.dtype == torch.float32
    scale = max(1.0, float(x64.abs().max()))
    err = float((x.double() - x64)[keep].abs().max())
    print(dims, "kept %d / %d, err %.3g" % (int(keep.sum()), n, err))
    assert err <= 64 * dims[0] * 2.0 ** -23 * scale
    # the log-density the sampler returns is the density of its draws
    x_again, logp = dist._made._sample_from_noise(normal, uniform, context, with_log_prob=True)
    assert torch.equal(x_again, x)
    with torch.no_grad():
        after = dist.log_prob(x, context)
    assert float((logp - after).abs().max()) <= 1e-5 * max(1.0, float(after.abs().max()))


def test_sample_shapes_and_missing_context():
    dist = M.build(5, 32, 5, 3, 2)
    context = torch.randn(3, 3)
    assert dist.sample(7, context).shape == (3, 7, 5)
    draws, logp = dist.sample_and_log_prob(7, context)
    assert draws.shape == (3, 7, 5) and logp.shape == (3, 7)
    with torch.no_grad():
        again = dist.log_prob(draws.reshape(21, 5), context.repeat_interleave(7, dim=0))
    assert float((again.reshape(3, 7) - logp).abs().max()) <= 1e-5 * max(1.0, float(again.abs().max()))
    free = M.build(6, 16, 3, None, 1)
    assert free.sample(7).shape == (7, 6)                    # the reference fails here (context.shape of None)
    draws, logp = free.sample_and_log_prob(9)
    assert draws.shape == (9, 6) and logp.shape == (9,)
    assert not draws.requires_grad


def test_sampler_law_of_column_zero():
    """(2, 4, 1, None, 2): column 0 sees no hidden unit, so it is N(mean, std^2) with the component's mean and
    std = softplus(ustd) + epsilon read from the final layer's bias.  Sample mean and variance of 20 000 draws within 5
    standard errors (std / sqrt(n); std^2 sqrt(2 / (n - 1)))."""
    dist = M.build(2, 4, 1, None, 2)
    bias = dist._made.final_layer.bias.detach().double()
    mean, std = float(bias[1]), float(F.softplus(bias[2]) + dist._made.epsilon)
    torch.manual_seed(11)
    n = 20000
    column = dist.sample(n)[:, 0].double()
    assert abs(float(column.mean()) - mean) <= 5 * std / n ** 0.5
    assert abs(float(column.var()) - std ** 2) <= 5 * std ** 2 * (2 / (n - 1)) ** 0.5


def test_sampler_cache_does_not_travel():
    from _util import copies, warm_modules

    made = M.build(6, 32, 4, None, 2)._made
    ops.static_memo(made, "mog_sample_ok", (6, None), lambda: True)
    pack, _ = made.inverse_packs(12, False)
    for other in copies(made):
        assert warm_modules(other) == [] and ops.cached(other, "mog_sample_ok") is None
    assert ops.cached(made, "mog_sample_ok") is True and ops.cached(made, "made_inverse_pack") is pack
