"""Batch statistics off the GPU: the option, the ``ops`` names, the support rule, the backward formulas of
``fc_batchnorm_train_backward`` restated in float64 against autograd, and the CPU route of ``BatchNorm``."""
import importlib
import subprocess
import sys

import pytest
import torch
from torch.nn import functional as F

from flowconductor_amd import _hip, ops, options, transforms as T

from _util import maxdiff


def test_option_exists_and_defaults_on():
    assert options.get("batch_statistics_kernels") is True
    with options.override(batch_statistics_kernels=False):
        assert options.get("batch_statistics_kernels") is False
        assert options.snapshot()["batch_statistics_kernels"] is False
    assert options.get("batch_statistics_kernels") is True


def test_ops_names_and_constants():
    for name in ("column_sums", "batchnorm_train", "batchnorm_train_autograd", "batch_statistics_supported"):
        assert callable(getattr(ops, name)), name
    assert ops.COLSTATS_MAX_PARTIALS == 512 and ops.COLSTATS_ROWS_PER_ITERATION == 2048
    for name in ("fc_batchnorm_train", "fc_batchnorm_train_backward", "fc_column_sums", "fc_colstats_workspace"):
        assert name in _hip.SIGNATURES


def test_header_constants_match_ops():
    import os
    import re

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "flowcon_hip.h")).read()
    value = lambda name: int(re.search(r"#define %s (\d+)" % name, text).group(1))
    assert value("FC_COLSTATS_MAX_PARTIALS") == ops.COLSTATS_MAX_PARTIALS
    assert value("FC_COLSTATS_ROWS_PER_ITERATION") == ops.COLSTATS_ROWS_PER_ITERATION
    assert value("FC_COLSTATS_MAX_FEATURES") == ops.MAX_ROW_FEATURES


def test_module_imports_without_the_library():
    script = ("import importlib, sys\n"
              "m = importlib.import_module('flowconductor_amd.ops.colstats')\n"
              "assert sys.modules['flowconductor_amd._hip']._lib is None\n"
              "print(sorted(n for n in ('column_sums', 'batchnorm_train') if hasattr(m, n)))\n")
    done = subprocess.run([sys.executable, "-c", script], capture_output=True, text=True,
                          cwd=importlib.import_module("os").path.dirname(importlib.import_module("os").path.dirname(__file__)))
    assert done.returncode == 0, done.stderr
    assert done.stdout.strip() == "['batchnorm_train', 'column_sums']"


def test_workspace_entry():
    lib = _hip.load()
    assert lib.fc_colstats_workspace(7) == ops.COLSTATS_MAX_PARTIALS * 15
    assert lib.fc_colstats_workspace(0) == 0 and lib.fc_colstats_workspace(513) == 0


def test_entries_refuse_bad_shapes_before_touching_memory():
    """n < 2, d > 512 and null pointers are hipErrorInvalidValue (1); nothing is launched, so this runs without a GPU."""
    import ctypes

    lib = _hip.load()
    p = ctypes.c_void_p(4096)        # never dereferenced: every call below fails its argument checks
    none = None
    assert lib.fc_batchnorm_train(p, p, p, p, p, p, p, p, none, none, p, 1, 4, 1e-5, 0.1, none) == 1
    assert lib.fc_batchnorm_train(p, p, p, p, p, p, p, p, none, none, p, 8, 513, 1e-5, 0.1, none) == 1
    assert lib.fc_batchnorm_train(p, p, p, none, p, p, p, p, none, none, p, 8, 4, 1e-5, 0.1, none) == 1
    assert lib.fc_batchnorm_train(p, p, p, p, p, p, p, p, p, none, p, 8, 4, 1e-5, 0.1, none) == 1
    assert lib.fc_column_sums(p, p, none, none, none, p, p, none, p, 1, 4, none) == 1
    assert lib.fc_column_sums(p, p, none, none, none, p, p, none, p, 8, 0, none) == 1
    assert lib.fc_column_sums(p, p, p, none, none, p, p, none, p, 8, 4, none) == 1
    assert lib.fc_column_sums(p, p, none, none, p, p, p, none, p, 8, 4, none) == 1
    assert lib.fc_batchnorm_train_backward(p, p, none, p, p, p, p, p, p, none, p, 1, 4, none) == 1
    assert lib.fc_batchnorm_train_backward(p, p, none, p, p, p, p, p, p, none, p, 8, 513, none) == 1
    assert lib.fc_batchnorm_train_backward(p, none, none, p, p, p, p, p, p, none, p, 8, 4, none) == 1


def test_support_rule():
    ok = ops.batch_statistics_supported
    assert not ok(torch.zeros(8, 4))                                   # CPU
    assert not ok(torch.zeros(8, 4, dtype=torch.float64))
    assert not ok(torch.zeros(1, 4)) and not ok(torch.zeros(8, 513)) and not ok(torch.zeros(8, 4, 2))
    assert not ok(None)
    meta = lambda *shape, **kw: torch.empty(*shape, device="meta", **kw)
    assert not ok(meta(8, 4))                                          # not a HIP device either


def _reference(x, uw, bias, eps):
    weight = F.softplus(uw) + eps
    var, mean = torch.var_mean(x, dim=0)
    y = weight * ((x - mean) / torch.sqrt(var + eps)) + bias
    return y, torch.sum(torch.log(weight) - 0.5 * torch.log(var + eps)) * x.new_ones(x.shape[0])


@pytest.mark.parametrize("n,d", [(2, 1), (3, 3), (17, 5), (64, 8)])
def test_backward_formulas_match_float64_autograd(n, d):
    """gx = w invstd (gy - s1 / N - xh s2 / (N - 1)) - GL invstd xh / (N - 1), g_w = s2 + GL / w, g_b = s1."""
    g = torch.Generator().manual_seed(100 * n + d)
    eps = 1e-5
    x = (torch.randn(n, d, generator=g, dtype=torch.float64) * 1.7 + 0.3).requires_grad_(True)
    uw = torch.randn(d, generator=g, dtype=torch.float64).requires_grad_(True)
    bias = torch.randn(d, generator=g, dtype=torch.float64).requires_grad_(True)
    gy = torch.randn(n, d, generator=g, dtype=torch.float64)
    gl = torch.randn(n, generator=g, dtype=torch.float64)
    y, lad = _reference(x, uw, bias, eps)
    weight = (F.softplus(uw) + eps).detach().requires_grad_(True)
    gx_ref, guw_ref, gb_ref = torch.autograd.grad((y, lad), (x, uw, bias), (gy, gl))
    with torch.no_grad():
        var, mean = torch.var_mean(x, dim=0)
        invstd = 1.0 / torch.sqrt(var + eps)
        xh = (x - mean) * invstd
        s1, s2, GL = gy.sum(0), (gy * xh).sum(0), gl.sum()
        gx = weight * invstd * (gy - s1 / n - xh * s2 / (n - 1)) - GL * invstd * xh / (n - 1)
        g_w, g_b = s2 + GL / weight, s1
    guw = g_w * torch.sigmoid(uw.detach())           # d softplus
    for got, ref in ((gx, gx_ref), (guw, guw_ref), (g_b, gb_ref)):
        assert maxdiff(got, ref) <= 1e-12 * max(1.0, float(ref.abs().max()))


def test_cpu_batchnorm_training_is_the_reference_expression_bit_for_bit():
    torch.manual_seed(5)
    t = T.BatchNorm(5).train()
    with torch.no_grad():
        t.unconstrained_weight.normal_()
        t.bias.normal_()
    x = (torch.randn(33, 5) * 2 + 0.7).requires_grad_(True)
    y, lad = t(x)
    var, mean = torch.var_mean(x, dim=0)
    expect = t.weight * ((x - mean) / torch.sqrt(var + t.eps)) + t.bias
    expect_lad = torch.sum(torch.log(t.weight) - 0.5 * torch.log(var + t.eps)) * x.new_ones(33)
    assert torch.equal(y, expect) and torch.equal(lad, expect_lad)
    assert torch.equal(t.running_mean, torch.zeros(5).lerp_(mean.detach(), 0.1))
    assert torch.equal(t.running_var, torch.zeros(5).lerp_(var.detach(), 0.1))
    (y.square().sum() - lad.sum()).backward()
    gx, = torch.autograd.grad(expect.square().sum() - expect_lad.sum(), x)
    assert torch.equal(x.grad, gx)
    y1, _ = t(torch.randn(1, 5))                           # N = 1: the reference's NaN stays
    assert bool(torch.isnan(y1).all())
