"""The device loop of the sum-of-sigmoids and sibling-spline layers (fc_made_inverse_sos / fc_made_inverse_spline) off the
GPU: ABI, the forms the four layers hand over, the LDS budget and the final-layer tiling beyond three parameter tiles."""
import ctypes
import os
import re

import pytest
import torch

from flowconductor_amd import _hip, ops
from flowconductor_amd import transforms as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", ["fc_made_inverse_sos", "fc_made_inverse_spline"])
def test_entries_are_declared_bound_and_exported(name):
    assert name in _hip.SIGNATURES
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "flowcon_hip.h")).read(), flags=re.S)
    decl = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, header)
    assert decl is not None, "%s is not declared in include/flowcon_hip.h" % name
    assert len(decl.group(1).split(",")) == len(_hip.SIGNATURES[name])
    assert hasattr(ctypes.CDLL(_hip.LIB_PATH), name), "libflowcon_hip.so does not export %s" % name
    assert _hip.ABI_VERSION == 3


def test_kinds_are_distinct():
    kinds = [ops.MADE_AFFINE, ops.MADE_RQ, ops.MADE_SOS, ops.MADE_SPLINE]
    assert len(set(kinds)) == 4
    assert ops.made_inverse_param_limit(ops.MADE_SOS) == 96
    assert all(ops.made_inverse_param_limit(k) == 48 for k in (ops.MADE_AFFINE, ops.MADE_RQ, ops.MADE_SPLINE))


def test_forms_of_the_four_layers():
    kind, per_dim, kw = T.MaskedSumOfSigmoidsTransform(8, 64).eval()._device_loop_form()
    assert (kind, per_dim) == (ops.MADE_SOS, 91)
    # the constants MaskedSumOfSigmoidsTransform._elementwise_inverse reaches the stand-alone kernel with
    assert kw == dict(n_sigmoids=30, offset=0.5, iterations=50, lim=120.0, log_scale_postact=0.0)
    kind, per_dim, kw = T.MaskedSumOfSigmoidsTransform(6, 64, n_sigmoids=6)._device_loop_form()
    assert (kind, per_dim, kw["n_sigmoids"]) == (ops.MADE_SOS, 19, 6)

    kind, per_dim, kw = T.MaskedPiecewiseLinearAutoregressiveTransform(8, 6, 64)._device_loop_form()
    assert (kind, per_dim) == (ops.MADE_SPLINE, 8) and kw == dict(kind=ops.SPLINE_LINEAR, num_bins=8)

    kind, per_dim, kw = T.MaskedPiecewiseQuadraticAutoregressiveTransform(6, 6, 64, tails="linear",
                                                                          tail_bound=3.0)._device_loop_form()
    assert (kind, per_dim) == (ops.MADE_SPLINE, 11)
    assert kw["kind"] == ops.SPLINE_QUADRATIC and kw["tails"] == "linear" and kw["tail_bound"] == 3.0
    assert kw["width_divisor"] == 1.0           # (a MADE does not expose hidden_features: autoregressive.py:430-432)
    kind, per_dim, kw = T.MaskedPiecewiseQuadraticAutoregressiveTransform(10, 5, 24)._device_loop_form()
    assert (kind, per_dim) == (ops.MADE_SPLINE, 21) and kw["tails"] is None

    kind, per_dim, kw = T.MaskedPiecewiseCubicAutoregressiveTransform(10, 9, 16)._device_loop_form()
    assert (kind, per_dim) == (ops.MADE_SPLINE, 22)
    assert kw == dict(kind=ops.SPLINE_CUBIC, num_bins=10, width_divisor=1.0, height_divisor=1.0)


def test_other_layers_keep_the_host_loop():
    assert T.MaskedDeepSigmoidTransform(6, 32, n_sigmoids=5)._device_loop_form() is None
    assert T.MaskedShiftAutoregressiveTransform(6, 32)._device_loop_form() is None
    assert T.MaskedUMNNAutoregressiveTransform(6, 32)._device_loop_form() is None


def test_lds_budget():
    assert ops.made_inverse_form_fits(64, 2, 91) and ops.made_inverse_form_fits(32, 3, 91)
    assert ops.made_inverse_form_fits(64, 3, 80)                 # five parameter tiles
    assert not ops.made_inverse_form_fits(64, 3, 91)             # three blocks, two k-steps, six parameter tiles: 167 744 B
    assert not ops.made_inverse_form_fits(33, 3, 91)
    assert not ops.made_inverse_form_fits(8, 4, 19)
    assert not ops.made_inverse_form_fits(8, 2, 97)
    assert not ops.made_inverse_form_fits(65, 2, 19)


def test_row_limit_of_the_default_route():
    """Only the sum of sigmoids hands very large batches back to the host loop: rows x sigmoids <= 30 x 2^16."""
    assert ops.made_inverse_row_limit(ops.MADE_SOS, 91) == 1 << 16
    assert ops.made_inverse_row_limit(ops.MADE_SOS, 46) == 1 << 17
    assert ops.made_inverse_row_limit(ops.MADE_SOS, 19) == 5 << 16
    assert all(ops.made_inverse_row_limit(k, 22) is None for k in (ops.MADE_AFFINE, ops.MADE_RQ, ops.MADE_SPLINE))


def test_made_inverse_refuses_what_the_entries_do_not_hold():
    """The form's own argument checks: the pure step of ``made_inverse``, before the library or a device is touched."""
    from flowconductor_amd.ops import conditioner

    t = T.MaskedSumOfSigmoidsTransform(6, 32, n_sigmoids=6)
    kind, per_dim, kw = t._device_loop_form()
    with pytest.raises(ValueError, match=r"20 parameters per dim \(the form has 19\)"):       # 3S + 1 does not match
        conditioner._made_inverse_entry(kind, 6, 2, per_dim + 1, kw)
    with pytest.raises(ValueError, match=r"D = 6, 4 blocks"):                                 # no such instantiation
        conditioner._made_inverse_entry(kind, 6, 4, per_dim, kw)
    with pytest.raises(TypeError, match="unknown arguments"):
        conditioner._made_inverse_entry(kind, 6, 2, per_dim, dict(kw, bins=3))
    c = T.MaskedPiecewiseCubicAutoregressiveTransform(10, 6, 32)
    kind, per_dim, kw = c._device_loop_form()
    with pytest.raises(ValueError, match=r"23 parameters per dim \(the form has 22\)"):
        conditioner._made_inverse_entry(kind, 6, 2, per_dim + 1, kw)


def _unfragment_final(frag, features, pt):
    """[D][ks 2][t PT][piece 2][lane 64][8] f16 fragments -> [D, 16 PT rows, 64] float (hi + lo)."""
    f = frag.reshape(features, 2, pt, 2, 4, 16, 8).float().sum(dim=3)      # [dim][ks][t][g][row][j]: lane = 16 g + row
    return f.permute(0, 2, 4, 1, 3, 5).reshape(features, 16 * pt, 64)      # row 16 t + row, k = 32 ks + 8 g + j


def test_final_layer_tiles_at_six_parameter_tiles():
    """S = 30: 91 parameters per dim in six 16-row tiles; rows 91 .. 95 of every dim are zero, the others are the masked
    final layer's rows of that dim (in the packed unit order) to the 22 bits of two f16 pieces."""
    torch.manual_seed(8)
    t = T.MaskedSumOfSigmoidsTransform(8, 64)
    made = t.autoregressive_net
    hf, hu, hb, ff, fu, fb, need = ops.pack_made_inverse(made, 8, 91)
    assert ff.dtype == torch.float16 and ff.numel() == 8 * 2 * 6 * 2 * 64 * 8
    assert fu.shape == (8,) and fb.shape == (8, 96) and need.shape == (8,)
    rows = _unfragment_final(ff, 8, 6) * fu.reshape(-1, 1, 1)
    assert float(rows[:, 91:].abs().max()) == 0.0 and float(fb[:, 91:].abs().max()) == 0.0
    final = made.final_layer
    w = (final.weight * final.mask).detach().reshape(8, 91, 64)
    order, _ = ops._made_pass_prefix(made, 8, 91, 64)
    # image column c (k-step c // 32) holds the hidden unit the accumulator layout keeps there: rank r at _hb_perm()[r]
    want = torch.zeros(8, 91, 64)
    want[:, :, ops._hb_perm()] = w[:, :, order]
    scale = w.abs().amax(dim=(1, 2)).clamp_min(1e-30).reshape(-1, 1, 1)
    assert float(((rows[:, :91] - want).abs() / scale).max()) <= 2.0 ** -21
    assert torch.equal(fb[:, :91], final.bias.detach().reshape(8, 91))
    assert int(need[0]) == 0 and bool((need[1:] >= need[:-1]).all())
