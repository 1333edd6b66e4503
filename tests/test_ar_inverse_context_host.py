"""The conditional device loop (fc_made_inverse_context) off the GPU: ABI, the context part of the pack, cache attributes and
the reference's statement that the context never reaches column 0 of an autoregressive inverse."""
import copy
import ctypes
import os
import re

import pytest
import torch

from _util import copies, warm_modules
from flowconductor_amd import _hip, ops
from flowconductor_amd import transforms as T
from oracle import torch_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (kind, D, hidden, C, blocks, N): the parity cases of tests/test_gpu_ar_inverse_context.py
SHAPES = [("maf", 6, 64, 3, 2, 1000), ("maf", 2, 4, 1, 2, 4096), ("maf", 40, 50, 32, 1, 333), ("maf", 3, 16, 7, 0, 50),
          ("rq_k8_tails", 6, 64, 4, 2, 1000), ("rq_k8_tails", 33, 24, 5, 2, 200), ("rq_k8_tails", 64, 64, 8, 2, 96),
          ("rq_k5_box", 5, 24, 7, 2, 77), ("rq_k10_box", 8, 64, 10, 2, 512), ("rq_k16_tails", 7, 32, 1, 3, 160)]


def build(kind, features, hidden, context_features, blocks):
    """The layer of a parity case, in eval mode: RQ layers with their parameters times 1.5, MAF layers as initialised
    (an affine inverse compounds 1 / scale over the dims: scaled up it reaches 1e6 and no bound means anything)."""
    torch.manual_seed(features + hidden)
    if kind == "maf":
        t = T.MaskedAffineAutoregressiveTransform(features, hidden, context_features=context_features, num_blocks=blocks)
    else:
        k = int(re.search(r"k(\d+)", kind).group(1))
        t = T.MaskedPiecewiseRationalQuadraticAutoregressiveTransform(
            features, hidden, context_features=context_features, num_bins=k, tails="linear" if "tails" in kind else None,
            tail_bound=3.0, num_blocks=blocks)
        with torch.no_grad():
            for p in t.parameters():
                p.mul_(1.5)
    return t.eval()


def inputs(kind, n, features, context_features, context_scale=1.0):
    g = torch.Generator().manual_seed(5)
    x = torch.rand(n, features, generator=g) * 2.2 - 1.1 if "box" in kind else torch.randn(n, features, generator=g) * 1.2
    return x, context_scale * torch.randn(n, context_features, generator=g)


def test_entry_is_declared_bound_and_exported():
    name = "fc_made_inverse_context"
    assert name in _hip.SIGNATURES
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "flowcon_hip.h")).read(), flags=re.S)
    decl = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, header)
    assert decl is not None, "%s is not declared in include/flowcon_hip.h" % name
    assert len(decl.group(1).split(",")) == len(_hip.SIGNATURES[name])
    assert hasattr(ctypes.CDLL(_hip.LIB_PATH), name), "libflowcon_hip.so does not export %s" % name
    assert _hip.ABI_VERSION == 3


def _unfragment(frag, layers):
    """[layers][t 4][piece 2][lane 64][8] f16 fragments -> [layers, 64 image rows, 32] float (hi + lo)."""
    f = frag.reshape(layers, 4, 2, 4, 16, 8).float().sum(dim=2)            # [layer][t][g][row][j]: lane = 16 g + row
    return f.permute(0, 1, 3, 2, 4).reshape(layers, 64, 32)                # row 16 t + row, k = 8 g + j


@pytest.mark.parametrize("features,hidden,context_features,blocks,per_dim",
                         [(6, 64, 3, 2, 2), (40, 50, 32, 1, 2), (33, 24, 5, 2, 23), (7, 32, 1, 3, 47), (3, 16, 7, 0, 2)])
def test_context_pack_maps_back_to_the_context_layers(features, hidden, context_features, blocks, per_dim):
    from flowconductor_amd.transforms.made import MADE

    torch.manual_seed(features)
    made = MADE(features, hidden, context_features=context_features, num_blocks=blocks, output_multiplier=per_dim)
    with torch.no_grad():
        for i, lin in enumerate([made.context_layer] + [b.context_layer for b in made.blocks]):
            lin.weight.mul_(3.0 ** i)             # the layers get different scales
    frag, unscale, bias = ops.pack_made_inverse_context(made, features, per_dim)
    layers = [made.context_layer] + [b.context_layer for b in made.blocks]
    assert frag.dtype == torch.float16 and frag.numel() == len(layers) * 4096
    assert unscale.shape == (len(layers),) and bias.shape == (len(layers), 64)
    order, need = ops._made_pass_prefix(made, features, per_dim, 64)
    assert torch.equal(need.to(torch.int32), ops.pack_made_inverse(made, features, per_dim)[-1].cpu())
    image = _unfragment(frag, len(layers)) * unscale.reshape(-1, 1, 1)
    for l, lin in enumerate(layers):
        w = torch.zeros(64, 32)
        w[:hidden, :context_features] = lin.weight.detach()
        b = torch.zeros(64)
        b[:hidden] = lin.bias.detach()
        # image row r (tile r // 16, row r % 16 of the accumulator) is the hidden unit of rank r
        scale = float(w.abs().max())
        assert float((image[l] - w[order]).abs().max()) <= 2.0 ** -21 * scale      # two f16 pieces: 22 bits under the layer's maximum
        # bias: [g][t][r] holds the unit in accumulator tile t, row 4 g + r: rank 16 t + 4 g + r of the renumbered stack
        by_rank = bias[l].reshape(4, 4, 4).permute(1, 0, 2).reshape(64)
        assert torch.equal(by_rank, b[order])


def test_context_lds_budget():
    assert ops.made_inverse_context_fits(64, 2, 47) and ops.made_inverse_context_fits(64, 3, 2)
    assert ops.made_inverse_context_fits(7, 3, 23)
    assert not ops.made_inverse_context_fits(7, 3, 47)           # three blocks, three parameter tiles
    assert not ops.made_inverse_context_fits(40, 3, 23)          # three blocks, two k-steps, two parameter tiles
    assert not ops.made_inverse_context_fits(8, 4, 2)


def test_device_loop_caches_do_not_travel():
    t = build("maf", 6, 32, 3, 2)
    net = t.autoregressive_net
    pack, context_pack = net.inverse_packs(2, True)
    ops.static_memo(t, "device_loop_ok", (0,), lambda: True)
    ops.static_memo(t, "device_loop_context_ok", (0,), lambda: True)
    deep, pickled, loaded = copies(t)
    for other in (deep, pickled, loaded):
        assert warm_modules(other) == []
        assert all(ops.cached(other, name) is None for name in ("device_loop_ok", "device_loop_context_ok"))
        assert all(ops.cached(other.autoregressive_net, name) is None
                   for name in ("made_inverse_pack", "made_inverse_context_pack"))
    assert all(torch.equal(a, b) for a, b in zip(loaded.state_dict().values(), t.state_dict().values()))
    assert ops.cached(net, "made_inverse_context_pack") is context_pack       # the original keeps its packs
    assert ops.cached(net, "made_inverse_pack") is pack and ops.cached(t, "device_loop_ok") is True


def test_inverse_packs_are_kept_per_output_width_and_follow_the_weights(monkeypatch):
    """MADE.inverse_packs: unchanged weights give the very same tensors, an in-place update re-packs what was made from
    the changed layer; a caller asking for another ``per_dim`` is never handed the pack of the first (a real net has one
    output width, so the packers are stubbed for that part)."""
    net = build("maf", 6, 32, 3, 2).autoregressive_net
    pack, context_pack = net.inverse_packs(2, True)
    again, context_again = net.inverse_packs(2, True)
    assert all(a is b for a, b in zip(pack + context_pack, again + context_again))
    assert net.inverse_packs(2, False) == (pack, None)
    assert all(torch.equal(a, b) for a, b in zip(pack, ops.pack_made_inverse(net, 6, 2)))
    assert all(torch.equal(a, b) for a, b in zip(context_pack, ops.pack_made_inverse_context(net, 6, 2)))
    with torch.no_grad():
        net.blocks[0].linear_layers[0].weight.mul_(2.0)
    fresh, context_same = net.inverse_packs(2, True)
    assert fresh is not pack and context_same is context_pack          # (no context layer changed)
    assert all(torch.equal(a, b) for a, b in zip(fresh, ops.pack_made_inverse(net, 6, 2)))
    assert not all(torch.equal(a, b) for a, b in zip(fresh, pack))
    with torch.no_grad():
        net.context_layer.bias.add_(0.5)
    assert net.inverse_packs(2, True)[1] is not context_pack
    monkeypatch.setattr(ops, "pack_made_inverse", lambda made, features, per_dim: ("pack", features, per_dim))
    monkeypatch.setattr(ops, "pack_made_inverse_context", lambda made, features, per_dim: ("context", features, per_dim))
    for per_dim in (23, 12, 23):
        assert net.inverse_packs(per_dim, True) == (("pack", 6, per_dim), ("context", 6, per_dim))


@pytest.mark.parametrize("kind,features,hidden,context_features,blocks,n", SHAPES)
def test_oracle_column_zero_ignores_the_context(kind, features, hidden, context_features, blocks, n):
    """float64 on the CPU: the reference's conditional inverse (made.py: dim 0's parameters are the final layer's biases)
    gives the same column 0 for unrelated contexts; the fixtures of the GPU parity cases are well conditioned."""
    t = build(kind, features, hidden, context_features, blocks)
    x, c1 = inputs(kind, n, features, context_features)
    c2 = 20 * torch.randn(n, context_features, generator=torch.Generator().manual_seed(6))
    with torch.no_grad():
        y32, _ = O.transform_apply(t, x.clone(), c1, inverse=True)
        t64 = copy.deepcopy(t).double()
        y1, _ = O.transform_apply(t64, x.double(), c1.double(), inverse=True)
        y2, _ = O.transform_apply(t64, x.double(), c2.double(), inverse=True)
    assert torch.equal(y1[:, 0], y2[:, 0])
    assert not torch.equal(y1[:, 1], y2[:, 1])
    assert float(y1.abs().max()) <= 100
    assert float((y32.double() - y1).abs().max()) <= 2e-4 * max(1.0, float(y1.abs().max()))
