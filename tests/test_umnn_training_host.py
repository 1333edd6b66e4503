"""UMNN training off the GPU: the option's default, the transposed image of ``fc_umnn_backward``, and the torch
composition's inverse under autograd -- the root of the search re-attached by the implicit-function theorem, values
unchanged."""
import pytest
import torch

from flowconductor_amd import ops, options
from flowconductor_amd.transforms.UMNN import IntegrandNet

import _umnn_training_util as G
import _umnn_util as U


def test_option_defaults_to_the_composition():
    assert options.get("umnn_training") is False


@pytest.mark.parametrize("hidden,cond", [([16], 1), ([50, 50], 20), ([64, 64, 64], 31), ([24, 40, 64], 7), ([7, 64], 31)])
def test_transposed_image_unpacks_to_the_transposed_weights(hidden, cond):
    torch.manual_seed(len(hidden) * 100 + cond)
    net = IntegrandNet(hidden, cond)
    lins = net.linears()
    fragt = ops.pack_umnn_backward(lins, torch.device("cpu"))
    assert fragt.dtype == torch.float16 and fragt.numel() == (16 * (len(hidden) - 1) + 8) * 512
    perm = ops._hb_perm()

    def unpack(flat, tiles):
        """[ks][tile][piece][lane][8] -> the matrix [16 tiles, 64] the fragments hold (lane l: row l & 15 of its tile,
        k = 32 ks + 8 (l >> 4) + j), pieces added, rows put back from accumulator order."""
        f = flat.view(2, tiles, 2, 64, 8).float()
        val = f[:, :, 0] + f[:, :, 1]                                 # [ks, tile, lane, 8]
        val = val.view(2, tiles, 4, 16, 8).permute(1, 3, 0, 2, 4).reshape(tiles * 16, 64)
        out = torch.empty_like(val)
        out[perm[:tiles * 16]] = val
        return out

    def check(got, w, rows, cols):
        want = torch.zeros(rows, cols)
        want[:w.shape[1], :w.shape[0]] = w.detach().t()
        sc, un = ops._pow2_scale(want.abs().amax().reshape(1))
        err = float((got * un - want).abs().max())
        print("transposed image err %.3e of max %.3e" % (err, float(want.abs().max())))
        assert err <= 2.0 ** -21 * float(want.abs().max())            # two f16 pieces: 22 bits of the largest entry
        assert torch.count_nonzero((got * un)[want == 0]) == 0         # padding and t's slot: exact zeros

    offset = 0
    for lin in lins[1:-1]:
        check(unpack(fragt[offset:offset + 16 * 512], 4), lin.weight, 64, 64)
        offset += 16 * 512
    first = lins[0].weight.detach().clone()
    first[:, 0] = 0
    check(unpack(fragt[offset:], 2), first, 32, 64)


_cases = {}


def _inverse_case(name):
    if name not in _cases:
        z = U.fixture(name)
        far = int(z["far_rows"])
        module = U.build(name).double()
        y = U.tensor(z, "y64")[far:]
        ctx = U.tensor(z, "context", torch.float64)
        ctx = None if ctx is None else ctx[far:]
        gen = torch.Generator().manual_seed(5)
        gx = torch.randn(y.shape, generator=gen, dtype=torch.float64)
        gl = torch.randn(y.shape[0], generator=gen, dtype=torch.float64)
        with torch.no_grad():
            plain = module.inverse(y, ctx)
        _cases[name] = (module, y, ctx, gx, gl, plain, G.autograd_grads(module, y, ctx, gx, gl, inverse=True))
    return _cases[name]


@pytest.mark.parametrize("name", U.FIXTURES)
def test_inverse_under_autograd_returns_the_same_values(name):
    module, y, ctx, gx, gl, plain, (x, lad, grads) = _inverse_case(name)
    assert torch.equal(x, plain[0]) and torch.equal(lad, plain[1])


@pytest.mark.parametrize("name", U.FIXTURES)
def test_inverse_carries_the_implicit_function_gradient(name):
    """Fails before the root was re-attached: x came out of a no_grad search and carried no gradient."""
    module, y, ctx, gx, gl, plain, (x, lad, grads) = _inverse_case(name)
    root, _, want = G.implicit_inverse_grads(module, y, ctx, gx, gl)
    assert torch.equal(root, x)
    assert set(want) == set(grads)
    for key in sorted(want):
        err, scale = U.maxdiff(grads[key], want[key]), float(want[key].abs().max())
        print("%s %s: err %.3e of max %.3e" % (name, key, err, scale))
        assert err <= 1e-9 * scale, (name, key, err, scale)
    assert float(want["inputs"].abs().max()) > 0
