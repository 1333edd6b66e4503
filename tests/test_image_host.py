"""Host-side checks of the image-flow layers (no GPU): exports, constructor errors and messages, state_dict keys of the
reference's fixtures, MultiscaleCompositeTransform bookkeeping, the SqueezeTransform inverse quirk and the new ABI
entries."""
import ctypes
import os
import re

import pytest
import torch

from _util import golden
from flowconductor_amd import _hip, distributions, flows, nn as fc_nn, ops, transforms, utils
from flowconductor_amd.nn import nets

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Lib:
    transforms, nets, utils, flows, distributions = transforms, nets, utils, flows, distributions


def build_image_flow():
    from make_image_golden import build_image_flow as build
    return build(_Lib)


def test_exports():
    for name in ("SqueezeTransform", "OneByOneConvolution", "MultiscaleCompositeTransform"):
        assert hasattr(transforms, name), name
    assert nets.ConvResidualNet is fc_nn.ConvResidualNet
    assert nets.ConvResidualBlock is fc_nn.ConvResidualBlock
    assert issubclass(transforms.OneByOneConvolution, transforms.LULinear)


def test_squeeze_constructor_and_shape():
    for bad in (1, 0, -2, 2.0, "2"):
        with pytest.raises(ValueError, match="Factor must be an integer > 1."):
            transforms.SqueezeTransform(factor=bad)
    t = transforms.SqueezeTransform(factor=3)
    assert t.get_output_shape(5, 9, 12) == (45, 3, 4)
    assert transforms.SqueezeTransform().factor == 2


def test_squeeze_input_checks():
    t = transforms.SqueezeTransform()
    with pytest.raises(ValueError, match="Expecting inputs with 4 dimensions"):
        t(torch.zeros(2, 3, 4))
    with pytest.raises(ValueError, match="Input image size not compatible with the factor."):
        t(torch.zeros(2, 3, 4, 5))
    with pytest.raises(ValueError, match="Expecting inputs with 4 dimensions"):
        t.inverse(torch.zeros(2, 8, 4))


def test_squeeze_inverse_quirk():
    """The inverse checks c >= 4 and c % 4 == 0 for every factor (the reference's check)."""
    with pytest.raises(ValueError, match="Invalid number of channel dimensions."):
        transforms.SqueezeTransform(2).inverse(torch.zeros(1, 2, 3, 3))
    with pytest.raises(ValueError, match="Invalid number of channel dimensions."):
        transforms.SqueezeTransform(3).inverse(torch.zeros(1, 9, 3, 3))    # a multiple of 9 but not of 4
    with pytest.raises(RuntimeError, match="is invalid for input of size"):
        transforms.SqueezeTransform(3).inverse(torch.zeros(1, 8, 3, 3))    # passes the check, fails the reshape


def test_conv_constructor_and_errors():
    t = transforms.OneByOneConvolution(4)
    assert t.using_cache is False and t.features == 4
    assert isinstance(t.permutation, transforms.RandomPermutation) and t.permutation._dim == 1
    with pytest.raises(ValueError, match="Inputs must be a 4D tensor."):
        t(torch.zeros(3, 4))
    with pytest.raises(ValueError, match="Inputs must be a 4D tensor."):
        t.inverse(torch.zeros(3, 4, 2))
    # identity_init: W = I at initialisation
    lower, upper = t._create_lower_upper()
    assert torch.allclose(lower @ upper, torch.eye(4))


@pytest.mark.parametrize("c", (1, 3, 12, 48, 128))
def test_conv_state_dict_matches_fixture(c):
    g = golden("image_conv_c%d" % c)
    sd = {k[4:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("sd::")}
    t = transforms.OneByOneConvolution(c)
    assert set(t.state_dict()) == set(sd)
    t.load_state_dict(sd, strict=True)
    assert torch.equal(t.permutation._permutation, sd["permutation._permutation"])


def test_image_flow_state_dict_matches_fixture():
    g = golden("image_flow")
    sd = {k[4:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("sd::")}
    flow = build_image_flow()
    assert set(flow.state_dict()) == set(sd)
    flow.load_state_dict(sd, strict=True)
    grads = {k[6:] for k in g.files if k.startswith("grad::")}
    assert grads == {k for k, _ in flow.named_parameters()}


def test_conv_residual_net_keys_and_init():
    torch.manual_seed(0)
    net = nets.ConvResidualNet(in_channels=3, out_channels=8, hidden_channels=16, context_channels=2, num_blocks=2)
    keys = set(net.state_dict())
    for k in ("initial_layer.weight", "final_layer.bias", "blocks.0.conv_layers.0.weight", "blocks.1.conv_layers.1.bias",
              "blocks.1.context_layer.weight"):
        assert k in keys
    assert net.initial_layer.in_channels == 5 and net.initial_layer.kernel_size == (1, 1)
    last = net.blocks[0].conv_layers[-1]
    assert last.weight.abs().max() <= 1e-3 and last.bias.abs().max() <= 1e-3
    x, ctx = torch.randn(2, 3, 5, 5), torch.randn(2, 2, 5, 5)
    assert net(x, ctx).shape == (2, 8, 5, 5)
    bn = nets.ConvResidualBlock(channels=4, use_batch_norm=True)
    assert "batch_norm_layers.1.running_mean" in bn.state_dict()


def test_multiscale_bookkeeping():
    with pytest.raises(TypeError, match="Split dimension must be a positive integer."):
        transforms.MultiscaleCompositeTransform(2, split_dim=0)
    with pytest.raises(TypeError, match="Split dimension must be a positive integer."):
        transforms.MultiscaleCompositeTransform(2, split_dim=1.0)
    ms = transforms.MultiscaleCompositeTransform(3)
    with pytest.raises(ValueError, match="No split_dim in output shape"):
        transforms.MultiscaleCompositeTransform(2, split_dim=4).add_transform(transforms.IdentityTransform(), (4, 2, 2))
    with pytest.raises(ValueError, match="Size of dimension 1 must be at least 2."):
        ms.add_transform(transforms.IdentityTransform(), (1, 4, 4))
    assert ms.add_transform(transforms.IdentityTransform(), (5, 8, 8)) == (2, 8, 8)
    assert ms.add_transform(transforms.IdentityTransform(), (8, 4, 4)) == (4, 4, 4)
    assert ms.add_transform(transforms.IdentityTransform(), (16, 2, 2)) is None
    assert ms._output_shapes == [(3, 8, 8), (4, 4, 4), (16, 2, 2)]
    with pytest.raises(RuntimeError, match="Adding more than 3 transforms is not allowed."):
        ms.add_transform(transforms.IdentityTransform(), (16, 2, 2))
    with pytest.raises(ValueError, match="Expecting NxD inputs"):
        ms.inverse(torch.zeros(2, 3, 4))
    part = transforms.MultiscaleCompositeTransform(2)
    part.add_transform(transforms.IdentityTransform(), (4, 2, 2))
    with pytest.raises(RuntimeError, match=r"Expecting exactly 2 transform\(s\) to be added."):
        part(torch.zeros(1, 4, 2, 2))
    with pytest.raises(RuntimeError, match=r"Expecting exactly 2 transform\(s\) to be added."):
        part.inverse(torch.zeros(1, 16))
    with pytest.raises(ValueError, match="No split_dim in inputs."):
        transforms.MultiscaleCompositeTransform(1, split_dim=2)(torch.zeros(3, 4))


def test_multiscale_split_and_merge_on_host():
    """Pure-torch children: the chunk / flatten / concatenate bookkeeping and its inverse."""
    ms = transforms.MultiscaleCompositeTransform(2)
    hidden = ms.add_transform(transforms.IdentityTransform(), (5, 2, 3))
    assert hidden == (2, 2, 3)
    ms.add_transform(transforms.IdentityTransform(), hidden)
    x = torch.randn(4, 5, 2, 3)
    y, lad = ms(x)
    assert y.shape == (4, 30) and not lad.any()
    assert torch.equal(y[:, :18], x[:, :3].reshape(4, -1)) and torch.equal(y[:, 18:], x[:, 3:].reshape(4, -1))
    back, lad_inv = ms.inverse(y)
    assert torch.equal(back, x) and not lad_inv.any()


def test_new_abi_entries():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "flowcon_hip.h")).read(), flags=re.S)
    lib = ctypes.CDLL(_hip.LIB_PATH)
    for name in ("fc_squeeze", "fc_conv1x1"):
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
        assert name in _hip.SIGNATURES
        assert hasattr(lib, name)
    assert "#define FC_CONV1X1_MAX_CHANNELS 128" in text
    assert ops.CONV1X1_MAX_CHANNELS == 128


def test_kernels_refuse_host_tensors():
    """No CPU fallback for the kernel paths."""
    with pytest.raises(RuntimeError, match="HIP device"):
        transforms.SqueezeTransform()(torch.zeros(1, 1, 2, 2))
    with torch.no_grad(), pytest.raises(RuntimeError, match="HIP device"):
        transforms.OneByOneConvolution(3)(torch.zeros(1, 3, 2, 2))
