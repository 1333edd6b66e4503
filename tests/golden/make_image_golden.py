"""Generate tests/golden/image_*.npz (flows on images) by importing the REFERENCE (FlowConductor) itself.

Runs only where the reference tree exists:
    python tests/golden/make_image_golden.py
It uses make_golden.py's import (with its placeholder for the third-party ``UMNN`` package).
- image_squeeze.npz: SqueezeTransform with factors 2 and 3 on odd channel counts, both directions.
- image_conv_c<C>.npz: OneByOneConvolution(C) with random L / U / bias (not the identity), both directions: inputs, the
  reference's float32 outputs / logabsdets, the same in float64 (keys ending in 64), and its state_dict (``sd::``).
- image_flow.npz: a two-level multiscale Glow-style flow (Squeeze, 2 x (ActNorm, 1x1 conv, affine coupling with a
  ConvResidualNet) per level) in eval mode with ActNorm initialised: its state_dict, log_prob of fixed inputs, the
  inverse of fixed noise (float32 and float64), and float64 gradients of the mean negative log-likelihood with respect
  to every parameter (``grad::`` keys, stored as float32).
These fixtures are not part of cases.CASES.
"""
import copy
import os

import numpy as np
import torch

from make_golden import HERE, import_reference

CONV_SIZES = {1: (4, 5, 7), 3: (4, 6, 6), 12: (3, 5, 4), 48: (2, 4, 4), 128: (2, 3, 4)}


def both(t, x, inverse):
    """The reference module in float32 and a float64 copy of it."""
    with torch.no_grad():
        f = t.inverse if inverse else t
        y, lad = f(x)
        t64 = copy.deepcopy(t).double()
        f64 = t64.inverse if inverse else t64
        y64, lad64 = f64(x.double())
    return [a.numpy() for a in (y, lad, y64, lad64)]


def squeeze_case(L):
    T = L.transforms
    gen = torch.Generator().manual_seed(5)
    out = {}
    for f, fwd_shape, inv_shape in ((2, (2, 3, 6, 8), (2, 12, 3, 5)), (3, (2, 5, 6, 9), (1, 36, 2, 3))):
        t = T.SqueezeTransform(factor=f)
        x = torch.randn(*fwd_shape, generator=gen)
        z = torch.randn(*inv_shape, generator=gen)
        with torch.no_grad():
            out["f%d_x" % f], out["f%d_y" % f] = x.numpy(), t(x)[0].numpy()
            out["f%d_inv_x" % f], out["f%d_inv_y" % f] = z.numpy(), t.inverse(z)[0].numpy()
    np.savez_compressed(os.path.join(HERE, "image_squeeze.npz"), **out)


def conv_cases(L):
    T = L.transforms
    for c, (n, h, w) in CONV_SIZES.items():
        torch.manual_seed(100 + c)
        t = T.OneByOneConvolution(c, identity_init=False)
        with torch.no_grad():
            t.bias.uniform_(-0.5, 0.5)
        gen = torch.Generator().manual_seed(200 + c)
        x = torch.randn(n, c, h, w, generator=gen)
        z = torch.randn(n, c, h, w, generator=gen)
        out = {"fwd_x": x.numpy(), "inv_x": z.numpy()}
        out["fwd_y"], out["fwd_lad"], out["fwd_y64"], out["fwd_lad64"] = both(t, x, False)
        out["inv_y"], out["inv_lad"], out["inv_y64"], out["inv_lad64"] = both(t, z, True)
        out.update({"sd::" + k: v.detach().numpy() for k, v in t.state_dict().items()})
        path = os.path.join(HERE, "image_conv_c%d.npz" % c)
        np.savez_compressed(path, **out)
        print(path, os.path.getsize(path))


def build_image_flow(L):
    """Input [B, 3, 16, 16]; level 1: Squeeze + 2 Glow steps on 12 channels, half split off; level 2: Squeeze + 2 steps on
    24 channels.  The same builder runs against this package in tests/test_gpu_image.py."""
    T, nets, utils = L.transforms, L.nets, L.utils

    def net(i, o):
        return nets.ConvResidualNet(in_channels=i, out_channels=o, hidden_channels=16)

    def steps(c):
        layers = []
        for _ in range(2):
            layers += [T.ActNorm(c), T.OneByOneConvolution(c),
                       T.AffineCouplingTransform(mask=utils.create_mid_split_binary_mask(c), transform_net_create_fn=net)]
        return layers

    ms = T.MultiscaleCompositeTransform(2)
    hidden = ms.add_transform(T.CompositeTransform([T.SqueezeTransform()] + steps(12)), (12, 8, 8))
    assert hidden == (6, 8, 8)
    assert ms.add_transform(T.CompositeTransform([T.SqueezeTransform()] + steps(24)), (24, 4, 4)) is None
    return L.flows.Flow(ms, L.distributions.StandardNormal([768]))


def flow_case(L):
    torch.manual_seed(17)
    flow = build_image_flow(L)
    gen = torch.Generator().manual_seed(23)
    x = torch.randn(4, 3, 16, 16, generator=gen) * 0.8 + 0.1
    noise = torch.randn(4, 768, generator=gen)
    with torch.no_grad():
        flow.train()
        flow.log_prob(torch.randn(16, 3, 16, 16, generator=gen))  # ActNorm data-dependent initialisation
        for p in flow.parameters():
            p.add_(0.05 * torch.randn(p.shape, generator=gen))
    flow.eval()
    out = {"x": x.numpy(), "noise": noise.numpy()}
    with torch.no_grad():
        out["log_prob"] = flow.log_prob(x).numpy()
        out["sample"] = flow._transform.inverse(noise)[0].numpy()
        f64 = copy.deepcopy(flow).double()
        out["log_prob64"] = f64.log_prob(x.double()).numpy()
        out["sample64"] = f64._transform.inverse(noise.double())[0].numpy()
    f64 = copy.deepcopy(flow).double().train()
    loss = -f64.log_prob(x.double()).mean()
    loss.backward()
    out["loss64"] = np.array(loss.item())
    out.update({"grad::" + k: p.grad.float().numpy() for k, p in f64.named_parameters()})
    out.update({"sd::" + k: v.detach().numpy() for k, v in flow.state_dict().items()})
    path = os.path.join(HERE, "image_flow.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path))


def main():
    L = import_reference()
    squeeze_case(L)
    conv_cases(L)
    flow_case(L)


if __name__ == "__main__":
    main()
