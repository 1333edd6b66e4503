"""Shared by tests/test_iresblock_training_host.py and tests/test_gpu_iresblock_training.py: training an ``iResBlock``
with the exact determinant as one autograd node (options ``iresblock_training``).

``reverse_sweep`` restates in float64 torch what ``fc_iresnet_backward`` computes: the forward as one computation with
D + 1 streams per row (a value stream h and tangent streams t_j), the cotangents ``s gy`` on the value stream's output
and ``gl s (A^-T)[:, j]`` on tangent stream j's, and plain reverse mode over the layers, the adjoint of a
pre-activation collecting ``eta2 act'' (W t_in) adj_t_out`` from every tangent stream.  The host test pins it to
``torch.autograd`` on the package's float64 composition; ``act_jet`` holds the nine activations' derivatives."""
import copy

import torch

from flowconductor_amd import ops, transforms
from flowconductor_amd.nn import nets
from flowconductor_amd.nn.nets import activations

CONTEXT = 3
SMALL = dict(c_embed_hidden_sizes=(16, 16, 6))

ACTIVATIONS = {      # one per kernel activation id
    "relu": lambda: "relu",
    "tanh": lambda: "tanh",
    "elu": lambda: "elu",
    "swish": lambda: "swish",
    "lipswish": lambda: activations.LipSwish(),
    "clipswish": lambda: "CLipSwish",
    "sin": lambda: activations.Sin(3.0),
    "csin": lambda: activations.CSin(10),
    "leaky_lswish": lambda: "LeakyLSwish",
}


def act_jet(act, t, p0, p1):
    """``f, f', f'', df/dp0, df'/dp0, df/dp1, df'/dp1`` of kernel activation ``act`` at ``t`` (float64 tensors)."""
    zero = torch.zeros_like(t)
    jet = dict(f=zero, df=zero, d2f=zero, f_p0=zero, df_p0=zero, f_p1=zero, df_p1=zero)
    if act == ops.IRES_ACT_RELU:
        jet.update(f=torch.where(t > 0, t, zero), df=(t > 0).to(t))
    elif act == ops.IRES_ACT_TANH:
        th = torch.tanh(t)
        jet.update(f=th, df=1 - th * th, d2f=-2 * th * (1 - th * th))
    elif act == ops.IRES_ACT_ELU:
        pos = t > 0
        jet.update(f=torch.where(pos, t, p0 * torch.expm1(t)), df=torch.where(pos, torch.ones_like(t), p0 * torch.exp(t)),
                   d2f=torch.where(pos, zero, p0 * torch.exp(t)), f_p0=torch.where(pos, zero, torch.expm1(t)),
                   df_p0=torch.where(pos, zero, torch.exp(t)))
    elif act in (ops.IRES_ACT_SIN, ops.IRES_ACT_CSIN):
        div = 2.0 ** 0.5 if act == ops.IRES_ACT_CSIN else 1.0
        a = p0 * t
        jet.update(f=torch.sin(a) / (p0 * div), df=torch.cos(a) / div, d2f=-p0 * torch.sin(a) / div,
                   f_p0=(a * torch.cos(a) - torch.sin(a)) / (p0 * p0 * div), df_p0=-t * torch.sin(a) / div)
    else:
        sg = torch.sigmoid(p0 * t)
        q = sg * (1 - sg)
        bend = q * (2 + p0 * t * (1 - 2 * sg)) / 1.1
        v, dv, d2v, v_p0, dv_p0 = t * sg / 1.1, (sg + p0 * t * q) / 1.1, p0 * bend, t * t * q / 1.1, t * bend
        if act in (ops.IRES_ACT_LIPSWISH, ops.IRES_ACT_CLIPSWISH):
            v, dv, d2v, v_p0, dv_p0 = (z / 1.004 for z in (v, dv, d2v, v_p0, dv_p0))
        elif act == ops.IRES_ACT_LEAKY_LSWISH:
            jet.update(f_p1=t - v, df_p1=1 - dv)
            v, dv = p1 * t + (1 - p1) * v, p1 + (1 - p1) * dv
            d2v, v_p0, dv_p0 = (1 - p1) * d2v, (1 - p1) * v_p0, (1 - p1) * dv_p0
        else:
            assert act == ops.IRES_ACT_SWISH
        jet.update(f=v, df=dv, d2f=d2v, f_p0=v_p0, df_p0=dv_p0)
    return jet


def layout(d, e, depth, growth, act):
    """Offsets of the image's pieces (include/flowcon_hip.h): ``layers`` = [(offset, w_in)], ``final`` = offset."""
    concat = act in ops.IRES_CONCAT_ACTS
    out_ch = growth // 2 if concat else growth
    op, dp = ops._pad4(out_ch), ops._pad4(d)
    at, w_in, layers = 4, d + e, []
    for _ in range(depth):
        layers.append((at, w_in))
        at += 4 + op + w_in * op
        w_in += growth
    assert at + dp + w_in * dp == ops.iresnet_image_floats(d, e, depth, growth, act)
    return dict(concat=concat, out_ch=out_ch, op=op, dp=dp, layers=layers, final=at, wtot=w_in)


def reverse_sweep(image, shape, x, gy, gl, extra=None, scale=None):
    """``(y, logabsdet, dx, dimage, dextra, dscale)`` in float64 from a float64 ``image`` of the net."""
    d, e, depth, growth, act = shape
    lay = layout(*shape)
    out_ch, op, dp, concat = lay["out_ch"], lay["op"], lay["dp"], lay["concat"]
    n = x.shape[0]
    p0, p1 = image[0], image[1]
    sc = torch.ones(n, dtype=x.dtype) if scale is None else scale
    h = x if extra is None else torch.cat([x, extra], 1)
    t = torch.zeros(n, d, d + e, dtype=x.dtype)
    t[:, :, :d] = torch.eye(d, dtype=x.dtype)
    tape = []
    for at, w_in in lay["layers"]:
        eta1, eta2 = image[at], image[at + 1]
        bias = image[at + 4:at + 4 + out_ch]
        w = image[at + 4 + op:at + 4 + op + w_in * op].view(w_in, op)[:, :out_ch]
        pre, u = h @ w + bias, t @ w
        j1 = act_jet(act, pre, p0, p1)
        j2 = act_jet(act, -pre, p0, p1) if concat else None
        tape.append((h, t, u, j1, j2))
        fs = [j1["f"]] + ([j2["f"]] if concat else [])
        ts = [j1["df"].unsqueeze(1) * u] + ([-j2["df"].unsqueeze(1) * u] if concat else [])
        h = torch.cat([eta1 * h, eta2 * torch.cat(fs, 1)], 1)
        t = torch.cat([eta1 * t, eta2 * torch.cat(ts, 2)], 2)
    at = lay["final"]
    wf = image[at + dp:at + dp + lay["wtot"] * dp].view(lay["wtot"], dp)[:, :d]
    g = h @ wf + image[at:at + d]
    jac = (t @ wf).transpose(1, 2)                      # jac[n, i, j] = dg_i / dx_j
    a = torch.eye(d, dtype=x.dtype) + sc.view(n, 1, 1) * jac
    y, lad = x + sc.unsqueeze(1) * g, torch.linalg.slogdet(a)[1]

    a_inv = torch.linalg.inv(a)
    c_h = sc.unsqueeze(1) * gy                           # cotangent of g
    c_t = (gl * sc).view(n, 1, 1) * a_inv                # c_t[n, j, i]: cotangent of column j of the Jacobian
    dscale = (gy * g).sum(1) + gl * torch.einsum("nji,nij->n", a_inv, jac)
    dimage = torch.zeros_like(image)
    dwf = torch.zeros(lay["wtot"], dp, dtype=x.dtype)
    dwf[:, :d] = h.t() @ c_h + torch.einsum("njk,nji->ki", t, c_t)
    dimage[at + dp:at + dp + lay["wtot"] * dp] = dwf.reshape(-1)
    dimage[at:at + d] = c_h.sum(0)
    adj_h, adj_t = c_h @ wf.t(), c_t @ wf.t()
    for (at, w_in), (h_in, t_in, u, j1, j2) in zip(reversed(lay["layers"]), reversed(tape)):
        eta1, eta2 = image[at], image[at + 1]
        w = image[at + 4 + op:at + 4 + op + w_in * op].view(w_in, op)[:, :out_ch]
        a1h, a1t = adj_h[:, w_in:w_in + out_ch], adj_t[:, :, w_in:w_in + out_ch]
        zero_h, zero_t = torch.zeros_like(a1h), torch.zeros_like(a1t)
        a2h, a2t = (adj_h[:, w_in + out_ch:w_in + 2 * out_ch], adj_t[:, :, w_in + out_ch:w_in + 2 * out_ch]) \
            if concat else (zero_h, zero_t)
        if j2 is None:
            j2 = {k: zero_h for k in j1}
        df1, df2 = j1["df"].unsqueeze(1), j2["df"].unsqueeze(1)
        adj_u = eta2 * (df1 * a1t - df2 * a2t)
        adj_pre = eta2 * (j1["df"] * a1h - j2["df"] * a2h) \
            + eta2 * ((j1["d2f"].unsqueeze(1) * a1t + j2["d2f"].unsqueeze(1) * a2t) * u).sum(1)
        dimage[at] = (adj_h[:, :w_in] * h_in).sum() + (adj_t[:, :, :w_in] * t_in).sum()
        dimage[at + 1] = (j1["f"] * a1h + j2["f"] * a2h).sum() + (u * (df1 * a1t - df2 * a2t)).sum()
        for key, slot in (("p0", 0), ("p1", 1)):
            dimage[slot] += eta2 * ((j1["f_" + key] * a1h + j2["f_" + key] * a2h).sum()
                                    + (u * (j1["df_" + key].unsqueeze(1) * a1t - j2["df_" + key].unsqueeze(1) * a2t)).sum())
        dw = torch.zeros(w_in, op, dtype=x.dtype)
        dw[:, :out_ch] = h_in.t() @ adj_pre + torch.einsum("njk,njo->ko", t_in, adj_u)
        dimage[at + 4 + op:at + 4 + op + w_in * op] = dw.reshape(-1)
        dimage[at + 4:at + 4 + out_ch] = adj_pre.sum(0)
        adj_h = eta1 * adj_h[:, :w_in] + adj_pre @ w.t()
        adj_t = eta1 * adj_t[:, :, :w_in] + adj_u @ w.t()
    dx = gy + adj_h[:, :d]
    return y, lad, dx, dimage, (adj_h[:, d:] if e else None), (dscale if scale is not None else None)


def make_block(net, seed, context_features=0, rough=True):
    """A brute-force block with non-trivial weights: alternate layers scaled past and below the Lipschitz coefficient
    (so the spectral clamp is active on some and its gradient through sigma non-zero), perturbed biases, concatenation
    weights and activation scalars, power-method vectors moved by a few training-mode calls; eval mode."""
    block = transforms.iResBlock(net, brute_force=True)
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        index = 0
        for name, p in block.nnet.named_parameters():
            if name.endswith("parametrizations.weight.original"):
                if rough:
                    p.mul_(2.5 if index % 2 == 0 else 0.6)
                index += 1
            elif (name.endswith("bias") and "dense_net" in name) or "unnormalized" in name or name.endswith("beta") \
                    or name.endswith("alpha"):
                p.add_(0.2 * torch.randn(p.shape, generator=gen))
    block.train()
    d = block.nnet.dimension
    context = torch.randn(32, context_features, generator=gen) if context_features else None
    for _ in range(10):
        block(torch.randn(32, d, generator=gen), context)
    return block.eval()


def conditional_net(kind, d=3, act="swish"):
    if kind == "input":
        return nets.InputConditionalDenseNet(dimension=d, context_features=CONTEXT, densenet_depth=2, densenet_growth=8,
                                             activation_function=ACTIVATIONS[act](), **SMALL)
    return nets.MultiplicativeAndInputConditionalDenseNet(
        dimension=d, context_features=CONTEXT, densenet_depth=2, densenet_growth=8,
        activation_function=ACTIVATIONS[act](), m_embed_hidden_sizes=(16, 16), **SMALL)


def named_gradients(block, x, context, gy, gl, inverse=False):
    """``{name: gradient}`` of ``<gy, y> + <gl, logabsdet>`` with respect to the rows (``"x"``), the context and every
    parameter that receives one, and the outputs ``(y, logabsdet)``, on whichever route ``block`` takes."""
    block.zero_grad()
    x = x.detach().clone().requires_grad_(True)
    context = None if context is None else context.detach().clone().requires_grad_(True)
    y, lad = (block.inverse if inverse else block)(x, context)
    ((gy * y).sum() + (gl * lad).sum()).backward()
    grads = {"x": x.grad.detach().clone()}
    if context is not None:
        grads["context"] = context.grad.detach().clone()
    for name, p in block.named_parameters():
        if p.grad is not None:
            grads[name] = p.grad.detach().clone()
    block.zero_grad()
    return grads, (y.detach(), lad.detach())


def double_copy(block):
    return copy.deepcopy(block).cpu().double()
