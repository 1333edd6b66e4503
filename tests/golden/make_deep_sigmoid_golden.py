"""Generate tests/golden/deep_sigmoid_<case>.npz (deep sigmoidal flow) by importing the REFERENCE (FlowConductor) itself.

Runs only where the reference tree exists:
    python tests/golden/make_deep_sigmoid_golden.py
It uses make_golden.py's import (with its placeholder for the third-party ``UMNN`` package).

* ``deep_sigmoid_ds_f<F>_s<S>_m<mollify %>.npz`` for the (features, S, mollify) of ``DS_CASES``:
  ``flowcon.transforms.DeepSigmoid`` with ``dsparams`` perturbed by unit normal noise.
* ``deep_sigmoid_ps_f6_s8.npz``: ``forward_given_params`` with per-sample ``dsparams`` [257, 6, 24] (recorded as data).
* ``deep_sigmoid_made_d<D>_h<hidden>_s<S>_ctx<C>.npz`` for the (D, hidden, S, context) of ``MADE_CASES``:
  ``MaskedDeepSigmoidTransform`` with every parameter multiplied by 1.5, the residual blocks' (near-)zero-initialised last
  layers perturbed and the final layer multiplied by 4, so that the parameters vary over the batch.

Every file holds the ``sd::`` state_dict entries, ``x`` [257, F] (``DeepSigmoid`` / per-sample: 3 randn with the first
``far_rows`` = 8 rows at +-50; MADE: 2 randn, ``far_rows`` = 0), ``context`` where there is one, the reference's float32
``y32`` / ``lad32``, ``y64`` / ``lad64`` from a ``.double()`` deep copy, the upstream gradients ``gy`` / ``gl`` and the
float64 gradients of ``(y * gy).sum() + (lad * gl).sum()`` with respect to ``x`` (``grad_x64``) and to every parameter
(``grad64::<name>``; ``grad_dsparams64`` for the per-sample case), and the float32 noise floors max|32 - 64| of outputs
and logabsdet over the ordinary rows (``floor_y_body`` / ``floor_lad_body``) and over the pushed rows (``..._far``).
The non-MADE files also hold an inverse block: ``x_inv`` = 1.5 randn [128, F] with ``y32_inv`` / ``lad32_inv``, the
float64 ``y64_inv`` / ``lad64_inv`` and their floors ``floor_y_inv`` / ``floor_lad_inv``.
If a file came out larger than the other fixtures, the widest case would drop its parameter gradients, as
make_mog_golden.py does; none needs to.  These fixtures are not part of cases.CASES.
"""
import copy
import os

import numpy as np
import torch

from make_golden import HERE, import_reference

ROWS = 257
FAR_ROWS = 8
INV_ROWS = 128
DS_CASES = [(7, 1, 0.0), (7, 4, 0.0), (5, 30, 0.0), (3, 4, 0.25), (70, 4, 0.0)]
MADE_CASES = [(5, 32, 30, None), (6, 24, 8, 3), (33, 16, 4, None)]
SIZE_LIMIT = 900 * 1024


def floors(out, tag, a32, a64, far):
    diff = (a32.double() - a64.detach()).abs()
    diff = diff.reshape(diff.shape[0], -1).max(dim=1).values
    out["floor_%s_body" % tag] = np.float64(diff[far:].max().item())
    out["floor_%s_far" % tag] = np.float64(diff[:far].max().item() if far else 0.0)


def record(name, module, x, gen, far, call=None, context=None, extra=None, x_inv=None):
    """``call(module, x, context, leaves)`` -> (y, lad); ``extra``: {key: tensor} of data leaves that also get gradients."""
    call = call or (lambda m, v, c, leaves: m(v, c))
    extra = extra or {}
    out = {"sd::" + k: v.detach().clone().numpy() for k, v in module.state_dict().items()}
    out["x"], out["far_rows"] = x.numpy(), np.int64(far)
    if context is not None:
        out["context"] = context.numpy()
    for k, v in extra.items():
        out[k] = v.numpy()
    with torch.no_grad():
        y32, lad32 = call(module, x.clone(), context, extra)
    m64 = copy.deepcopy(module).double()
    x64 = x.double().requires_grad_(True)
    leaves64 = {k: v.double().requires_grad_(True) for k, v in extra.items()}
    y64, lad64 = call(m64, x64, None if context is None else context.double(), leaves64)
    gy = torch.randn(y64.shape, generator=gen)
    gl = torch.randn(lad64.shape, generator=gen)
    ((y64 * gy.double()).sum() + (lad64 * gl.double()).sum()).backward()
    for t in (y32, lad32, y64, lad64, x64.grad):
        assert torch.isfinite(t).all(), name
    out.update(y32=y32.numpy(), lad32=lad32.numpy(), y64=y64.detach().numpy(), lad64=lad64.detach().numpy(),
               gy=gy.numpy(), gl=gl.numpy(), grad_x64=x64.grad.numpy())
    for k, v in leaves64.items():
        assert torch.isfinite(v.grad).all(), name
        out["grad_%s64" % k] = v.grad.numpy()
    for pname, p in m64.named_parameters():
        if p.grad is not None:
            assert torch.isfinite(p.grad).all(), (name, pname)
            out["grad64::" + pname] = p.grad.numpy()
    floors(out, "y", y32, y64, far)
    floors(out, "lad", lad32, lad64, far)
    if x_inv is not None:
        with torch.no_grad():
            yi32, li32 = call(module, x_inv.clone(), context, {k: v[:x_inv.shape[0]] for k, v in extra.items()})
            yi64, li64 = call(m64, x_inv.double(), None, {k: v.double()[:x_inv.shape[0]] for k, v in extra.items()})
        assert torch.isfinite(yi32).all() and torch.isfinite(li32).all()
        out.update(x_inv=x_inv.numpy(), y32_inv=yi32.numpy(), lad32_inv=li32.numpy(), y64_inv=yi64.numpy(),
                   lad64_inv=li64.numpy())
        out["floor_y_inv"] = np.float64((yi32.double() - yi64).abs().max().item())
        out["floor_lad_inv"] = np.float64((li32.double() - li64).abs().max().item())
    path = os.path.join(HERE, "deep_sigmoid_%s.npz" % name)
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size <= SIZE_LIMIT, (name, size)
    print("%-28s floor y body %.2e far %.2e | lad body %.2e far %.2e | inv y %.2e lad %.2e | max|y_inv| %.2f | %d bytes"
          % (name, out["floor_y_body"], out["floor_y_far"], out["floor_lad_body"], out["floor_lad_far"],
             out.get("floor_y_inv", float("nan")), out.get("floor_lad_inv", float("nan")),
             float(np.abs(out["y32_inv"]).max()) if x_inv is not None else float("nan"), size))


def inputs(features, gen, scale, far):
    x = scale * torch.randn(ROWS, features, generator=gen)
    if far:
        x[:far] = torch.tensor([50.0, -50.0] * (far // 2)).reshape(-1, 1)
    return x


def main():
    L = import_reference()
    T = L.transforms
    seed = 700
    for features, n_sigmoids, mollify in DS_CASES:
        seed += 1
        gen = torch.Generator().manual_seed(seed)
        torch.manual_seed(seed)
        module = T.DeepSigmoid(features, n_sigmoids=n_sigmoids, mollify=mollify)
        with torch.no_grad():
            module.dsparams.add_(torch.randn(module.dsparams.shape, generator=gen))
        record("ds_f%d_s%d_m%d" % (features, n_sigmoids, round(100 * mollify)), module, inputs(features, gen, 3.0, FAR_ROWS),
               gen, FAR_ROWS, x_inv=1.5 * torch.randn(INV_ROWS, features, generator=gen))

    seed += 1
    gen = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    module = T.DeepSigmoid(6, n_sigmoids=8)
    dsparams = module.dsparams.detach()[None] + torch.randn(ROWS, 6, 24, generator=gen)
    record("ps_f6_s8", module, inputs(6, gen, 3.0, FAR_ROWS), gen, FAR_ROWS,
           call=lambda m, v, c, leaves: m.forward_given_params(v, dsparams=leaves["dsparams"]),
           extra={"dsparams": dsparams}, x_inv=1.5 * torch.randn(INV_ROWS, 6, generator=gen))

    for features, hidden, n_sigmoids, context_features in MADE_CASES:
        seed += 1
        gen = torch.Generator().manual_seed(seed)
        torch.manual_seed(seed)
        module = T.autoregressive.MaskedDeepSigmoidTransform(features, hidden, n_sigmoids=n_sigmoids, context_features=context_features)
        with torch.no_grad():
            for p in module.parameters():
                p.mul_(1.5)
            for block in module.autoregressive_net.blocks:
                last = block.linear_layers[-1]
                last.weight.add_(0.3 / hidden ** 0.5 * torch.randn(last.weight.shape, generator=gen))
                last.bias.add_(0.1 * torch.randn(last.bias.shape, generator=gen))
            module.autoregressive_net.final_layer.weight.mul_(4.0)
            module.autoregressive_net.final_layer.bias.mul_(4.0)
        module.eval()
        context = torch.randn(ROWS, context_features, generator=gen) if context_features else None
        record("made_d%d_h%d_s%d_ctx%d" % (features, hidden, n_sigmoids, context_features or 0), module,
               inputs(features, gen, 2.0, 0), gen, 0, context=context)


if __name__ == "__main__":
    main()
