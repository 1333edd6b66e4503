"""Generate tests/golden/svd_linear_<case>.npz and qr_linear_<case>.npz by importing the REFERENCE (FlowConductor) itself.

Runs only where the reference tree exists:
    python tests/golden/make_linear_family_golden.py
It uses make_golden.py's import.  Every case builds ``flowcon.transforms.SVDLinear`` / ``QRLinear`` and perturbs the
parameters after construction: q-vectors + 0.3 randn, diagonal and triangle parameters randn / sqrt(D), bias randn
(100 randn in ``svd_linear_d64_k64``, so that subtracting the bias before the inverse product matters).

Each file holds: ``sd::`` state_dict entries; ``x`` [257, D]; the reference's float32 forward ``y32`` / ``lad32`` and its
float32 inverse of ``y32`` (``xinv32`` / ``ladinv32``); the same from a float64 deep copy on the same inputs (``lad64``,
``ladinv64``, and the [257, D] outputs as float32 differences ``y64_minus_y32`` / ``xinv64_minus_xinv32``, ``xinv64`` being
the float64 inverse of ``y32``: the float64 value is the float32 array plus the difference, exact to 1e-13, at half the
bytes -- with float64 arrays the D = 130 files exceed the size limit of a committed file); ``gy`` and the float64 gradients
of ``(y * gy).sum() + lad.sum()`` with respect to ``x`` (``grad_x64``, rounded to float32 for storage: 6e-8 relative
against a gradient tolerance of 2e-5 K) and every parameter (``grad64::<name>``, float64); ``floor_fwd`` / ``floor_inv``:
the float32 noise floors max|float32 - float64| over outputs and logabsdet of each direction.
These fixtures are not part of cases.CASES.
"""
import copy
import os

import numpy as np
import torch

from make_golden import HERE, import_reference

ROWS = 257
SVD_CASES = [(5, 2), (64, 64), (130, 6)]
QR_CASES = [(5, 3), (64, 16), (130, 4)]


def perturb(module, kind, features, bias_scale, gen):
    with torch.no_grad():
        for name, p in module.named_parameters():
            if name.endswith("q_vectors"):
                p.add_(0.3 * torch.randn(p.shape, generator=gen))
            elif name == "bias":
                p.copy_(bias_scale * torch.randn(p.shape, generator=gen))
            else:
                p.copy_(torch.randn(p.shape, generator=gen) / features ** 0.5)


def record(L, kind, features, k, gen):
    torch.manual_seed(2000 + features + k)
    cls = L.transforms.SVDLinear if kind == "svd" else L.transforms.QRLinear
    module = cls(features, k)
    perturb(module, kind, features, 100.0 if (kind, features, k) == ("svd", 64, 64) else 1.0, gen)
    module.eval()
    x = torch.randn(ROWS, features, generator=gen)
    gy = torch.randn(ROWS, features, generator=gen)
    out = {"sd::" + name: v.detach().clone().numpy() for name, v in module.state_dict().items()}
    out["x"], out["gy"] = x.numpy(), gy.numpy()
    with torch.no_grad():
        y32, lad32 = module(x.clone())
        xinv32, ladinv32 = module.inverse(y32.clone())
    module64 = copy.deepcopy(module).double()
    x64 = x.double().requires_grad_(True)
    y64, lad64 = module64(x64)
    ((y64 * gy.double()).sum() + lad64.sum()).backward()
    with torch.no_grad():
        xinv64, ladinv64 = module64.inverse(y32.double())
    for t in (y32, lad32, xinv32, ladinv32, y64, lad64, xinv64, ladinv64, x64.grad):
        assert torch.isfinite(t).all()
    out.update(y32=y32.numpy(), lad32=lad32.numpy(), xinv32=xinv32.numpy(), ladinv32=ladinv32.numpy(),
               y64_minus_y32=(y64.detach() - y32.double()).float().numpy(), lad64=lad64.detach().numpy(),
               xinv64_minus_xinv32=(xinv64 - xinv32.double()).float().numpy(), ladinv64=ladinv64.numpy(),
               grad_x64=x64.grad.float().numpy())
    for name, p in module64.named_parameters():
        assert torch.isfinite(p.grad).all()
        out["grad64::" + name] = p.grad.numpy()
    out["floor_fwd"] = np.float64(max((y32.double() - y64.detach()).abs().max().item(),
                                      (lad32.double() - lad64.detach()).abs().max().item()))
    out["floor_inv"] = np.float64(max((xinv32.double() - xinv64).abs().max().item(),
                                      (ladinv32.double() - ladinv64).abs().max().item()))
    path = os.path.join(HERE, "%s_linear_d%d_k%d.npz" % (kind, features, k))
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size <= 1 << 20, path
    print("%s_linear_d%d_k%d floor fwd %.2e inv %.2e | max|y| %.1f max|xinv| %.1f | roundtrip32 %.2e | %d bytes"
          % (kind, features, k, out["floor_fwd"], out["floor_inv"], float(y64.detach().abs().max()), float(xinv64.abs().max()),
             float((xinv32 - x).abs().max()), size))


def main():
    L = import_reference()
    seed = 500
    for kind, cases in (("svd", SVD_CASES), ("qr", QR_CASES)):
        for features, k in cases:
            record(L, kind, features, k, torch.Generator().manual_seed(seed))
            seed += 1


if __name__ == "__main__":
    main()
