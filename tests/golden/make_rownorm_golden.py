"""Generate tests/golden/radial_d*.npz, unit_vector_d*.npz and naive_linear_d*.npz by importing the REFERENCE (FlowConductor)
itself.

Runs only where the reference tree exists:
    python tests/golden/make_rownorm_golden.py
It uses make_golden.py's import.  Cases (257 rows each):
  radial_d{1,2,5,64,130}          ``flowcon.transforms.RadialTransform(D)``, alpha / beta / z_0 perturbed after construction
                                  (alpha += 0.5 randn, beta += 0.5 randn, z_0 = randn), row ``edge_row`` of x set exactly to z_0
  unit_vector_d{1,2,3,20,63,130}  ``UnitVector(d)``, inputs randn scaled by min(1, sqrt(10 / d)) so that 1 - y_last >= 0.05 on
                                  every row (asserted)
  naive_linear_d{1,5,64,130}      ``NaiveLinear(D)``: the orthogonal init plus 0.3 randn / sqrt(D), bias randn (100 randn at
                                  D = 64, so that subtracting the bias before the inverse product matters)

Each file holds: ``sd::`` state_dict entries; ``x``; ``gy``; the reference's float32 forward ``y32`` / ``lad32`` and, where the
reference has an inverse (not for radial), its float32 inverse of ``y32`` (``xinv32`` / ``ladinv32``); the same from a float64
deep copy on the same inputs (``lad64`` / ``ladinv64`` and the [257, D] outputs as float32 differences ``y64_minus_y32`` /
``xinv64_minus_xinv32``: the float64 value is the float32 array plus the difference, exact to 1e-13, at half the bytes, so
that every file stays under the size limit of a committed file); the float64 gradients of ``(y * gy).sum() + lad.sum()``
with respect to ``x`` (``grad_x64``, rounded to float32 for storage) and every parameter that has one (``grad64::<name>``;
[D, D] ones rounded to float32 too) -- for radial the sum leaves out row ``edge_row``, where the reference's autograd
yields NaN through the norm's gradient; for unit_vector also ``grad_y64``: the gradient of
``(x * gy[:, :d]).sum() + lad.sum()`` of the inverse direction with respect to its float64 input ``y32``;
``floor_fwd_y`` / ``floor_fwd_lad`` / ``floor_inv_x`` / ``floor_inv_lad``: the float32 noise floors max|float32 - float64|.
These fixtures are not part of cases.CASES.
"""
import copy
import os

import numpy as np
import torch

from make_golden import HERE, import_reference

ROWS = 257
EDGE_ROW = 3
RADIAL = [1, 2, 5, 64, 130]
UNIT = [1, 2, 3, 20, 63, 130]
NAIVE = [1, 5, 64, 130]


def build(L, kind, d, gen):
    torch.manual_seed(3000 + d)
    if kind == "radial":
        module = L.transforms.RadialTransform(d)
        with torch.no_grad():
            module.alpha.add_(0.5 * torch.randn(1, generator=gen))
            module.beta.add_(0.5 * torch.randn(1, generator=gen))
            module.z_0.copy_(torch.randn(1, d, generator=gen))
        x = torch.randn(ROWS, d, generator=gen) * 1.5
        x[EDGE_ROW] = module.z_0.detach()[0]
        width = d
    elif kind == "unit_vector":
        module = L.transforms.UnitVector(d)
        x = torch.randn(ROWS, d, generator=gen) * min(1.0, (10.0 / d) ** 0.5)
        width = d + 1
    else:
        module = L.transforms.NaiveLinear(d)
        with torch.no_grad():
            module._weight.add_(0.3 * torch.randn(d, d, generator=gen) / d ** 0.5)
            module.bias.copy_((100.0 if d == 64 else 1.0) * torch.randn(d, generator=gen))
        x = torch.randn(ROWS, d, generator=gen)
        width = d
    return module.eval(), x, torch.randn(ROWS, width, generator=gen)


def record(L, kind, d, gen):
    module, x, gy = build(L, kind, d, gen)
    has_inverse = kind != "radial"
    out = {"sd::" + name: v.detach().clone().numpy() for name, v in module.state_dict().items()}
    out["x"], out["gy"] = x.numpy(), gy.numpy()
    with torch.no_grad():
        y32, lad32 = module(x.clone())
        if has_inverse:
            xinv32, ladinv32 = module.inverse(y32.clone())
    module64 = copy.deepcopy(module).double()
    x64 = x.double().requires_grad_(True)
    y64, lad64 = module64(x64)
    if kind == "radial":
        out["edge_row"] = np.int64(EDGE_ROW)
        # a mask would still poison the sums through 0 * NaN: differentiate the other rows only
        rows = torch.arange(ROWS) != EDGE_ROW
        x_rest = x.double()[rows].requires_grad_(True)
        y_rest, lad_rest = module64(x_rest)
        ((y_rest * gy.double()[rows]).sum() + lad_rest.sum()).backward()
        grad_x = torch.zeros(ROWS, d, dtype=torch.float64)
        grad_x[rows] = x_rest.grad
    else:
        ((y64 * gy.double()).sum() + lad64.sum()).backward()
        grad_x = x64.grad
    finite = [y32, lad32, y64, lad64, grad_x]
    out.update(y32=y32.numpy(), lad32=lad32.numpy(), y64_minus_y32=(y64.detach() - y32.double()).float().numpy(),
               lad64=lad64.detach().numpy(), grad_x64=grad_x.float().numpy())
    out["floor_fwd_y"] = np.float64((y32.double() - y64.detach()).abs().max().item())
    out["floor_fwd_lad"] = np.float64((lad32.double() - lad64.detach()).abs().max().item())
    for name, p in module64.named_parameters():
        if p.grad is None:
            assert kind == "unit_vector" and name == "dim_sphere"
            continue
        finite.append(p.grad)
        out["grad64::" + name] = p.grad.float().numpy() if p.grad.dim() == 2 and p.grad.shape[0] > 1 else p.grad.numpy()
    if has_inverse:
        yin = y32.double().requires_grad_(kind == "unit_vector")
        xinv64, ladinv64 = module64.inverse(yin)
        if kind == "unit_vector":
            assert float((1 - y64.detach()[:, -1]).min()) >= 0.05
            ((xinv64 * gy.double()[:, :d]).sum() + ladinv64.sum()).backward()
            out["grad_y64"] = yin.grad.float().numpy()
            finite.append(yin.grad)
        xinv64, ladinv64 = xinv64.detach(), ladinv64.detach()
        finite += [xinv32, ladinv32, xinv64, ladinv64]
        out.update(xinv32=xinv32.numpy(), ladinv32=ladinv32.numpy(), ladinv64=ladinv64.numpy(),
                   xinv64_minus_xinv32=(xinv64 - xinv32.double()).float().numpy())
        out["floor_inv_x"] = np.float64((xinv32.double() - xinv64).abs().max().item())
        out["floor_inv_lad"] = np.float64((ladinv32.double() - ladinv64).abs().max().item())
    for t in finite:
        assert torch.isfinite(t).all()
    path = os.path.join(HERE, "%s_d%d.npz" % (kind, d))
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size <= 1 << 20, path
    print("%s_d%d floors fwd y %.2e lad %.2e%s | max|y| %.1f | %d bytes"
          % (kind, d, out["floor_fwd_y"], out["floor_fwd_lad"],
             " inv x %.2e lad %.2e" % (out["floor_inv_x"], out["floor_inv_lad"]) if has_inverse else "",
             float(y64.detach().abs().max()), size))


def main():
    L = import_reference()
    seed = 700
    for kind, dims in (("radial", RADIAL), ("unit_vector", UNIT), ("naive_linear", NAIVE)):
        for d in dims:
            record(L, kind, d, torch.Generator().manual_seed(seed))
            seed += 1


if __name__ == "__main__":
    main()
