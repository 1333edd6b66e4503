"""Generate tests/golden/mog_<case>.npz (mixture-of-Gaussians MADE densities) by importing the REFERENCE (FlowConductor)
itself.

Runs only where the reference tree exists:
    python tests/golden/make_mog_golden.py
It uses make_golden.py's import.  Every case builds ``flowcon.distributions.MADEMoG`` with ``custom_initialization=True``,
multiplies all parameters by 1.5 and perturbs the residual blocks' (near-)zero-initialised last layers, so that the hidden
stack and the context reach the mixture parameters.

mog_<case>.npz for the cases (D, hidden, C, context, blocks) of ``CASES``: ``sd::`` state_dict entries, ``x`` [257, D] whose
first 8 rows are pushed to +-50 in every column, ``context``, the reference's float32 ``log_prob32``, the same from a
float64 deep copy (``log_prob64``), and the float64 gradient of ``log_prob.sum()`` with respect to ``x`` (``grad_x64``) and
to every parameter (``grad64::<name>``).  ``floor_body`` / ``floor_far`` are the float32 noise floors
max|log_prob32 - log_prob64| over the ordinary rows and over the pushed rows (printed).  The widest case records no
parameter gradients (``grad_x64`` only): with them its file would exceed the size limit of a committed file.
No sampling outputs are recorded: the reference's ``Categorical`` stream cannot be reproduced.
These fixtures are not part of cases.CASES.
"""
import copy
import os

import numpy as np
import torch

from make_golden import HERE, import_reference

ROWS = 257
FAR_ROWS = 8
CASES = [(2, 4, 1, None, 2), (5, 32, 5, 3, 2), (8, 50, 10, 16, 2), (33, 24, 10, 5, 2), (64, 64, 16, 8, 1)]


def case_name(features, hidden, components, context, blocks):
    return "d%d_h%d_c%d_ctx%d_b%d" % (features, hidden, components, context or 0, blocks)


def record(L, case, gen):
    features, hidden, components, context_features, blocks = case
    torch.manual_seed(1000 + features)
    dist = L.distributions.MADEMoG(features, hidden, context_features, num_blocks=blocks,
                                   num_mixture_components=components, custom_initialization=True)
    with torch.no_grad():
        for p in dist.parameters():
            p.mul_(1.5)
        for block in dist._made.blocks:
            last = block.linear_layers[-1]
            last.weight.add_(0.3 / hidden ** 0.5 * torch.randn(last.weight.shape, generator=gen))
            last.bias.add_(0.1 * torch.randn(last.bias.shape, generator=gen))
    dist.eval()
    x = 1.5 * torch.randn(ROWS, features, generator=gen)
    x[:FAR_ROWS] = torch.tensor([50.0, -50.0] * (FAR_ROWS // 2)).reshape(-1, 1)
    context = torch.randn(ROWS, context_features, generator=gen) if context_features else None
    out = {"sd::" + k: v.detach().clone().numpy() for k, v in dist.state_dict().items()}
    out["x"] = x.numpy()
    if context is not None:
        out["context"] = context.numpy()
    with torch.no_grad():
        lp32 = dist.log_prob(x.clone(), context)
    dist64 = copy.deepcopy(dist).double()
    x64 = x.double().requires_grad_(True)
    lp64 = dist64.log_prob(x64, None if context is None else context.double())
    lp64.sum().backward()
    assert torch.isfinite(lp32).all() and torch.isfinite(lp64).all()
    diff = (lp32.double() - lp64.detach()).abs()
    out["log_prob32"], out["log_prob64"] = lp32.numpy(), lp64.detach().numpy()
    out["grad_x64"] = x64.grad.numpy()
    if features * hidden * components < 64 * 64 * 16:
        for name, p in dist64.named_parameters():
            out["grad64::" + name] = p.grad.numpy()
    out["floor_body"] = np.float64(diff[FAR_ROWS:].max().item())
    out["floor_far"] = np.float64(diff[:FAR_ROWS].max().item())
    path = os.path.join(HERE, "mog_%s.npz" % case_name(*case))
    np.savez_compressed(path, **out)
    print("%-24s floor body %.2e far %.2e | log_prob body [%.1f, %.1f] far [%.1f, %.1f] | %d bytes"
          % (case_name(*case), out["floor_body"], out["floor_far"], out["log_prob64"][FAR_ROWS:].min(), out["log_prob64"][FAR_ROWS:].max(),
             out["log_prob64"][:FAR_ROWS].min(), out["log_prob64"][:FAR_ROWS].max(), os.path.getsize(path)))


def main():
    L = import_reference()
    for seed, case in enumerate(CASES):
        record(L, case, torch.Generator().manual_seed(400 + seed))


if __name__ == "__main__":
    main()
