"""Shared by tests/test_umnn_training_host.py and tests/test_gpu_umnn_training.py: gradients of the UMNN modules through
autograd, and the implicit-function yardstick of the inverse direction built from the forward map."""
import torch


def _leaf(t):
    return None if t is None else t.detach().clone().requires_grad_(True)


def _named(module, x, ctx, grads):
    names = ["inputs"] + (["context"] if ctx is not None else []) + [n for n, _ in module.named_parameters()]
    assert len(names) == len(grads)
    like = [x] + ([ctx] if ctx is not None else []) + [p for _, p in module.named_parameters()]
    return {n: (torch.zeros_like(t) if g is None else g.detach()) for n, g, t in zip(names, grads, like)}


def autograd_grads(module, inputs, ctx, g_out, g_lad, inverse=False, create_graph=False):
    """``(outputs, logabsdet, {name: gradient})`` of the loss (out g_out).sum() + (lad g_lad).sum() of ``module(inputs,
    ctx)`` (``inverse``: ``module.inverse``) with respect to the inputs, the context and every parameter."""
    x, c = _leaf(inputs), _leaf(ctx)
    out, lad = (module.inverse if inverse else module)(x, c)
    loss = (out * g_out).sum() + (lad * g_lad).sum()
    wrt = [x] + ([c] if c is not None else []) + list(module.parameters())
    grads = torch.autograd.grad(loss, wrt, allow_unused=True, create_graph=create_graph)
    return out.detach(), lad.detach(), _named(module, x, c, grads)


def implicit_inverse_grads(module, targets, ctx, g_out, g_lad):
    """The same gradients for ``module.inverse`` by the implicit-function theorem, from the FORWARD map G of the module
    (the torch composition) at the root x the ``no_grad`` inverse returns:  G(x; ctx, theta) = y, lad_inv = -lad(x), so with
    u = g_out - d(lad g_lad)/dx and J = dG/dx per row,  g_y = J^-T u  and every other gradient is that of
    -(lad g_lad).sum() - (G v).sum() with v = g_y held constant."""
    with torch.no_grad():
        root, lad_inv = module.inverse(targets, ctx)
    x, c = _leaf(root), _leaf(ctx)
    image, lad = module(x, c)
    direct = -(lad * g_lad).sum()
    u = g_out + torch.autograd.grad(direct, x, retain_graph=True)[0]
    d = x.shape[1]
    jac = torch.stack([torch.autograd.grad(image[:, i].sum(), x, retain_graph=True)[0] for i in range(d)], dim=1)
    v = torch.linalg.solve(jac.transpose(1, 2).cpu(), u.unsqueeze(-1).cpu()).squeeze(-1).to(u.device)    # [rows] D x D systems
    wrt = ([c] if c is not None else []) + list(module.parameters())
    rest = torch.autograd.grad(direct - (image * v).sum(), wrt, allow_unused=True)
    return root, lad_inv, _named(module, x, c, [v] + list(rest))
