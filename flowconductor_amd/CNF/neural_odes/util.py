"""Divergence estimators and noise samplers of the ODE function."""
import torch
from torch import nn


def divergence_bf(dx, y, create_graph=True, **unused_kwargs):
    """Exact divergence ``sum_i d dx_i / d y_i`` of ``[N, D]`` rows: one backward pass per dimension.  ``create_graph``
    keeps the result differentiable (the default, as training needs it)."""
    total = 0.0
    last = y.shape[1] - 1
    for i in range(y.shape[1]):
        grad = torch.autograd.grad(dx[:, i].sum(), y, create_graph=create_graph,
                                   retain_graph=create_graph or i < last)[0]
        total = total + grad[:, i]
    return total.contiguous()


def divergence_approx(f, y, e=None):
    """Hutchinson's estimate ``e^T (df/dy) e`` from one vector-Jacobian product."""
    e_jac = torch.autograd.grad(f, y, e, create_graph=True)[0]
    return (e_jac * e).reshape(y.shape[0], -1).sum(dim=1)


def sample_rademacher_like(y):
    """+-1 with equal probability, drawn on the device of ``y``."""
    return torch.randint(0, 2, y.shape, device=y.device).to(y) * 2 - 1


def sample_gaussian_like(y):
    return torch.randn_like(y)


def _get_minibatch_jacobian(y, x, create_graph=True):
    """``[N, D_y, D_x]`` Jacobian of per-row outputs with respect to per-row inputs, row of the Jacobian by row."""
    assert y.shape[0] == x.shape[0]
    y = y.reshape(y.shape[0], -1)
    rows = [torch.autograd.grad(y[:, j], x, torch.ones_like(y[:, j]), retain_graph=True,
                                create_graph=create_graph)[0].reshape(x.shape[0], -1) for j in range(y.shape[1])]
    return torch.stack(rows, dim=1)


class Lambda(nn.Module):
    def __init__(self, f):
        super().__init__()
        self.f = f

    def forward(self, x):
        return self.f(x)
