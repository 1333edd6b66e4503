"""FFJORD regularisers: extra ODE states that integrate a penalty on the dynamics along the trajectory."""
import torch
from torch import nn

from flowconductor_amd import options

from ..util import _get_minibatch_jacobian


class RegularizedODEfunc(nn.Module):
    """Appends one state derivative per regularisation function to what ``odefunc`` returns (when the solver carries
    such states: in training mode)."""

    def __init__(self, odefunc, regularization_fns):
        super().__init__()
        self.odefunc = odefunc
        self.regularization_fns = regularization_fns

    def before_odeint(self, *args, **kwargs):
        self.odefunc.before_odeint(*args, **kwargs)

    def forward(self, t, state):
        if len(state) <= 2:
            return self.odefunc(t, tuple(state[:2]))

        class SharedContext:        # the Jacobian, computed once for the functions that share it
            pass

        # the regularisers differentiate dx again: the once-differentiable training kernels step aside
        with torch.enable_grad(), options.override(cnf_training=False):
            x, logp = state[:2]
            if not x.requires_grad:
                x = x.detach().requires_grad_(True)
            dstate = tuple(self.odefunc(t, (x, logp)))
            dx, dlogp = dstate[:2]
            return dstate + tuple(fn(x, logp, dx, dlogp, SharedContext) for fn in self.regularization_fns)

    @property
    def _num_evals(self):
        return self.odefunc._num_evals


def _batch_root_mean_squared(tensor):
    tensor = tensor.reshape(tensor.shape[0], -1)
    return torch.mean(torch.norm(tensor, p=2, dim=1) / tensor.shape[1] ** 0.5)


def _jacobian(x, dx, context):
    if not hasattr(context, "jac"):
        context.jac = _get_minibatch_jacobian(dx, x)
    return context.jac


def l1_regularzation_fn(x, logp, dx, dlogp, unused_context):
    return torch.mean(torch.abs(dx))


def l2_regularzation_fn(x, logp, dx, dlogp, unused_context):
    return _batch_root_mean_squared(dx)


def directional_l2_regularization_fn(x, logp, dx, dlogp, unused_context):
    return _batch_root_mean_squared(torch.autograd.grad(dx, x, dx, create_graph=True)[0])


def jacobian_frobenius_regularization_fn(x, logp, dx, dlogp, context):
    return _batch_root_mean_squared(_jacobian(x, dx, context))


def jacobian_diag_frobenius_regularization_fn(x, logp, dx, dlogp, context):
    return _batch_root_mean_squared(torch.diagonal(_jacobian(x, dx, context), dim1=1, dim2=2))


def jacobian_offdiag_frobenius_regularization_fn(x, logp, dx, dlogp, context):
    jac = _jacobian(x, dx, context)
    diagonal = torch.diagonal(jac, dim1=1, dim2=2)
    off = jac.reshape(jac.shape[0], -1).square().sum(dim=1) - diagonal.square().sum(dim=1)
    return torch.mean(off / (diagonal.shape[1] * (diagonal.shape[1] - 1)))
