"""Activations of the Lipschitz-constrained DenseNets (classes, attributes and ``state_dict`` keys of
flowcon/nn/nets/activations.py).  Every one of them is 1-Lipschitz, which the bound of an invertible residual block
rests on.  ``_does_concat`` marks the two that double their channel count by acting on ``cat(x, -x)``.

Plain torch: they run on any device and differentiate through autograd.  The eval-mode kernels of
``csrc/fc_iresblock.hip`` evaluate the element-wise ones (and their derivatives) themselves."""
import math

import torch
import torch.nn.functional as F
from torch import nn


class FullSort(nn.Module):
    """Sorts the features of every row (a permutation per row: 1-Lipschitz, gradient-norm preserving)."""

    def forward(self, x):
        return torch.sort(x, 1)[0]


class MaxMin(nn.Module):
    """Max and min of consecutive feature pairs: ``[max of every pair | min of every pair]``."""

    def forward(self, x):
        batch, features = x.shape
        pairs = x.view(batch, features // 2, 2)
        return torch.cat([torch.max(pairs, 2)[0], torch.min(pairs, 2)[0]], 1)


class LipschitzCube(nn.Module):
    """``x^3 / 3`` inside (-1, 1), continued with slope one outside."""

    def forward(self, x):
        upper = (x >= 1).to(x) * (x - 2 / 3)
        lower = (x <= -1).to(x) * (x + 2 / 3)
        middle = ((x > -1) * (x < 1)).to(x) * x ** 3 / 3
        return upper + lower + middle


class Swish(nn.Module):
    """``x sigmoid(softplus(beta) x) / 1.1`` with a learnable ``beta``."""

    def __init__(self):
        super().__init__()
        self.beta = nn.Parameter(torch.tensor([0.5]))

    def forward(self, x):
        return (x * torch.sigmoid_(x * F.softplus(self.beta))).div_(1.1)


class Sin(nn.Module):
    """``sin(w0 x) / w0``."""

    def __init__(self, w0=1):
        super().__init__()
        self.w0 = w0

    def forward(self, x):
        return torch.sin(x * self.w0) / self.w0


class CSin(nn.Module):
    """``sin(w0 cat(x, -x)) / (w0 sqrt 2)``: twice the channels, still 1-Lipschitz."""

    def __init__(self, w0=1):
        super().__init__()
        self.w0 = w0
        self._does_concat = True

    def forward(self, x):
        x = torch.cat((x, -x), 1)
        return torch.sin(x * self.w0) / (self.w0 * math.sqrt(2))


class LeakyLSwish(nn.Module):
    """``a x + (1 - a) swish(x)`` with ``a = sigmoid(alpha)``, ``alpha`` and ``beta`` learnable."""

    def __init__(self):
        super().__init__()
        self.alpha = nn.Parameter(torch.tensor([-3.]))
        self.beta = nn.Parameter(torch.tensor([0.5]))

    def forward(self, x):
        alpha = torch.sigmoid(self.alpha)
        return alpha * x + (1 - alpha) * (x * torch.sigmoid_(x * F.softplus(self.beta))).div_(1.1)


class CLipSwish(nn.Module):
    """``swish(cat(x, -x)) / 1.004``: the default activation of the i-DenseNets."""

    def __init__(self):
        super().__init__()
        self.swish = Swish()
        self._does_concat = True

    def forward(self, x):
        x = torch.cat((x, -x), 1)
        return self.swish(x).div_(1.004)


class LipSwish(nn.Module):
    """``swish(x) / 1.004``."""

    def __init__(self):
        super().__init__()
        self.swish = Swish()

    def forward(self, x):
        return self.swish(x).div_(1.004)
