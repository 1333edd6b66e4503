"""The time-conditioned linear layers.  With ``h = W x + b`` from ``_layer``:

    IgnoreLinear         h
    ConcatLinear         W [t | x] + b                      (t is the first input column of ``_layer``)
    ConcatLinear_v2      h + w_b t
    SquashLinear         h sigmoid(w_g t + b_g)
    ConcatSquashLinear   h sigmoid(w_g t + b_g) + w_b t
    HyperLinear          W(t) x + b(t), both from a small net of t
    BlendLinear          (1 - t) h_0 + t h_1

The first five are one form, ``(W x + b + w_t t) gate + w_b t``, which is what the HIP kernels evaluate
(csrc/fc_cnf.hip); the weights of the last two depend on t."""
import torch
import torch.nn.functional as F
from torch import nn

__all__ = ["IgnoreLinear", "ConcatLinear", "ConcatLinear_v2", "SquashLinear", "ConcatSquashLinear", "HyperLinear",
           "BlendLinear", "weights_init"]


def weights_init(m):
    name = m.__class__.__name__
    if "Linear" in name or "Conv" in name:
        nn.init.constant_(m.weight, 0)
        nn.init.normal_(m.bias, 0, 0.01)


class HyperLinear(nn.Module):
    def __init__(self, dim_in, dim_out, hypernet_dim=8, n_hidden=1, activation=nn.Tanh):
        super().__init__()
        self.dim_in = dim_in
        self.dim_out = dim_out
        self.params_dim = dim_in * dim_out + dim_out
        dims = [1] + [hypernet_dim] * n_hidden + [self.params_dim]
        layers = []
        for i in range(1, len(dims)):
            layers.append(nn.Linear(dims[i - 1], dims[i]))
            if i < len(dims) - 1:
                layers.append(activation())
        self._hypernet = nn.Sequential(*layers)
        self._hypernet.apply(weights_init)

    def forward(self, t, x):
        params = self._hypernet(t.view(1, 1)).view(-1)
        bias = params[:self.dim_out]
        weight = params[self.dim_out:].view(self.dim_out, self.dim_in)
        return F.linear(x, weight, bias)


class IgnoreLinear(nn.Module):
    def __init__(self, dim_in, dim_out):
        super().__init__()
        self._layer = nn.Linear(dim_in, dim_out)

    def forward(self, t, x):
        return self._layer(x)


class ConcatLinear(nn.Module):
    def __init__(self, dim_in, dim_out):
        super().__init__()
        self._layer = nn.Linear(dim_in + 1, dim_out)

    def forward(self, t, x):
        return self._layer(torch.cat([torch.ones_like(x[:, :1]) * t, x], dim=1))


class ConcatLinear_v2(nn.Module):
    def __init__(self, dim_in, dim_out):
        super().__init__()
        self._layer = nn.Linear(dim_in, dim_out)
        self._hyper_bias = nn.Linear(1, dim_out, bias=False)

    def forward(self, t, x):
        return self._layer(x) + self._hyper_bias(t.view(-1, 1))


class SquashLinear(nn.Module):
    def __init__(self, dim_in, dim_out):
        super().__init__()
        self._layer = nn.Linear(dim_in, dim_out)
        self._hyper = nn.Linear(1, dim_out)

    def forward(self, t, x):
        return self._layer(x) * torch.sigmoid(self._hyper(t.view(-1, 1)))


class ConcatSquashLinear(nn.Module):
    def __init__(self, dim_in, dim_out):
        super().__init__()
        self._layer = nn.Linear(dim_in, dim_out)
        self._hyper_bias = nn.Linear(1, dim_out, bias=False)
        self._hyper_gate = nn.Linear(1, dim_out)

    def forward(self, t, x):
        gate = torch.sigmoid(self._hyper_gate(t.view(-1, 1)))
        return self._layer(x) * gate + self._hyper_bias(t.view(-1, 1))


class BlendLinear(nn.Module):
    def __init__(self, dim_in, dim_out, layer_type=nn.Linear, **unused_kwargs):
        super().__init__()
        self._layer0 = layer_type(dim_in, dim_out)
        self._layer1 = layer_type(dim_in, dim_out)

    def forward(self, t, x):
        y0 = self._layer0(x)
        return y0 + (self._layer1(x) - y0) * t
