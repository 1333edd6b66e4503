"""``nn.Sequential`` / ``nn.Linear`` under the names the DenseNets of flowcon/nn/nets/extended_basic_nets.py are built
from, with their two helpers: ``build_clone`` (a detached copy) and ``build_jvp_net`` (the same layer without bias,
for pushing tangents through)."""
import torch
from torch import nn


class ExtendedSequential(nn.Sequential):
    def build_clone(self):
        return ExtendedSequential(*[m.build_clone() for m in self])

    def build_jvp_net(self, *args):
        with torch.no_grad():
            nets, y = [], args
            for m in self:
                jvp_net, *y = m.build_jvp_net(*y)
                nets.append(jvp_net)
            return (ExtendedSequential(*nets), *y)


class ExtendedLinear(nn.Linear):
    def _detached(self, with_bias):
        with torch.no_grad():
            with_bias = with_bias and self.bias is not None
            m = nn.Linear(self.in_features, self.out_features, bias=with_bias, device=self.weight.device)
            m.weight.data.copy_(self.weight.detach())
            if with_bias:
                m.bias.data.copy_(self.bias.detach())
            return m

    def build_clone(self):
        return self._detached(with_bias=True)

    def build_jvp_net(self, x):
        """The tangent map of a linear layer has no bias."""
        with torch.no_grad():
            return self._detached(with_bias=False), self.forward(x).detach().clone()
