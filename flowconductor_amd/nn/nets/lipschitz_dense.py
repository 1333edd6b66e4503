"""One layer of a Lipschitz DenseNet (``LipschitzDenseLayer`` of flowcon/nn/nets/lipschitz_dense.py): the input and the
layer's output are concatenated with weights ``eta1``, ``eta2`` on a circle of radius ``lip_coeff``, so that the
concatenation of a 1-Lipschitz identity and a 1-Lipschitz layer is ``lip_coeff``-Lipschitz."""
import torch
import torch.nn.functional as F
from torch import nn


class LipschitzDenseLayer(nn.Module):
    def __init__(self, network, learnable_concat=False, lip_coeff=0.98):
        super().__init__()
        self.network = network
        self.lip_coeff = lip_coeff
        if learnable_concat:
            self.K1_unnormalized = nn.Parameter(torch.tensor([1.]))
            self.K2_unnormalized = nn.Parameter(torch.tensor([1.]))
        else:
            self.register_buffer("K1_unnormalized", torch.tensor([1.]))
            self.register_buffer("K2_unnormalized", torch.tensor([1.]))

    def get_eta1_eta2(self, beta=0.1):
        eta1 = F.softplus(self.K1_unnormalized) + beta
        eta2 = F.softplus(self.K2_unnormalized) + beta
        norm = torch.sqrt(eta1 ** 2 + eta2 ** 2)
        return (eta1 / norm) * self.lip_coeff, (eta2 / norm) * self.lip_coeff

    def forward(self, x):
        out = self.network(x)
        eta1, eta2 = self.get_eta1_eta2()
        return torch.cat([x * eta1, out * eta2], dim=1)
