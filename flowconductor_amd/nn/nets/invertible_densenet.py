"""Lipschitz-constrained DenseNets, the contractive networks of invertible residual blocks (classes, constructor
arguments, attributes and ``state_dict`` keys of flowcon/nn/nets/invertible_densenet.py).

A net is ``densenet_depth`` ``LipschitzDenseLayer``s -- a spectrally normalised linear layer, the activation, and the
weighted concatenation with the layer's input -- followed by one spectrally normalised linear layer back to
``dimension`` outputs.  All dense layers of a net share ONE activation module (one ``beta`` for ``CLipSwish``).  The
conditional variants feed a context in as extra input channels, as a factor in (-1, 1) on the output, or through a
row-stochastic last layer produced by a hyper-network; none of them changes the Lipschitz bound with respect to x.

Plain torch throughout.  In eval mode ``transforms.iResBlock`` evaluates the unconditional, input-conditional and
multiplicative nets with the kernels of ``csrc/fc_iresblock.hip``."""
import logging
from abc import abstractmethod
from pprint import pformat
from typing import Callable, Tuple, Union

import torch

from flowconductor_amd.nn.nets import activations
from flowconductor_amd.nn.nets.extended_basic_nets import ExtendedLinear, ExtendedSequential
from flowconductor_amd.nn.nets.lipschitz_dense import LipschitzDenseLayer
from flowconductor_amd.nn.nets.mlp import MLP
from flowconductor_amd.nn.nets.spectral_norm import scaled_spectral_norm

ACTIVATION_FNS = {
    'relu': torch.nn.ReLU,
    'tanh': torch.nn.Tanh,
    'elu': torch.nn.ELU,
    'selu': torch.nn.SELU,
    'fullsort': activations.FullSort,
    'maxmin': activations.MaxMin,
    'swish': activations.Swish,
    'LeakyLSwish': activations.LeakyLSwish,
    'CLipSwish': activations.CLipSwish,
    'lcube': activations.LipschitzCube,
    'csin': activations.CSin,
}

logger = logging.getLogger()


def _warn_unused(obj, kwargs):
    if len(kwargs) > 0:
        logger.warning("Unused kwargs for class '{}': \n {}".format(obj.__class__.__name__, pformat(kwargs)))


class _DenseNet(torch.nn.Module):
    def __init__(self,
                 dimension,
                 densenet_depth: int = 2,
                 densenet_growth: int = 16,
                 activation_function: Union[str, Callable] = "CLipSwish",
                 lip_coeff: float = 0.98,
                 n_lipschitz_iters: int = 5):
        super().__init__()
        self.dimension = dimension
        self.densenet_depth = densenet_depth
        self.densenet_growth = densenet_growth
        self.lip_coeff = lip_coeff
        self.n_lipschitz_iters = n_lipschitz_iters

        assert n_lipschitz_iters > 0, "n_lipschitz_iters must be > 0"
        assert lip_coeff > 0, "lip_coeff must be > 0"

        if isinstance(activation_function, str):
            assert activation_function in ACTIVATION_FNS.keys(), f"Activation function {activation_function} not found."
            self.activation = ACTIVATION_FNS[activation_function]()
        else:
            self.activation = activation_function
        self.output_channels = self.calc_output_channels(self.activation, self.densenet_growth)

    def spectral_normalization(self, network):
        return scaled_spectral_norm(network, n_power_iterations=self.n_lipschitz_iters, domain=2, codomain=2,
                                    coeff=self.lip_coeff)

    def build_densenet(self, total_in_channels, densenet_depth, densenet_growth, learnable_concat=True,
                       include_last_layer=True) -> Tuple[ExtendedSequential, int]:
        layers = []
        for _ in range(densenet_depth):
            linear = self.spectral_normalization(torch.nn.Linear(total_in_channels, self.output_channels))
            layers.append(LipschitzDenseLayer(ExtendedSequential(linear, self.activation),
                                              learnable_concat=learnable_concat, lip_coeff=self.lip_coeff))
            total_in_channels += densenet_growth
        if include_last_layer:
            layers.append(self.spectral_normalization(ExtendedLinear(total_in_channels, self.dimension)))
            total_in_channels = 1
        return ExtendedSequential(*layers), total_in_channels

    @staticmethod
    def calc_output_channels(activation, densenet_growth):
        # a concatenating activation doubles the channels, so its linear layer emits half the growth
        if getattr(activation, "_does_concat", False):
            assert densenet_growth % 2 == 0, "Select an even densenet growth size for CLipSwish!"
            return densenet_growth // 2
        return densenet_growth

    @classmethod
    def factory(cls, condition_input=False, condition_lastlayer=False, condition_multiplicative=False, **kwargs):
        table = {
            # (input, last layer, multiplicative)
            (False, False, False): DenseNet,
            (True, False, False): InputConditionalDenseNet,
            (False, True, False): LastLayerConditionalDenseNet,
            (False, False, True): LastLayerConditionalDenseNet,
            (True, True, False): MixedConditionalDenseNet,
            (True, False, True): MultiplicativeAndInputConditionalDenseNet,
        }
        key = (bool(condition_input), bool(condition_lastlayer), bool(condition_multiplicative))
        if key not in table:
            raise NotImplementedError("This combination of conditions for a Lipschitz Network is not implemented .")
        lipschitz_network = table[key]
        return lambda: lipschitz_network(**kwargs)

    @abstractmethod
    def forward(self, x, context=None):
        pass


class DenseNet(_DenseNet):
    """A Lipschitz-continuous network g(x) with Lipschitz constant at most ``lip_coeff``."""

    def __init__(self,
                 dimension,
                 densenet_depth: int = 2,
                 densenet_growth: int = 16,
                 activation_function: Union[str, Callable] = "CLipSwish",
                 lip_coeff: float = 0.98,
                 n_lipschitz_iters: int = 5,
                 **kwargs):
        super().__init__(dimension=dimension, densenet_depth=densenet_depth, densenet_growth=densenet_growth,
                         activation_function=activation_function, lip_coeff=lip_coeff,
                         n_lipschitz_iters=n_lipschitz_iters)
        if len(kwargs) > 0:
            logger.warning("Unused kwargs for {}: {}".format(self.__class__.__name__, pformat(kwargs)))
        self.dense_net, self.densenet_final_layer_dim = self.build_densenet(self.dimension, self.densenet_depth,
                                                                            self.densenet_growth)

    def forward(self, x, context=None):
        assert context is None, "Context not supported for this Class."
        return self.dense_net(x)


class InputConditionalDenseNet(_DenseNet):
    """g(x; c) = h(cat[x, f(c)]): a DenseNet h that is Lipschitz in x, and an embedding f of the context."""

    def __init__(self, dimension, context_features, densenet_depth, densenet_growth=16,
                 c_embed_hidden_sizes=(128, 128, 10), activation_function=activations.Swish, lip_coeff=0.98,
                 n_lipschitz_iters=5, **kwargs):
        super().__init__(dimension=dimension, densenet_depth=densenet_depth, densenet_growth=densenet_growth,
                         activation_function=activation_function, lip_coeff=lip_coeff,
                         n_lipschitz_iters=n_lipschitz_iters)
        _warn_unused(self, kwargs)
        self.context_features = context_features
        self.c_embed_hidden_sizes = c_embed_hidden_sizes

        self.bn = torch.nn.BatchNorm1d(self.context_features)
        self.dense_net, self.densenet_final_layer_dim = self.build_densenet(
            total_in_channels=self.dimension + self.c_embed_hidden_sizes[-1], densenet_growth=densenet_growth,
            densenet_depth=densenet_depth, include_last_layer=True)
        self.context_embedding_net = MLP((self.context_features,), (self.c_embed_hidden_sizes[-1],),
                                         hidden_sizes=self.c_embed_hidden_sizes, activation=torch.nn.SiLU())

    def forward(self, inputs, context=None):
        embedding = self.context_embedding_net(self.bn(context))
        return self.dense_net(torch.cat([inputs, embedding], -1))


class MultiplicativeAndInputConditionalDenseNet(_DenseNet):
    """g(x; c) = phi(c) h(x; c) with phi(c) in (-1, 1) and h an input-conditional DenseNet."""

    def __init__(self, dimension, context_features, densenet_depth, densenet_growth=16,
                 c_embed_hidden_sizes=(128, 128, 10), m_embed_hidden_sizes=(128, 128),
                 activation_function=activations.Swish, lip_coeff=0.98, n_lipschitz_iters=5, **kwargs):
        super().__init__(dimension=dimension, densenet_depth=densenet_depth, densenet_growth=densenet_growth,
                         activation_function=activation_function, lip_coeff=lip_coeff,
                         n_lipschitz_iters=n_lipschitz_iters)
        _warn_unused(self, kwargs)
        self.context_features = context_features
        self.c_embed_hidden_sizes = c_embed_hidden_sizes
        self.m_embed_hidden_sizes = m_embed_hidden_sizes

        self.bn = torch.nn.BatchNorm1d(self.context_features)
        self.dense_net, self.densenet_final_layer_dim = self.build_densenet(
            total_in_channels=self.dimension + self.c_embed_hidden_sizes[-1], densenet_growth=densenet_growth,
            densenet_depth=densenet_depth, include_last_layer=True)
        self.factor_net = MLP((self.context_features,), (1,), hidden_sizes=self.m_embed_hidden_sizes,
                              activation=torch.nn.SiLU())
        self.embedding = MLP((self.context_features,), (self.c_embed_hidden_sizes[-1],),
                             hidden_sizes=self.c_embed_hidden_sizes, activation=torch.nn.SiLU())

    def forward(self, inputs, context=None):
        context = self.bn(context)
        factor = self.factor_net(context)
        embedding = self.embedding(context)
        return torch.nn.functional.tanh(factor) * self.dense_net(torch.cat([inputs, embedding], -1))


class MultiplicativeConditionalDenseNet(_DenseNet):
    """g(x; c) = phi(c) h(x) with phi(c) in (-1, 1) and h an unconditional DenseNet."""

    def __init__(self, dimension, context_features, densenet_depth, densenet_growth=16,
                 c_embed_hidden_sizes=(128, 128, 10), m_embed_hidden_sizes=(128, 128),
                 activation_function=activations.Swish, lip_coeff=0.98, n_lipschitz_iters=5, **kwargs):
        super().__init__(dimension=dimension, densenet_depth=densenet_depth, densenet_growth=densenet_growth,
                         activation_function=activation_function, lip_coeff=lip_coeff,
                         n_lipschitz_iters=n_lipschitz_iters)
        _warn_unused(self, kwargs)
        self.context_features = context_features
        self.c_embed_hidden_sizes = c_embed_hidden_sizes
        self.m_embed_hidden_sizes = m_embed_hidden_sizes

        self.bn = torch.nn.BatchNorm1d(self.context_features)
        # as in the reference, the first layer is sized for an embedding that forward() never appends
        self.dense_net, self.densenet_final_layer_dim = self.build_densenet(
            total_in_channels=self.dimension + self.c_embed_hidden_sizes[-1], densenet_growth=densenet_growth,
            densenet_depth=densenet_depth, include_last_layer=True)
        self.factor_net = MLP((self.context_features,), (1,), hidden_sizes=self.m_embed_hidden_sizes,
                              activation=torch.nn.SiLU())

    def forward(self, inputs, context=None):
        factor = self.factor_net(self.bn(context))
        return torch.nn.functional.tanh(factor) * self.dense_net(inputs)


class LastLayerAttention(torch.nn.Module):
    """The conditional last layer: rows of a softmax-normalised (row-stochastic) matrix produced from the context."""

    def __init__(self, dimension, context_features, value_dim, hidden_sizes=(64, 64), activation=activations.Swish()):
        super().__init__()
        self.dimension = dimension
        self.context_features = context_features
        self.hidden_sizes = hidden_sizes
        self.value_dim = value_dim
        self.activation = activation

        self.bias_net = MLP((self.context_features,), (self.dimension,), hidden_sizes=self.hidden_sizes,
                            activation=self.activation)
        self.weight_network = MLP((self.context_features,), (self.dimension, self.value_dim),
                                  hidden_sizes=self.hidden_sizes, activation=self.activation)

    def attention(self, context, values):
        weights = torch.nn.functional.softmax(self.weight_network(context), dim=-1)
        return torch.bmm(weights, values).squeeze() + self.bias_net(context)


class LastLayerConditionalDenseNet(_DenseNet):
    """A DenseNet whose last layer A(c) comes from a hyper-network, every row passed through a softmax so that the
    Lipschitz constant stays what it was."""

    def __init__(self, dimension, context_features, densenet_depth, densenet_growth=16,
                 last_layer_hidden_sizes=(64, 64), activation_function=activations.Swish, lip_coeff=0.98,
                 n_lipschitz_iters=5, **kwargs):
        super().__init__(dimension=dimension, densenet_depth=densenet_depth, densenet_growth=densenet_growth,
                         activation_function=activation_function, lip_coeff=lip_coeff,
                         n_lipschitz_iters=n_lipschitz_iters)
        _warn_unused(self, kwargs)
        self.context_features = context_features
        self.last_layer_hidden_sizes = last_layer_hidden_sizes

        self.bn = torch.nn.BatchNorm1d(self.context_features)
        self.dense_net, self.densenet_final_layer_dim = self.build_densenet(
            total_in_channels=self.dimension, densenet_growth=densenet_growth, densenet_depth=densenet_depth,
            include_last_layer=False)
        self.custom_attention = LastLayerAttention(dimension=self.dimension, context_features=self.context_features,
                                                   value_dim=self.densenet_final_layer_dim,
                                                   hidden_sizes=self.last_layer_hidden_sizes)

    def forward(self, inputs, context=None):
        context = self.bn(context)
        values = self.dense_net(inputs).unsqueeze(-1)
        return self.custom_attention.attention(context, values)


class MixedConditionalDenseNet(_DenseNet):
    """Input-conditional first layer and hyper-network last layer together."""

    def __init__(self, dimension, context_features, densenet_depth, densenet_growth=16,
                 last_layer_hidden_sizes=(64, 64), c_embed_hidden_sizes=(32, 32, 10),
                 activation_function=activations.Swish, lip_coeff=0.98, n_lipschitz_iters=5, **kwargs):
        super().__init__(dimension=dimension, densenet_depth=densenet_depth, densenet_growth=densenet_growth,
                         activation_function=activation_function, lip_coeff=lip_coeff,
                         n_lipschitz_iters=n_lipschitz_iters)
        _warn_unused(self, kwargs)
        self.context_features = context_features
        self.c_embed_hidden_sizes = c_embed_hidden_sizes
        self.last_layer_hidden_sizes = last_layer_hidden_sizes

        self.output_channels = self.calc_output_channels(self.activation, self.densenet_growth)
        self.bn = torch.nn.BatchNorm1d(self.context_features)
        self.dense_net, self.densenet_final_layer_dim = self.build_densenet(
            total_in_channels=self.dimension + self.c_embed_hidden_sizes[-1], densenet_growth=densenet_growth,
            densenet_depth=densenet_depth, include_last_layer=False)
        self.custom_attention = LastLayerAttention(dimension=self.dimension, context_features=self.context_features,
                                                   value_dim=self.densenet_final_layer_dim,
                                                   hidden_sizes=self.last_layer_hidden_sizes)
        self.context_embedding_net = MLP((self.context_features,), (self.c_embed_hidden_sizes[-1],),
                                         hidden_sizes=self.c_embed_hidden_sizes, activation=torch.nn.SiLU())

    def forward(self, inputs, context=None):
        context = self.bn(context)
        embedding = self.context_embedding_net(context)
        values = self.dense_net(torch.cat([inputs, embedding], -1)).unsqueeze(-1)
        return self.custom_attention.attention(context, values)
