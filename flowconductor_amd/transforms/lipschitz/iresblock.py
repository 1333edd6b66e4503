"""``iResBlock``: the invertible residual block ``y = x + g(x)`` over a Lipschitz-constrained network ``g`` (classes,
constructor arguments and ``state_dict`` keys of flowcon/transforms/lipschitz/iresblock.py).

Two routes:

* the torch composition, as in the reference: in training mode a stochastic power-series estimate of
  ``log det(I + dg/dx)`` (or the exact determinant with ``brute_force=True``), in eval mode always the exact one from
  ``dimension`` backward passes; the inverse is the fixed-point iteration ``x <- y - g(x)`` with the reference's
  batch-wide stopping test.  It runs on any device and dtype and differentiates;
* in eval mode, without gradients, for float32 ``[N, D]`` rows on a HIP device and a net within the kernels' limits
  (D <= 16, depth <= 4, total width <= 128, an element-wise or CLipSwish / CSin activation; ``DenseNet``,
  ``InputConditionalDenseNet``, ``MultiplicativeAndInputConditionalDenseNet``): ``fc_iresnet_forward`` computes value,
  exact forward-mode Jacobian and its LU in one launch, and ``fc_iresnet_inverse`` iterates every row to its own
  convergence in one launch without a host sync.  The per-row stopping test is ``|x - x_prev| <= atol + rtol |y|``
  ("Invertible residual blocks").

By default ``train()`` mode never takes the kernels, whatever ``brute_force`` says, and neither does a call that needs a
gradient.  With ``options.override(iresblock_training=True)`` a ``forward`` call that needs a gradient and would compute
the EXACT determinant -- ``train()`` mode with ``brute_force=True``, eval mode with autograd on -- is one autograd node:
``fc_iresnet_forward`` on an image that torch builds differentiably from the live modules (so the gradient of the image
flows on into the spectral normalisation, the concatenation weights and the activation scalars, and a training-mode
call advances the power iteration exactly as one composition call does), and ``fc_iresnet_backward``, which recomputes
the streams and sweeps them in reverse.  The node is once differentiable (``ops.IRES_DOUBLE_BACKWARD_MSG``).  The
power-series estimators (their law is stochastic), ``inverse`` with gradients, float64 modules, hooks, a ``bn`` in
training mode and every net outside the kernels' limits stay on the composition ("iResBlock training")."""
import abc
import contextlib
import copy
import logging
from typing import Tuple

import torch

from flowconductor_amd import ops, options as fc_options
from flowconductor_amd.nn.nets import activations
from flowconductor_amd.nn.nets.invertible_densenet import (
    DenseNet,
    InputConditionalDenseNet,
    MultiplicativeAndInputConditionalDenseNet,
    _DenseNet,
)
from flowconductor_amd.nn.nets.lipschitz_dense import LipschitzDenseLayer
from flowconductor_amd.transforms.base import Transform, own_autograd_check
from flowconductor_amd.transforms.lipschitz.util import (
    BiasedParameterGenerator,
    ParameterGenerator,
    UnbiasedParameterGenerator,
)
from flowconductor_amd.utils.torchutils import batch_jacobian, logabsdet

logger = logging.getLogger()

__all__ = ['iResBlock']


def _kernel_activation(act):
    """``(kernel activation id, p0, p1)`` with p0 / p1 as zero-argument callables returning tensors or floats, or None
    for an activation the kernels do not evaluate (exact types only: a subclass may compute anything)."""
    kind = type(act)
    if kind is torch.nn.ReLU:
        return ops.IRES_ACT_RELU, None, None
    if kind is torch.nn.Tanh:
        return ops.IRES_ACT_TANH, None, None
    if kind is torch.nn.ELU:
        return ops.IRES_ACT_ELU, (lambda: float(act.alpha)), None
    if kind is activations.Swish:
        return ops.IRES_ACT_SWISH, (lambda: torch.nn.functional.softplus(act.beta)), None
    if kind is activations.LipSwish:
        return ops.IRES_ACT_LIPSWISH, (lambda: torch.nn.functional.softplus(act.swish.beta)), None
    if kind is activations.CLipSwish:
        return ops.IRES_ACT_CLIPSWISH, (lambda: torch.nn.functional.softplus(act.swish.beta)), None
    if kind is activations.Sin and act.w0 != 0:
        return ops.IRES_ACT_SIN, (lambda: float(act.w0)), None
    if kind is activations.CSin and act.w0 != 0:
        return ops.IRES_ACT_CSIN, (lambda: float(act.w0)), None
    if kind is activations.LeakyLSwish:
        return (ops.IRES_ACT_LEAKY_LSWISH, (lambda: torch.nn.functional.softplus(act.beta)),
                (lambda: torch.sigmoid(act.alpha)))
    return None


class iResBlock(Transform):
    """Invertible residual block over a network with Lipschitz constant below one.  ``brute_force`` selects the exact
    log-determinant in training mode too; otherwise ``unbiased_estimator`` chooses between the Russian-roulette and the
    truncated power series, ``options['trace_estimator']`` between ``'neumann'`` and ``'basic'``.  Eval mode is always
    exact."""

    _HIP_AUTOGRAD = True    # with autograd on: the differentiable torch composition, or the node of ops.iresnet_autograd

    _backward_blocks = 0    # tests: a cap on fc_iresnet_backward's grid below the kernel's own (0: the kernel's)

    def __init__(self, contractive_network: _DenseNet, brute_force=False, unbiased_estimator=True, **options):
        super().__init__()
        self.nnet = contractive_network
        self.brute_force = brute_force
        self.unbiased_estimator = unbiased_estimator

        self.train_determinant_estimator = DeterminantEstimator.build(
            network=self.nnet, brute_force=self.brute_force, unbiased_power_series=unbiased_estimator, **options)
        self.test_time_determinant_estimator = DeterminantEstimator.build(network=self.nnet, brute_force=True,
                                                                          **options)

    # ---- the torch composition ------------------------------------------------------------------------------------

    @property
    def logabsdet_estimator(self):
        return self.train_determinant_estimator if self.training else self.test_time_determinant_estimator

    def _inverse_fixed_point(self, y, context=None, atol=1e-5, rtol=1e-5):
        """Picard iteration ``x <- y - g(x)`` from ``x = y``, with the reference's stopping rule: the SQUARED step of
        every element of the batch is below ``atol + rtol |y|``; at most 1001 further evaluations."""
        tol = atol + rtol * y.abs()
        previous, current = y, y - self.nnet(y, context)
        for _ in range(1001):
            if bool(((current - previous).square() < tol).all()):
                return current
            previous, current = current, y - self.nnet(current, context)
        logger.info('Iterations exceeded 1000 for inverse.')
        return current

    def _g_and_logabsdet(self, x, context=None):
        """g(x) and log|det d(x + g(x))/dx| from the estimator of the current mode."""
        keep_graph = torch.is_grad_enabled()
        with torch.enable_grad():
            g, lad = self.logabsdet_estimator.logabsdet_and_g(x, training=self.training, context=context)
        if not keep_graph:
            g, lad = g.detach(), lad.detach()
        return g, lad

    # ---- the kernels ----------------------------------------------------------------------------------------------

    def _kernel_plan(self):
        """What is fixed by how the net is built: ``(activation id, p0, p1, e, multiplicative)`` or None."""
        net = self.nnet
        kind = type(net)
        if kind is DenseNet:
            e, multiplicative = 0, False
        elif kind is InputConditionalDenseNet:
            e, multiplicative = int(net.c_embed_hidden_sizes[-1]), False
        elif kind is MultiplicativeAndInputConditionalDenseNet:
            e, multiplicative = int(net.c_embed_hidden_sizes[-1]), True
        else:
            return None
        act = _kernel_activation(net.activation)
        if act is None or not ops.iresnet_supported(net.dimension, e, net.densenet_depth, net.densenet_growth, act[0]):
            return None
        layers = list(net.dense_net)
        if len(layers) != net.densenet_depth + 1 or not isinstance(layers[-1], torch.nn.Linear):
            return None
        w_in = net.dimension + e
        for layer in layers[:-1]:
            if not (isinstance(layer, LipschitzDenseLayer) and len(layer.network) == 2
                    and isinstance(layer.network[0], torch.nn.Linear) and layer.network[1] is net.activation
                    and layer.network[0].in_features == w_in and layer.network[0].out_features == net.output_channels
                    and layer.network[0].bias is not None):
                return None
            w_in += net.densenet_growth
        if layers[-1].in_features != w_in or layers[-1].out_features != net.dimension or layers[-1].bias is None:
            return None
        return act + (e, multiplicative)

    def _use_kernels(self, inputs, context):
        if self.training or self.nnet.training or not isinstance(inputs, torch.Tensor):
            return None
        if torch.is_grad_enabled() and self._needs_gradient(inputs, context):
            return None
        # a sub-module in training mode (net.bn.train()) means the composition
        if any(m.training for m in ops.module_list(self.nnet)):
            return None
        return self._plan_for(inputs, context)

    def _needs_gradient(self, inputs, context):
        return (inputs.requires_grad or (context is not None and context.requires_grad)
                or any(p.requires_grad for p in ops.param_list(self)))

    def _plan_for(self, inputs, context):
        """The kernel plan if rows, context, parameters and net are what the kernels take (whatever the mode), or None."""
        if not (inputs.is_cuda and inputs.dtype == torch.float32 and inputs.dim() == 2
                and inputs.shape[1] == self.nnet.dimension and inputs.shape[0] > 0):
            return None
        params = ops.param_list(self)
        if any(p.dtype != torch.float32 or p.device != inputs.device for p in params) or ops.has_hooks(self.nnet):
            return None
        plan = ops.static_memo(self, "static_ok", (id(self.nnet), id(self.nnet.activation)), self._kernel_plan)
        if plan is None:
            return None
        if (plan[3] > 0 or plan[4]) != (context is not None):
            return None     # the composition raises what the reference raises
        if context is not None and not (context.is_cuda and context.dtype == torch.float32 and context.dim() == 2
                                        and context.shape[0] == inputs.shape[0]):
            return None
        return plan

    def _use_training_kernels(self, inputs, context):
        """The plan for the one-node training route (options ``iresblock_training``): a call that needs a gradient and
        whose estimator is the exact one."""
        if not fc_options.get("iresblock_training") or not isinstance(inputs, torch.Tensor):
            return None
        if type(self.logabsdet_estimator) is not BruteForceDeterminantEstimator:
            return None     # a power-series estimate is a random variable whose law must stay what it is
        if not torch.is_grad_enabled() or not self._needs_gradient(inputs, context):
            return None
        bn = getattr(self.nnet, "bn", None)
        if bn is not None and bn.training:
            return None     # batch statistics of the context: the composition's business
        return self._plan_for(inputs, context)

    def _image_constants(self):
        """The plain Python numbers that end up in the image (they have no version counter to watch)."""
        net = self.nnet
        act = net.activation
        layers = net.dense_net
        return (getattr(act, "w0", None), getattr(act, "alpha", None) if isinstance(act, torch.nn.ELU) else None,
                net.lip_coeff) + tuple(layer.lip_coeff for layer in layers[:-1]) + tuple(
            (layer.network[0] if i < len(layers) - 1 else layer).parametrizations.weight[0].coeff
            for i, layer in enumerate(layers))

    def _image(self, plan):
        """The packed, normalised net on the device, once per parameter version (no host sync)."""
        net = self.nnet
        key = ops.cache_key(*ops.param_list(self), *ops.buffer_list(net), extra=self._image_constants())
        return ops.memo(self, "ires_image", key, lambda: self._pack_image(plan))

    def _pack_image(self, plan):
        net = self.nnet
        act_id = plan[0]
        with torch.no_grad():
            # the constants of the eval-mode net (normalised weights, eta1 / eta2, activation scalars) are evaluated by
            # the modules' own code on a float64 copy and rounded to float32 once
            dense64 = copy.deepcopy(net.dense_net).double()
            device = dense64[-1].bias.device
            _, p0, p1 = _kernel_activation(dense64[0].network[1])

            def scalar(fn):
                if fn is None:
                    return torch.zeros(1, dtype=torch.float64, device=device)
                value = fn()
                if isinstance(value, torch.Tensor):
                    return value.reshape(1).double()
                return torch.full((1,), value, dtype=torch.float64, device=device)

            def padded(linear):
                weight, bias = linear.weight, linear.bias     # eval mode: W / max(1, sigma / coeff) from the stored u, v
                out = ops._pad4(weight.shape[0])
                wt = torch.zeros(weight.shape[1], out, dtype=torch.float64, device=device)
                wt[:, :weight.shape[0]] = weight.t()
                b = torch.zeros(out, dtype=torch.float64, device=device)
                b[:weight.shape[0]] = bias
                return [b, wt.reshape(-1)]

            zeros2 = torch.zeros(2, dtype=torch.float64, device=device)
            pieces = [scalar(p0), scalar(p1), zeros2]
            for layer in list(dense64)[:-1]:
                eta1, eta2 = layer.get_eta1_eta2()
                pieces += [eta1.reshape(1), eta2.reshape(1), zeros2] + padded(layer.network[0])
            pieces += padded(dense64[-1])
            image = torch.cat(pieces).float().contiguous()
        expected = ops.iresnet_image_floats(net.dimension, plan[3], net.densenet_depth, net.densenet_growth, act_id)
        assert image.numel() == expected, (image.numel(), expected)
        return image

    def _training_image(self, plan):
        """The image of ``_pack_image``, built differentiably in the modules' own dtype (float32 on the kernel route) from
        the live modules: every parametrised
        ``weight`` is evaluated exactly once (in training mode with its power iteration, as one composition call does),
        and the result is never cached -- it is a node of the caller's graph."""
        net = self.nnet
        layers = list(net.dense_net)
        device, dtype = layers[-1].bias.device, layers[-1].bias.dtype
        _, p0, p1 = _kernel_activation(net.activation)

        def scalar(fn):
            if fn is None:
                return torch.zeros(1, dtype=dtype, device=device)
            value = fn()
            if isinstance(value, torch.Tensor):
                return value.reshape(1)
            return torch.full((1,), value, dtype=dtype, device=device)

        def normalised(linear):
            # What ``linear.weight`` evaluates, once: the power iteration in training mode, then W / max(1, sigma /
            # coeff) with the factor held in float32 -- but sigma = <u, W v> summed in float64.  A float32 sum leaves
            # sigma, and with it every entry of a clamped weight, up to 3 ulp from the image of ``_pack_image``.
            norm, original = linear.parametrizations.weight[0], linear.parametrizations.weight.original
            if norm.training:
                norm._power_method(original, norm.n_power_iterations)
            sigma = torch.dot(norm._u.clone().double(), original.double() @ norm._v.clone().double())
            return original / torch.clamp(sigma / norm.coeff, min=1.0).to(torch.float32)

        def padded(linear):
            weight, bias = normalised(linear), linear.bias
            pad = ops._pad4(weight.shape[0]) - weight.shape[0]
            return [torch.nn.functional.pad(bias, (0, pad)), torch.nn.functional.pad(weight.t(), (0, pad)).reshape(-1)]

        zeros2 = torch.zeros(2, dtype=dtype, device=device)
        pieces = [scalar(p0), scalar(p1), zeros2]
        for layer in layers[:-1]:
            eta1, eta2 = layer.get_eta1_eta2()
            pieces += [eta1.reshape(1), eta2.reshape(1), zeros2] + padded(layer.network[0])
        pieces += padded(layers[-1])
        image = torch.cat(pieces)
        expected = ops.iresnet_image_floats(net.dimension, plan[3], net.densenet_depth, net.densenet_growth, plan[0])
        assert image.numel() == expected and image.dtype == dtype, (image.numel(), expected, image.dtype)
        return image

    def _extras(self, plan, context, differentiable=False):
        """Per-row extra input channels and output factor of the conditional nets (torch, eval-mode ``bn``);
        ``differentiable``: under the caller's autograd mode, so the context nets train through them."""
        net, extra, scale = self.nnet, None, None
        if context is None:
            return extra, scale
        with contextlib.nullcontext() if differentiable else torch.no_grad():
            context = net.bn(context)
            if plan[4]:
                scale = torch.tanh(net.factor_net(context)).reshape(-1).contiguous()
                extra = net.embedding(context).contiguous()
            else:
                extra = net.context_embedding_net(context).contiguous()
        return extra, scale

    def _shape_args(self, plan):
        net = self.nnet
        return net.dimension, plan[3], net.densenet_depth, net.densenet_growth, plan[0]

    def inverse_iterations(self):
        """Largest per-row iteration count of the last kernel ``inverse`` call (reads a device word: a host sync; for
        tools and tests).  None before the first such call."""
        word = ops.cached(self, "ires_iters")
        return None if word is None else int(word.item())

    # ---- the two directions -----------------------------------------------------------------------------------------

    @own_autograd_check
    def forward(self, inputs, context=None):
        plan = self._use_kernels(inputs, context)
        if plan is not None:
            extra, scale = self._extras(plan, context)
            return ops.iresnet_forward(inputs, self._image(plan), *self._shape_args(plan), extra=extra, scale=scale)
        plan = self._use_training_kernels(inputs, context)
        if plan is not None:
            extra, scale = self._extras(plan, context, differentiable=True)
            return ops.iresnet_autograd(inputs, self._training_image(plan), *self._shape_args(plan), extra=extra,
                                        scale=scale, _max_blocks=self._backward_blocks)
        g, logdetgrad = self._g_and_logabsdet(inputs, context=context)
        return inputs + g, logdetgrad.view(-1)

    @own_autograd_check
    def inverse(self, inputs, context=None):
        plan = self._use_kernels(inputs, context)
        if plan is not None:
            extra, scale = self._extras(plan, context)
            image, shape = self._image(plan), self._shape_args(plan)
            word = ops.memo(self, "ires_iters", inputs.device,
                            lambda: torch.zeros(1, dtype=torch.int32, device=inputs.device))
            x = ops.iresnet_inverse(inputs, image, *shape, extra=extra, scale=scale, iterations_out=word)
            _, lad = ops.iresnet_forward(x, image, *shape, extra=extra, scale=scale)
            return x, -lad
        x = self._inverse_fixed_point(inputs, context)
        return x, -self._g_and_logabsdet(x, context=context)[1]

    def extra_repr(self):
        estimator = self.train_determinant_estimator
        trace = getattr(getattr(estimator, "trace_estimator", None), "__name__", None)
        return 'brute_force={}, unbiased_estimator={}, trace_estimator={}'.format(
            self.brute_force, self.unbiased_estimator, trace)

    class Factory:
        """Collects the two halves of a block's configuration and builds as many blocks of it as asked for:
        ``Factory().set_densenet(**densenet_kwargs).set_logabsdet_estimator(brute_force=..., **options).build()``.
        ``set_densenet`` takes the arguments of ``DenseNet.factory`` (the ``condition_*`` switches included)."""

        _MISSING = {"args_iResBlock": "iResBlock arguments not set. Call set_iresblock.",
                    "densenet_factory": "DenseNet arguments not set. Call set_densenet."}

        def __init__(self):
            self._parts = dict.fromkeys(self._MISSING)

        args_iResBlock = property(lambda self: self._parts["args_iResBlock"])
        densenet_factory = property(lambda self: self._parts["densenet_factory"])

        def set_densenet(self, **kwargs):
            self._parts["densenet_factory"] = DenseNet.factory(**kwargs)
            return self

        def set_logabsdet_estimator(self, brute_force=False, unbiased_estimator=True, **options):
            self._parts["args_iResBlock"] = {"brute_force": brute_force, "unbiased_estimator": unbiased_estimator,
                                             **options}
            return self

        def build(self) -> 'iResBlock':
            for part, message in self._MISSING.items():
                assert self._parts[part] is not None, message
            return iResBlock(contractive_network=self.densenet_factory(), **self.args_iResBlock)


def _differentiable_input(x):
    """``x`` as a tensor autograd can differentiate with respect to, without touching the caller's tensor."""
    return x if x.requires_grad else x.detach().requires_grad_(True)


def _vjp(g, x, v, create_graph):
    """``v^T dg/dx`` per row; the graph of ``g`` is kept for the next product."""
    return torch.autograd.grad(g, x, v, create_graph=create_graph, retain_graph=True)[0]


def _row_dot(a, b):
    return (a.flatten(1) * b.flatten(1)).sum(dim=1)


class DeterminantEstimator(torch.nn.Module):
    """Base of the estimators of ``log|det(I + dg/dx)|``: ``logabsdet_and_g(x)`` returns ``(g(x), logabsdet [N])``."""

    OPTION_DEFAULTS = {"n_exact_terms": 2, "n_samples": 1, "n_power_series": 5, "trace_estimator": "neumann"}

    def __init__(self, network: _DenseNet, parameter_generator: ParameterGenerator):
        super().__init__()
        self.nnet = network
        self.parameter_generator = parameter_generator

    def logabsdet_and_g(self, x, context=None, training=False, **kwargs):
        coeff_fn, n_power_series = self.parameter_generator.sample_parameters(training=training)
        g, lad = self._g_and_logabsdet(coeff_fn=coeff_fn, n_power_series=n_power_series, x=x, context=context)
        return g, lad.view(-1)

    @abc.abstractmethod
    def _g_and_logabsdet(self, coeff_fn, n_power_series, x, context=None) -> Tuple[torch.Tensor, torch.Tensor]:
        pass

    @staticmethod
    def build(network, brute_force=False, unbiased_power_series=True, **options):
        """The exact estimator, or a power-series one with the Russian-roulette (unbiased) or the truncated (biased)
        coefficients; ``options`` override ``OPTION_DEFAULTS``."""
        if brute_force:
            return BruteForceDeterminantEstimator(network=network)
        chosen = {**DeterminantEstimator.OPTION_DEFAULTS, **options}
        if unbiased_power_series:
            generator = UnbiasedParameterGenerator(n_exact_terms=chosen["n_exact_terms"], n_samples=chosen["n_samples"])
        else:
            generator = BiasedParameterGenerator(n_power_series=chosen["n_power_series"])
        return ApproxTraceDeterminantEstimator(network=network, parameter_generator=generator,
                                               trace_estimator=chosen["trace_estimator"])


class BruteForceDeterminantEstimator(DeterminantEstimator):
    """The exact determinant: the full Jacobian from one backward pass per output dimension, then ``slogdet``."""

    def __init__(self, network: _DenseNet):
        super().__init__(network=network, parameter_generator=None)

    def logabsdet_and_g(self, x, context=None, training=False, **kwargs):
        return self._g_and_logabsdet(None, None, x, context=context)

    def _g_and_logabsdet(self, coeff_fn, n_power_series, x, context=None):
        x = _differentiable_input(x)
        g = self.nnet(x, context)
        jacobian = batch_jacobian(g, x)
        return g, logabsdet(jacobian + torch.eye(jacobian.shape[1], dtype=jacobian.dtype, device=jacobian.device))


class ApproxTraceDeterminantEstimator(DeterminantEstimator):
    """``log det(I + J) = sum_k (-1)^(k+1) c_k tr(J^k) / k`` with Hutchinson's trace estimate ``tr(A) ~ e^T A e`` from
    one Gaussian probe ``e`` and the products ``e^T J^k`` built up by vector-Jacobian products.

    * ``'basic'`` sums the series itself; with ``training`` every product stays differentiable.
    * ``'neumann'`` returns a surrogate whose GRADIENT is the estimate of the log-determinant's gradient
      (``d/dtheta log det(I + J) = tr((I + J)^-1 dJ/dtheta)``, the inverse as a Neumann series): the series
      ``e^T sum_k (-1)^k c_k J^k`` is formed without a graph, and only one last product with ``J`` is differentiable,
      so memory does not grow with the number of terms."""

    def __init__(self, *args, trace_estimator="neumann", **kwargs):
        super().__init__(*args, **kwargs)
        estimators = {"neumann": self.neumann_logdet_estimator, "basic": self.basic_logdet_estimator}
        if trace_estimator not in estimators:
            raise NotImplementedError(f"Unknown estimator '{trace_estimator}'. Has to be 'neumann' or 'basic'.")
        self.trace_estimator = estimators[trace_estimator]

    def logabsdet_and_g(self, x, context=None, training=False, **kwargs):
        coeff_fn, n_power_series = self.parameter_generator.sample_parameters(training=training)
        return self._g_and_logabsdet(coeff_fn=coeff_fn, n_power_series=n_power_series, x=x, context=context)

    def _g_and_logabsdet(self, coeff_fn, n_power_series, x, context=None) -> Tuple[torch.Tensor, torch.Tensor]:
        probe = torch.randn_like(x)
        x = _differentiable_input(x)
        g = self.nnet(x, context)
        return g, self.trace_estimator(g, x, n_power_series, probe, coeff_fn, self.training)

    @staticmethod
    def _series(g, x, n_power_series, probe, weight, create_graph):
        """Yields ``(weight(k), probe^T J^k)`` for k = 1 .. n_power_series."""
        product = probe
        for k in range(1, n_power_series + 1):
            product = _vjp(g, x, product, create_graph)
            yield weight(k), product

    @staticmethod
    def basic_logdet_estimator(g, x, n_power_series, vareps, coeff_fn, training):
        total = torch.zeros((), dtype=x.dtype, device=x.device)
        terms = ApproxTraceDeterminantEstimator._series(
            g, x, n_power_series, vareps, lambda k: (-1) ** (k + 1) / k * coeff_fn(k), create_graph=training)
        for weight, product in terms:
            total = total + weight * _row_dot(product, vareps)
        return total

    @staticmethod
    def neumann_logdet_estimator(g, x, n_power_series, vareps, coeff_fn, training):
        with torch.no_grad():
            series = vareps
            terms = ApproxTraceDeterminantEstimator._series(
                g, x, n_power_series, vareps, lambda k: (-1) ** k * coeff_fn(k), create_graph=False)
            for weight, product in terms:
                series = series + weight * product
        return _row_dot(_vjp(g, x, series, create_graph=training), vareps)
