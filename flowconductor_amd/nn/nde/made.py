"""``MixtureOfGaussiansMADE``: a MADE whose outputs are, per input feature, the logits, means and unconstrained standard
deviations of a mixture of Gaussians (API and ``state_dict`` keys of flowcon/nn/nde/made.py:284-426).

The density is one HIP kernel on the final layer's output (``fc_mog_log_prob``, with ``fc_mog_log_prob_backward`` under
autograd); ancestral sampling runs its D passes in ONE kernel (``fc_made_mog_sample`` / ``fc_made_mog_sample_context``:
the device loop of the autoregressive inverse with a mixture column step) wherever that kernel has the shape, and as a
host loop of D conditioner passes on PyTorch otherwise.  Every route has a torch composition twin
(``log_prob_composition``, ``_sample_host_loop``) that serves CPU tensors, float64 and the shapes the kernels lack.

Two things differ from the MADE of ``transforms/made.py`` this class derives from, both as in the reference's
``nn/nde/made.py`` (which is NOT a copy of its ``transforms/made.py``): the context term of the initial layer enters
without an activation (nn/nde/made.py:274-281), and with feed-forward blocks no activation follows the initial layer.
"""
import numpy as np
import torch
from torch.nn import functional as F

from flowconductor_amd import ops, options
from flowconductor_amd.transforms.made import MADE, device_loop_rows_ok, pad_rows


class MixtureOfGaussiansMADE(MADE):
    def __init__(self, features, hidden_features, context_features=None, num_blocks=2, num_mixture_components=5,
                 use_residual_blocks=True, random_mask=False, activation=F.relu, dropout_probability=0.0,
                 use_batch_norm=False, epsilon=1e-2, custom_initialization=True):
        if use_residual_blocks and random_mask:
            raise ValueError("Residual blocks can't be used with random masks.")
        super().__init__(features, hidden_features, context_features=context_features, num_blocks=num_blocks,
                         output_multiplier=3 * num_mixture_components, use_residual_blocks=use_residual_blocks,
                         random_mask=random_mask, activation=activation, dropout_probability=dropout_probability,
                         use_batch_norm=use_batch_norm)
        self.num_mixture_components = num_mixture_components
        self.features = features
        self.hidden_features = hidden_features
        self.epsilon = epsilon
        if custom_initialization:
            self._initialize()

    def _initialize(self):
        """nn/nde/made.py:390-419: logits near zero (mixture coefficients about uniform), unconstrained standard
        deviations near softplus^-1(1 - epsilon) (standard deviations about 1); the means keep nn.Linear's default."""
        rows = self.features * self.num_mixture_components
        final = self.final_layer
        final.weight.data[::3, :] = self.epsilon * torch.randn(rows, self.hidden_features)
        final.bias.data[::3] = self.epsilon * torch.randn(rows)
        final.weight.data[2::3] = self.epsilon * torch.randn(rows, self.hidden_features)
        final.bias.data[2::3] = (torch.log(torch.exp(torch.Tensor([1 - self.epsilon])) - 1) * torch.ones(rows)
                                 + self.epsilon * torch.randn(rows))

    # ---- the conditioner ---------------------------------------------------------------------------------------------
    def hidden(self, inputs, context=None):
        """Everything before the final masked Linear, as nn/nde/made.py:274-279 composes it."""
        h = self.initial_layer(inputs)
        if context is not None:
            h = h + self.context_layer(context)
        for block in self.blocks:
            h = block(h, context)
        return h

    def hip_hidden_supported(self, context=None):
        """The fused hidden stack applies without a context only: ``fc_resnet_hidden_context`` passes the initial
        layer's context term through the activation (transforms/made.py), this net adds it as it is."""
        return context is None and super().hip_hidden_supported(None)

    def _params(self, inputs, context):
        """The final layer's output [N, D * 3C]; the hidden stack runs in ``fc_resnet_hidden`` where it applies
        (inference, no context, >= 16 float32 device rows)."""
        n = inputs.shape[0]
        if (inputs.dim() == 2 and inputs.is_cuda and inputs.dtype == torch.float32 and n >= ops.HIDDEN_ROWS
                and options.get("fused_hidden") and self.hip_hidden_supported(context) and not ops.has_hooks(self)
                and not self._needs_grad(inputs, context)):
            body = n - n % ops.HIDDEN_ROWS
            hidden = self.hidden_hip(inputs[:body].contiguous())
            if body < n:
                tail = self.hidden(inputs[body:], None)
                hidden = torch.cat((hidden, F.pad(tail, (0, hidden.shape[1] - tail.shape[1]))))
            weight, bias = self.masked_final(hidden.shape[1])
            return F.linear(hidden, weight, bias)
        return self.final_layer(self.hidden(inputs, context))

    def _needs_grad(self, inputs, context=None):
        return torch.is_grad_enabled() and (inputs.requires_grad or (context is not None and context.requires_grad)
                                            or any(p.requires_grad for p in ops.param_list(self)))

    # ---- density -----------------------------------------------------------------------------------------------------
    def _density_kernel_ok(self, inputs):
        return (inputs.dim() == 2 and inputs.is_cuda and inputs.dtype == torch.float32 and inputs.shape[0] >= 1
                and 1 <= self.num_mixture_components <= ops.MOG_MAX_COMPONENTS and not ops.has_hooks(self)
                and inputs.shape[1] == self.features)

    def log_prob(self, inputs, context=None):
        if not self._density_kernel_ok(inputs):
            return self.log_prob_composition(inputs, context)
        params = self._params(inputs, context)
        return ops.mog_log_prob(inputs, params, self.num_mixture_components, self.epsilon)

    def log_prob_composition(self, inputs, context=None):
        """The reference's expression (nn/nde/made.py:328-353) on PyTorch."""
        outputs = self.forward(inputs, context=context)
        return _mixture_log_density(outputs.reshape(*inputs.shape, self.num_mixture_components, 3), inputs, self.epsilon)

    # ---- sampling ----------------------------------------------------------------------------------------------------
    def sample(self, num_samples, context=None):
        """``[B, num_samples, D]`` draws for the B rows of ``context`` (nn/nde/made.py:355-388), ``[num_samples, D]``
        without one (an extension: the reference fails on ``context.shape``).  The draws live on the parameters' device
        (the reference allocates them on the CPU whatever the device).

        Column d picks its component by inverse-CDF selection on one uniform number where the reference calls
        ``Categorical.sample``: the draws follow the same law, but not the same random stream."""
        return self.sample_and_log_prob(num_samples, context)[0]

    def sample_and_log_prob(self, num_samples, context=None):
        """The draws of ``sample`` and their log-densities ([B, num_samples] / [num_samples]) from the same pass: the
        sampler holds every column's mixture parameters when it draws the column."""
        weight = self.final_layer.weight
        rows_context = None
        rows = num_samples
        if context is not None:
            context = torch.as_tensor(context).to(device=weight.device, dtype=weight.dtype)
            rows_context = context.repeat_interleave(num_samples, dim=0)       # torchutils.repeat_rows
            rows = rows_context.shape[0]
        normal = torch.randn(rows, self.features, device=weight.device, dtype=weight.dtype)
        uniform = torch.rand(rows, self.features, device=weight.device, dtype=weight.dtype)
        draws, log_prob = self._sample_from_noise(normal, uniform, rows_context, with_log_prob=True)
        if context is None:
            return draws, log_prob
        return draws.reshape(-1, num_samples, self.features), log_prob.reshape(-1, num_samples)

    def _sample_from_noise(self, normal, uniform, context_rows=None, with_log_prob=False):
        """The deterministic part of sampling: ``normal``, ``uniform`` [rows, D] noise -> draws [rows, D].  Column d takes
        component ``k = min{k : uniform_d * S < sum_{j <= k} e_j}`` with ``e_j = exp(logit_j - max logit)`` and
        ``S = sum_j e_j`` (the last component when no partial sum exceeds it), then ``x_d = mean_k + std_k * normal_d``.
        No gradient flows through sampling (as in the reference).  ``with_log_prob``: also the draws' log-density."""
        with torch.no_grad():
            if self._sample_kernel_ok(normal, context_rows):
                draws, log_prob = self._sample_device_loop(normal, uniform, context_rows)
            else:
                draws, log_prob = self._sample_host_loop(normal, uniform, context_rows)
        return (draws, log_prob) if with_log_prob else draws

    def _sample_kernel_ok(self, normal, context):
        """``fc_made_mog_sample(_context)`` has the shape: float32 device noise and context as the device loops take them
        (``device_loop_rows_ok``), a context exactly when the net has context layers, <= 16 components, a MADE the loops
        hold (``MADE.device_loop_supported``), no hooks.  Sampling runs under ``no_grad``: gradients are not asked about."""
        if hasattr(self, "context_layer") != (context is not None) or not device_loop_rows_ok(normal, context):
            return False

        def structure_ok():
            return (1 <= self.num_mixture_components <= ops.MOG_MAX_COMPONENTS
                    and self.device_loop_supported(normal.shape[1], 3 * self.num_mixture_components, 48, context))

        key = (normal.shape[1], None if context is None else context.shape[1]) + ops.structure_key(self)
        return ops.static_memo(self, "mog_sample_ok", key, structure_ok) and not ops.has_hooks(self)

    def _sample_device_loop(self, normal, uniform, context):
        pack, context_pack = self.inverse_packs(3 * self.num_mixture_components, context is not None)
        n = normal.shape[0]
        draws, log_prob = ops.made_mog_sample(
            pad_rows(normal), pad_rows(uniform), pack, len(self.blocks), self.num_mixture_components, self.epsilon,
            context=None if context is None else pad_rows(context), context_pack=context_pack)
        return (draws, log_prob) if draws.shape[0] == n else (draws[:n], log_prob[:n])

    def _sample_host_loop(self, normal, uniform, context):
        """D conditioner passes, pass d fixing column d with the selection rule of ``_sample_from_noise`` on the same
        noise.  Only column d is written in pass d, so the unfinished columns stay zero between passes: the hidden-stack
        kernel scales every row by its maximum before the f16 split and must not see values a kept column never reads
        (``AutoregressiveTransform.inverse`` clears them for the same reason)."""
        n, components = normal.shape[0], self.num_mixture_components
        draws = torch.zeros_like(normal)
        log_prob = normal.new_zeros(n)
        for d in range(self.features):
            outputs = self._params(draws, context).reshape(n, self.features, components, 3)[:, d]
            logits, means, unconstrained_stds = outputs[..., 0], outputs[..., 1], outputs[..., 2]
            weights = torch.exp(logits - logits.max(dim=-1, keepdim=True).values)
            partial = torch.cumsum(weights, dim=-1)
            target = uniform[:, d:d + 1] * partial[:, -1:]
            chosen = (target >= partial).sum(dim=-1, keepdim=True).clamp(max=components - 1)
            stds = F.softplus(unconstrained_stds) + self.epsilon
            column = means.gather(1, chosen)[:, 0] + stds.gather(1, chosen)[:, 0] * normal[:, d]
            draws[:, d] = column
            log_prob += _mixture_log_density(outputs, column, self.epsilon, sum_features=False)
        return draws, log_prob


def _mixture_log_density(outputs, inputs, epsilon, sum_features=True):
    """nn/nde/made.py:332-353 on ``outputs`` [..., C, 3] and ``inputs`` [...]."""
    logits, means, unconstrained_stds = outputs[..., 0], outputs[..., 1], outputs[..., 2]
    log_mixture_coefficients = torch.log_softmax(logits, dim=-1)
    stds = F.softplus(unconstrained_stds) + epsilon
    terms = torch.logsumexp(
        log_mixture_coefficients - 0.5 * (np.log(2 * np.pi) + 2 * torch.log(stds) + ((inputs[..., None] - means) / stds) ** 2),
        dim=-1)
    return torch.sum(terms, dim=-1) if sum_features else terms
