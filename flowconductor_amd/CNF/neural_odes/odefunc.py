"""``ODEnet`` (the dynamics network) and ``ODEfunc`` (dynamics plus divergence: the right-hand side of the CNF's
augmented ODE); classes, constructor arguments and ``state_dict`` keys of flowcon/CNF/neural_odes/odefunc.py.

Three routes for ``ODEfunc.forward``:

* the torch composition: the net, then in eval mode the exact divergence from ``D`` backward passes, in training mode
  ``divergence_fn`` (Hutchinson's estimator with a noise vector fixed per solve, or the exact one).  Any device and
  dtype, differentiable;
* in eval mode, without gradients, for contiguous float32 ``[N, D]`` rows on a HIP device and an ``ODEnet`` within
  the kernel's limits (D <= 16, at most 4 hidden layers of at most 64 units, ignore / concat / concat_v2 / squash /
  concatsquash layers, no act_norm): ``fc_cnf_field`` computes the value and the exact forward-mode divergence in
  one launch, for batches up to the size at which it measured faster than the composition (``ops.cnf_rows_pay``;
  DESIGN.md, "Continuous normalizing flows");
* with options ``cnf_training``, in training mode or wherever a gradient is needed, under the same conditions with at
  most 3 hidden layers, two states and no gradient for ``t``: one autograd node of ``fc_cnf_field_train`` and
  ``fc_cnf_field_backward`` (Hutchinson's estimate with the solve's noise, or the exact divergence), once
  differentiable, for batches up to ``ops.CNF_TRAIN_MAX_LANES`` lanes ("CNF training").

Only ``conv=False`` nets are built."""
import contextlib
import weakref
from typing import NamedTuple

import torch
from torch import nn

from flowconductor_amd import ops, options

from . import diffeq_layers
from .util import Lambda, divergence_approx, divergence_bf, sample_gaussian_like, sample_rademacher_like

__all__ = ["ODEnet", "ODEfunc"]


class _KernelPlan(NamedTuple):
    """What is fixed by how the net is built, as the CNF kernels take it (``ODEfunc._kernel_plan``)."""
    d: int              # width of the rows: the first layer's inputs without the time column of a concat layer
    hidden: tuple
    layer_kind: int
    activation: int
    p0: float


def _square(x):
    return x ** 2


NONLINEARITIES = {
    "tanh": nn.Tanh(),
    "relu": nn.ReLU(),
    "softplus": nn.Softplus(),
    "elu": nn.ELU(),
    "swish": nn.SiLU(),
    "square": Lambda(_square),
    "identity": nn.Identity(),
}

_LINEAR_LAYERS = {
    "ignore": diffeq_layers.IgnoreLinear,
    "hyper": diffeq_layers.HyperLinear,
    "squash": diffeq_layers.SquashLinear,
    "concat": diffeq_layers.ConcatLinear,
    "concat_v2": diffeq_layers.ConcatLinear_v2,
    "concatsquash": diffeq_layers.ConcatSquashLinear,
    "blend": diffeq_layers.BlendLinear,
    "concatcoord": diffeq_layers.ConcatLinear,
}

_KERNEL_LAYERS = {
    diffeq_layers.IgnoreLinear: ops.CNF_LAYER_IGNORE,
    diffeq_layers.ConcatLinear: ops.CNF_LAYER_CONCAT,
    diffeq_layers.ConcatLinear_v2: ops.CNF_LAYER_CONCAT_V2,
    diffeq_layers.SquashLinear: ops.CNF_LAYER_SQUASH,
    diffeq_layers.ConcatSquashLinear: ops.CNF_LAYER_CONCATSQUASH,
}


def _kernel_activation(act):
    """``(kernel activation id, p0)`` or None for a module the kernels do not evaluate (exact types only)."""
    kind = type(act)
    if kind is nn.Tanh:
        return ops.CNF_ACT_TANH, 1.0
    if kind is nn.ReLU:
        return ops.CNF_ACT_RELU, 1.0
    if kind is nn.Softplus and act.beta == 1 and act.threshold == 20:
        return ops.CNF_ACT_SOFTPLUS, 1.0
    if kind is nn.ELU:
        return ops.CNF_ACT_ELU, float(act.alpha)
    if kind is nn.SiLU:
        return ops.CNF_ACT_SWISH, 1.0
    if act is NONLINEARITIES["square"]:
        return ops.CNF_ACT_SQUARE, 1.0
    if kind is nn.Identity:
        return ops.CNF_ACT_IDENTITY, 1.0
    return None


class ODEnet(nn.Module):
    """The dynamics ``f(t, y)``: time-conditioned linear layers of one ``layer_type`` with ``nonlinearity`` between
    them, the output multiplied by ``scale_output``."""

    def __init__(self, hidden_dims, input_shape, strides, conv, layer_type="concat", nonlinearity="softplus",
                 num_squeeze=0, act_norm=False, scale_output=1):
        super().__init__()
        if conv:
            raise NotImplementedError("flowconductor_amd: ODEnet is built for conv=False only; the convolutional "
                                      "diffeq layers are not part of this package")
        if num_squeeze:
            raise NotImplementedError("flowconductor_amd: ODEnet(num_squeeze > 0) belongs to the convolutional nets, "
                                      "which are not part of this package")
        self.act_norm = act_norm
        if act_norm:
            from flowconductor_amd.transforms import ActNorm

            self.t_actnorm = ActNorm(1)
            self.x_actnorm = ActNorm(input_shape[0])
        self.scale_output = scale_output
        self.num_squeeze = num_squeeze
        base_layer = _LINEAR_LAYERS[layer_type]
        layers, width = [], input_shape[0]
        for dim_out in tuple(hidden_dims) + (input_shape[0],):
            layers.append(base_layer(width, dim_out))
            width = dim_out
        self.layers = nn.ModuleList(layers)
        self.activation_fns = nn.ModuleList([NONLINEARITIES[nonlinearity]] * (len(layers) - 1))

    def forward(self, t, y):
        if self.act_norm:
            t = self.t_actnorm(t.view(-1, 1))[0].view(t.shape)
            y, _ = self.x_actnorm(y)
        dx = y
        for index, layer in enumerate(self.layers):
            dx = layer(t, dx)
            if index < len(self.layers) - 1:
                dx = self.activation_fns[index](dx)
        return dx * self.scale_output


class ODEfunc(nn.Module):
    """``forward(t, (y, logp, ...)) -> (dy/dt, dlogp/dt = -div_y f, zeros...)``."""

    def __init__(self, diffeq, divergence_fn="approximate", residual=False, rademacher=False):
        super().__init__()
        assert divergence_fn in ("brute_force", "approximate")
        self.diffeq = diffeq
        self.residual = residual
        self.rademacher = rademacher
        self.divergence_fn = divergence_bf if divergence_fn == "brute_force" else divergence_approx
        self.register_buffer("_num_evals", torch.tensor(0.))
        self.before_odeint()

    def before_odeint(self, e=None):
        self._e = e
        self._drop_training_image()
        self._num_evals.fill_(0)

    def num_evals(self):
        return self._num_evals.item()

    # ---- the kernel ---------------------------------------------------------------------------------------------------

    def _kernel_plan(self):
        """What is fixed by how the net is built, a ``_KernelPlan``, or None."""
        net = self.diffeq
        if type(net) is not ODEnet or net.act_norm or net.num_squeeze:
            return None
        layers = list(net.layers)
        kind = _KERNEL_LAYERS.get(type(layers[0])) if layers else None
        if kind is None or any(type(layer) is not type(layers[0]) for layer in layers):
            return None
        extra = 1 if kind == ops.CNF_LAYER_CONCAT else 0
        widths = [layers[0]._layer.in_features - extra]
        for layer in layers:
            if layer._layer.in_features - extra != widths[-1] or layer._layer.bias is None:
                return None
            widths.append(layer._layer.out_features)
        if widths[-1] != widths[0] or not ops.cnf_supported(widths[0], widths[1:-1]):
            return None
        if len(net.activation_fns) != len(layers) - 1 or any(a is not net.activation_fns[0] for a in net.activation_fns):
            return None
        act = _kernel_activation(net.activation_fns[0]) if len(layers) > 1 else (ops.CNF_ACT_IDENTITY, 1.0)
        if act is None:
            return None
        return _KernelPlan(widths[0], tuple(widths[1:-1]), kind, act[0], act[1])

    def _use_kernels(self, y):
        """The plan when this call can run on the eval-mode kernels, else None."""
        route = options.get("cnf_kernels")
        if not route or self.training or not isinstance(y, torch.Tensor):
            return None
        if not (y.is_cuda and y.dtype == torch.float32 and y.dim() == 2 and y.shape[0] > 0 and y.is_contiguous()):
            return None
        if route != "force" and not ops.cnf_rows_pay(y.shape[0], y.shape[1]):
            return None     # measured slower than the composition ("Continuous normalizing flows")
        if self._needs_grad(y):
            return None
        if any(m.training for m in ops.module_list(self)):
            return None
        return self._plan_for(y)

    def _needs_grad(self, y):
        return torch.is_grad_enabled() and (y.requires_grad or any(p.requires_grad for p in ops.param_list(self)))

    def _use_training_kernels(self, t, states):
        """``(plan, hutchinson)`` when this call can run as one ``fc_cnf_field_train`` / ``fc_cnf_field_backward``
        node (options ``cnf_training``), else None: training mode or a gradient needed, no regulariser states (they
        differentiate ``dy`` again), no gradient for ``t``, the eval kernels' conditions on the net and the rows, a
        net within ``ops.cnf_train_supported`` and a batch within ``ops.CNF_TRAIN_MAX_LANES`` lanes."""
        route = options.get("cnf_training")
        y = states[0]
        if not route or len(states) != 2 or not isinstance(y, torch.Tensor):
            return None
        if isinstance(t, torch.Tensor) and t.requires_grad and torch.is_grad_enabled():
            return None
        if not (y.is_cuda and y.dtype == torch.float32 and y.dim() == 2 and y.shape[0] > 0 and y.is_contiguous()):
            return None
        if not (self.training or self._needs_grad(y)):
            return None
        hutchinson = self.training and self.divergence_fn is divergence_approx      # eval mode is always exact
        if route != "force" and not ops.cnf_train_rows_pay(y.shape[0], y.shape[1], hutchinson):
            return None     # no measured win over the composition ("CNF training")
        e = self._e
        if hutchinson and e is not None and not (
                isinstance(e, torch.Tensor) and e.dtype == torch.float32 and e.device == y.device
                and e.shape == y.shape and e.is_contiguous() and not e.requires_grad):
            return None
        plan = self._plan_for(y)
        if plan is None or not ops.cnf_train_supported(plan.d, plan.hidden):
            return None
        return plan, hutchinson

    def _plan_for(self, y):
        """The plan when the net, its parameters and the evaluation counter are what the kernels take for the float32
        device rows ``y``, else None."""
        params = ops.param_list(self)
        if any(p.dtype != torch.float32 or p.device != y.device for p in params) or ops.has_hooks(self):
            return None
        if self._num_evals.dtype != torch.float32 or self._num_evals.device != y.device:
            return None
        net = self.diffeq
        structure = (id(net), len(getattr(net, "layers", ())), id(getattr(net, "activation_fns", None)),
                     getattr(net, "act_norm", None), getattr(net, "num_squeeze", None))
        plan = ops.static_memo(self, "cnf_plan", structure, self._kernel_plan)
        if plan is None or y.shape[1] != plan.d:
            return None
        scale = net.scale_output
        if isinstance(scale, torch.Tensor) or not isinstance(self.residual, (bool, int)):
            return None
        return plan

    def _image(self, plan):
        """The packed net on the device, once per parameter version (torch ops on the device, no host sync)."""
        return ops.memo(self, "cnf_image", ops.cache_key(*ops.param_list(self)), lambda: self._pack_image(plan))

    def _training_image(self, plan):
        """The packed net as a differentiable function of the parameters, one tensor per solve: every evaluation of
        a solve hands its ``g_image`` to the same node, so the unpacking runs once per backward.  ``before_odeint``
        drops it, and so does the first gradient that reaches it (a backward frees its graph): a later call packs
        again."""
        def build():
            image, token, owner = self._pack_image(plan, differentiable=True), object(), weakref.ref(self)

            def consumed(grad):
                module = owner()
                held = None if module is None else ops.cached(module, "cnf_training_image")
                if held is not None and held[0] is token:
                    module._drop_training_image()

            image.register_hook(consumed)
            return token, image

        return ops.memo(self, "cnf_training_image", ops.cache_key(*ops.param_list(self)), build)[1]

    def _drop_training_image(self):
        self.__dict__.get("_fc_cache", {}).pop("cnf_training_image", None)

    def _pack_image(self, plan, differentiable=False):
        kind, pieces = plan.layer_kind, []
        with (contextlib.nullcontext() if differentiable else torch.no_grad()):
            for layer in self.diffeq.layers:
                weight, bias = layer._layer.weight, layer._layer.bias
                out = weight.shape[0]
                op = ops._cnf_pad4(out)
                zero = weight.new_zeros(op)

                def padded(vector):
                    return torch.cat([vector.reshape(-1), weight.new_zeros(op - out)])

                w_t = w_g = b_g = w_b = zero
                if kind == ops.CNF_LAYER_CONCAT:
                    w_t, weight = padded(weight[:, 0]), weight[:, 1:]
                elif kind == ops.CNF_LAYER_CONCAT_V2:
                    w_b = padded(layer._hyper_bias.weight)
                elif kind == ops.CNF_LAYER_SQUASH:
                    w_g, b_g = padded(layer._hyper.weight), padded(layer._hyper.bias)
                elif kind == ops.CNF_LAYER_CONCATSQUASH:
                    w_g, b_g = padded(layer._hyper_gate.weight), padded(layer._hyper_gate.bias)
                    w_b = padded(layer._hyper_bias.weight)
                wt = weight.new_zeros(weight.shape[1], op)
                wt[:, :out] = weight.t()
                pieces += [padded(bias), w_t, w_g, b_g, w_b, wt.reshape(-1)]
            image = torch.cat(pieces).contiguous()
        assert image.numel() == ops.cnf_image_floats(plan.d, plan.hidden), image.numel()
        return image

    def _kernel_args(self, plan):
        """The arguments ``ops.cnf_field`` / ``ops.cnf_integrate`` share, as keywords."""
        return dict(image=self._image(plan), d=plan.d, hidden=plan.hidden, layer_kind=plan.layer_kind,
                    activation=plan.activation, residual=bool(self.residual),
                    scale_output=float(self.diffeq.scale_output), p0=plan.p0, evals=self._num_evals)

    # ---- one evaluation -----------------------------------------------------------------------------------------------

    def forward(self, t, states):
        assert len(states) >= 2
        y = states[0]
        if len(states) == 2 and not (isinstance(t, torch.Tensor) and t.requires_grad and torch.is_grad_enabled()):
            plan = self._use_kernels(y)
            if plan is not None:
                if isinstance(t, torch.Tensor):
                    if t.is_cuda:
                        t = t.detach().reshape(1).to(device=y.device, dtype=torch.float32)
                    else:
                        t = float(t)
                dy, negdiv = ops.cnf_field(t, y, **self._kernel_args(plan))
                return dy, negdiv.view(-1, 1)
        route = self._use_training_kernels(t, states)
        if route is not None:
            return self._training_node(t, y, *route)
        return self._composition(t, states)

    def _training_node(self, t, y, plan, hutchinson):
        """One evaluation as one autograd node (one launch forward, one backward); without a gradient to carry, the
        forward launch alone."""
        if self.training and self._e is None:       # where, and by the call with which, the composition draws it
            self._e = sample_rademacher_like(y) if self.rademacher else sample_gaussian_like(y)
        if isinstance(t, torch.Tensor):
            t = t.detach().reshape(1).to(device=y.device, dtype=torch.float32) if t.is_cuda else float(t)
        e = self._e if hutchinson else None
        kw = self._kernel_args(plan)
        if not self._needs_grad(y):
            dy, negdiv = ops.cnf_field_train(t, y, e, **kw)
        else:
            if torch.is_grad_enabled() and any(p.requires_grad for p in ops.param_list(self)):
                kw["image"] = self._training_image(plan)
            image = kw.pop("image")
            dy, negdiv = ops._CnfFieldFunction.apply(y, image, e, t, kw)
        return dy, negdiv.view(-1, 1)

    def _composition(self, t, states):
        y = states[0]
        self._num_evals += 1
        t = torch.as_tensor(t).to(y)
        batch = y.shape[0]
        if self.training and self._e is None:       # fixed for the whole solve (before_odeint clears it)
            self._e = sample_rademacher_like(y) if self.rademacher else sample_gaussian_like(y)
        keep_graph = torch.is_grad_enabled()
        with torch.enable_grad():
            y_in = y if y.requires_grad else y.detach().requires_grad_(True)
            dy = self.diffeq(t, y_in, *states[2:])
            if self.training:
                divergence = self.divergence_fn(dy, y_in, e=self._e).view(batch, 1)
            else:   # eval mode is always exact
                divergence = divergence_bf(dy, y_in, create_graph=keep_graph).view(batch, 1)
            if self.residual:
                dy = dy - y_in
                divergence = divergence - float(y[0].numel())
        negdiv = -divergence
        if not keep_graph:
            dy, negdiv = dy.detach(), negdiv.detach()
        return (dy, negdiv) + tuple(torch.zeros_like(s) for s in states[2:])
