"""``CNF``: a continuous normalizing flow, the solution map of ``dz/dt = f(t, z)`` with ``dlogp/dt = -div f`` carried
along (class, constructor arguments and ``state_dict`` keys of flowcon/CNF/cnf.py), and ``CNFTransform``, which makes
one a ``Transform``.

The solver is the package's own (``flowconductor_amd.CNF.odeint``).  ``solver_options`` reaches it in eval mode as
well as in training mode (a fixed-step ``test_solver`` is of little use without its ``step_size``).

Routes of ``CNF.forward`` in eval mode, for an ``odefunc`` the kernels take (see ``ODEfunc``) and two integration
times:
* ``test_solver`` in ``euler`` / ``midpoint`` / ``rk4``: the whole solve is one ``fc_cnf_integrate`` launch;
* ``dopri5``: the host loop of ``odeint`` with one ``fc_cnf_field`` launch per evaluation, the batch judged as one
  system;
* ``dopri5`` with options ``cnf_dopri5_kernel`` (off by default), tolerances of at least 1e-6 and a batch within
  ``ops.cnf_dopri5_rows_pay``: the whole adaptive solve is one ``fc_cnf_dopri5`` launch in which every row controls
  its own step (a row is judged by its own error, and one that cannot finish within ``max_num_steps``, clipped to
  4096, attempts returns NaN where the host loop raises).
In training mode, or wherever a gradient is needed, with options ``cnf_solve_training`` (off by default), a solver in
``euler`` / ``midpoint`` / ``rk4``, two integration times that are numbers, no regulariser and a net within
``ops.cnf_solve_train_fits``: the whole solve is one autograd node, one ``fc_cnf_integrate_train`` launch forward and one
``fc_cnf_integrate_backward`` launch backward (``_training_solve``; DESIGN.md, "CNF training: the whole solve").
Everything else is the torch composition on the tensors' device (or the per-evaluation nodes of ``cnf_training``)."""
import torch
from torch import nn

from flowconductor_amd import ops, options
from flowconductor_amd.transforms.base import Transform

from .neural_odes.odefunc import ODEfunc
from .neural_odes.util import divergence_approx, sample_gaussian_like, sample_rademacher_like
from .neural_odes.wrappers.cnf_regularization import RegularizedODEfunc
from .odeint import fixed_grid_steps, odeint

__all__ = ["CNF", "CNFTransform"]


class CNF(nn.Module):
    def __init__(self, odefunc, T=1.0, train_T=False, regularization_fns=None, solver='dopri5', atol=1e-5, rtol=1e-5):
        super().__init__()
        sqrt_end_time = torch.sqrt(torch.tensor(float(T)))
        if train_T:
            self.register_parameter("sqrt_end_time", nn.Parameter(sqrt_end_time))
        else:
            self.register_buffer("sqrt_end_time", sqrt_end_time)
        nreg = 0
        if regularization_fns is not None:
            odefunc = RegularizedODEfunc(odefunc, regularization_fns)
            nreg = len(regularization_fns)
        self.odefunc = odefunc
        self.nreg = nreg
        self.regularization_states = None
        self.solver = solver
        self.atol = atol
        self.rtol = rtol
        self.test_solver = solver
        self.test_atol = atol
        self.test_rtol = rtol
        self.solver_options = {}

    def _default_times(self, z):
        """``[0, sqrt_end_time ** 2]``: a tensor where the end time is being trained, else two floats whose read of
        the buffer is kept per version of it (no host sync on later calls)."""
        end = self.sqrt_end_time
        if end.requires_grad and torch.is_grad_enabled():
            return torch.stack([torch.zeros_like(end), end * end]).to(z)
        value = ops.memo(self, "end_time", ops.cache_key(end), lambda: float((end.detach() * end.detach()).float()))
        return [0.0, value]

    def _kernel_solve(self, z, logpz, times):
        """``(z_t, logp_t)`` from one ``fc_cnf_integrate`` or ``fc_cnf_dopri5`` launch, or None when this call is not
        one for them."""
        method = ops.CNF_METHODS.get(self.test_solver)
        adaptive = method is None and self.test_solver == "dopri5" and bool(options.get("cnf_dopri5_kernel"))
        if self.training or not (adaptive or method is not None) or len(times) != 2 \
                or any(isinstance(v, torch.Tensor) for v in times):
            return None
        func = self.odefunc.odefunc if isinstance(self.odefunc, RegularizedODEfunc) else self.odefunc
        if type(func) is not ODEfunc or ops.has_hooks(self):
            return None
        if not (isinstance(logpz, torch.Tensor) and logpz.is_cuda and logpz.dtype == torch.float32
                and logpz.device == z.device and logpz.numel() == z.shape[0] and logpz.is_contiguous()
                and not (torch.is_grad_enabled() and logpz.requires_grad)):
            return None
        plan = func._use_kernels(z)
        if plan is None:
            return None
        if adaptive:
            return self._dopri5_solve(func, plan, z, logpz, times)
        steps = fixed_grid_steps(times[0], times[1], self.solver_options)
        z_t, logp_t = ops.cnf_integrate(z, logpz, t0=times[0], t1=times[1], steps=steps, method=method,
                                        **func._kernel_args(plan))
        return z_t, logp_t.view(logpz.shape)

    def _dopri5_solve(self, func, plan, z, logpz, times):
        """The adaptive solve in one ``fc_cnf_dopri5`` launch (options ``cnf_dopri5_kernel``), or None: tolerances
        below ``ops.CNF_DOPRI5_MIN_TOL``, a batch beyond ``ops.cnf_dopri5_rows_pay`` (unless the option is "force"),
        or solver options the kernel has no argument for keep the host loop."""
        tolerances = (self.test_atol, self.test_rtol)
        if not all(isinstance(v, (int, float)) for v in tolerances) \
                or not ops.cnf_dopri5_fits(plan.d, plan.hidden, *tolerances):
            return None
        if options.get("cnf_dopri5_kernel") != "force" and not ops.cnf_dopri5_rows_pay(z.shape[0], z.shape[1]):
            return None     # no measured win over the host loop ("dopri5 in one launch")
        first_step = self.solver_options.get("first_step")
        if first_step is not None and not (isinstance(first_step, (int, float)) and 0.0 < first_step < float("inf")):
            return None
        max_attempts = ops.cnf_dopri5_attempts(self.solver_options.get("max_num_steps"))
        if max_attempts is None:
            return None
        z_t, logp_t, _ = ops.cnf_dopri5(z, logpz, t0=times[0], t1=times[1], atol=tolerances[0], rtol=tolerances[1],
                                        first_step=first_step, max_attempts=max_attempts, **func._kernel_args(plan))
        return z_t, logp_t.view(logpz.shape)

    def _training_solve(self, z, logpz, times):
        """``(z_t, logp_t)`` from one ``_CnfSolveFunction`` node (options ``cnf_solve_training``): one
        ``fc_cnf_integrate_train`` launch forward and one ``fc_cnf_integrate_backward`` launch backward; or None when
        this call is not one for them, before anything has been drawn or counted."""
        route = options.get("cnf_solve_training")
        func = self.odefunc
        if not route or self.nreg or type(func) is not ODEfunc or ops.has_hooks(self) \
                or func.training != self.training:
            return None
        method = ops.CNF_METHODS.get(self.solver if self.training else self.test_solver)
        if method is None or len(times) != 2 or any(isinstance(v, torch.Tensor) for v in times):
            return None
        if not (isinstance(z, torch.Tensor) and z.is_cuda and z.dtype == torch.float32 and z.dim() == 2
                and z.shape[0] > 0 and z.is_contiguous()):
            return None
        if not (isinstance(logpz, torch.Tensor) and logpz.is_cuda and logpz.dtype == torch.float32
                and logpz.device == z.device and logpz.shape == (z.shape[0], 1) and logpz.is_contiguous()):
            return None
        if not (self.training or func._needs_grad(z)):
            return None
        hutchinson = func.training and func.divergence_fn is divergence_approx      # eval mode is always exact
        if route != "force" and not ops.cnf_solve_train_rows_pay(z.shape[0], z.shape[1], hutchinson):
            return None     # the per-evaluation nodes' measured limit ("CNF training: the whole solve")
        e = func._e
        if hutchinson and e is not None and not (
                isinstance(e, torch.Tensor) and e.dtype == torch.float32 and e.device == z.device
                and e.shape == z.shape and e.is_contiguous() and not e.requires_grad):
            return None
        plan = func._plan_for(z)
        steps = fixed_grid_steps(times[0], times[1], self.solver_options)
        if plan is None or not ops.cnf_solve_train_fits(z.shape[0], plan.d, plan.hidden, steps, method, hutchinson):
            return None
        if func.training and func._e is None:       # where, and by the call with which, the composition draws it
            func._e = sample_rademacher_like(z) if func.rademacher else sample_gaussian_like(z)
        kw = func._kernel_args(plan)
        kw.update(t0=times[0], t1=times[1], steps=steps, method=method)
        e = func._e if hutchinson else None
        if not (func._needs_grad(z) or (torch.is_grad_enabled() and logpz.requires_grad)):
            z_t, logp_t = ops.cnf_integrate_train(z, logpz, e, **kw)        # nothing to carry: no tape
            return z_t, logp_t.view(logpz.shape)
        if torch.is_grad_enabled() and any(p.requires_grad for p in ops.param_list(func)):
            kw["image"] = func._training_image(plan)
        image = kw.pop("image")
        return ops._CnfSolveFunction.apply(z, logpz, image, e, kw)

    def forward(self, z, logpz=None, integration_times=None, reverse=False):
        _logpz = torch.zeros(z.shape[0], 1).to(z) if logpz is None else logpz
        if integration_times is None:
            times = self._default_times(z)
        elif isinstance(integration_times, torch.Tensor) and integration_times.requires_grad \
                and torch.is_grad_enabled():
            times = integration_times.to(z)
        else:       # numbers on the host (reading a device tensor waits for the device)
            times = [float(v) for v in torch.as_tensor(integration_times).detach().reshape(-1).tolist()]
        if reverse:
            times = torch.flip(times, [0]) if isinstance(times, torch.Tensor) else times[::-1]

        self.odefunc.before_odeint()        # refresh the evaluation count and the noise
        solved = self._kernel_solve(z, _logpz, times)
        if solved is None:
            solved = self._training_solve(z, _logpz, times)
        if solved is not None:
            z_t, logpz_t = solved
            self.regularization_states = ()
        else:
            if self.training:
                state = (z, _logpz) + tuple(torch.tensor(0).to(z) for _ in range(self.nreg))
                state_t = odeint(self.odefunc, state, times, atol=self.atol, rtol=self.rtol, method=self.solver,
                                 options=self.solver_options)
            else:
                state_t = odeint(self.odefunc, (z, _logpz), times, atol=self.test_atol, rtol=self.test_rtol,
                                 method=self.test_solver, options=self.solver_options)
            if len(times) == 2:
                state_t = tuple(s[1] for s in state_t)
            z_t, logpz_t = state_t[:2]
            self.regularization_states = state_t[2:]
        return (z_t, logpz_t) if logpz is not None else z_t

    def get_regularization_states(self):
        reg_states = self.regularization_states
        self.regularization_states = None
        return reg_states

    def num_evals(self):
        """Function evaluations of the last solve (reads a device word: a host sync)."""
        return self.odefunc._num_evals.item()


class CNFTransform(Transform):
    """A ``CNF`` as a ``Transform`` (an extension: the reference has no such adapter): ``forward`` integrates from 0 to
    T and returns ``(z_T, logabsdet)`` with ``logabsdet = log|det dz_T / dz_0| = -(logp_T - logp_0)``; ``inverse``
    integrates backwards.  With it a CNF sits in ``CompositeTransform`` and ``Flow``."""

    _HIP_AUTOGRAD = True    # delegates: the routes that run with autograd on are the differentiable composition

    def __init__(self, cnf):
        super().__init__()
        self.cnf = cnf

    def _run(self, inputs, context, reverse):
        if context is not None:
            raise ValueError("CNFTransform takes no context")
        outputs, delta = self.cnf(inputs, torch.zeros(inputs.shape[0], 1, dtype=inputs.dtype, device=inputs.device),
                                  reverse=reverse)
        return outputs, -delta.reshape(inputs.shape[0])

    def forward(self, inputs, context=None):
        return self._run(inputs, context, reverse=False)

    def inverse(self, inputs, context=None):
        return self._run(inputs, context, reverse=True)
