"""Unconstrained Monotonic Neural Networks (Wehenkel & Louppe, NeurIPS 2019): the monotone map

    z = h_0 + int_0^x f(t, h) dt,      f = ELU(MLP(t, h)) + 1 > 0,      dz/dx = f(x, h)

behind ``MaskedUMNNAutoregressiveTransform``, ``UMNNCouplingTransform`` and ``ConditionalUMNNTransform`` (API and
``state_dict`` keys of flowcon/transforms/UMNN/MonotonicNormalizer.py).  The reference hands the integral to the
third-party ``UMNN`` package; here the package owns it: Clenshaw-Curtis quadrature on the nodes cos(i pi / nb_steps),

    z = h_0 + (x / 2) sum_i w_i f((x / 2) (s_i + 1), h),      weights from ``cc_weights`` (float64, interpolatory),

with Leibniz' rule for the gradient (d/dx = f(x, h); the parameters and ``h`` differentiate under the integral sign).
``fc_umnn`` (csrc/fc_umnn.hip) runs both directions on the matrix cores for 2-D float32 device tensors in inference;
with ``options`` ``umnn_training`` a call that needs a gradient runs the same launch under ``ops.umnn_autograd``, whose
backward is ``fc_umnn_backward`` (csrc/fc_umnn_backward.hip: the integrand recomputed in the kernel).  Everything else
takes the torch composition of this file; its inverse under autograd re-attaches the root of the search by the
implicit-function theorem, so ``x`` carries its gradient with respect to ``z``, ``h`` and the parameters.
"""
import numpy as np
import torch
from torch import nn

from flowconductor_amd import ops, options

BRACKET = 20.0          # the inverse searches [-BRACKET, BRACKET] (MonotonicNormalizer.py:69-70)
BISECTION_STEPS = 25    # (:73)


def cc_weights(nb_steps):
    """``(nodes, weights)``, float64 arrays of ``nb_steps + 1`` entries: the Clenshaw-Curtis rule on [-1, 1] with nodes
    ``cos(i pi / nb_steps)``.  The weights are the interpolatory ones (the integral of the Lagrange polynomials on these
    nodes), exact for polynomials up to degree ``nb_steps``, from their closed cosine series

        w_i = c_i / n (1 - sum_{j=1}^{n div 2} b_j / (4 j^2 - 1) cos(2 j i pi / n)),   c_i = 1 at the ends, else 2,
                                                                                       b_j = 1 for 2 j = n, else 2.

    The kernel, the torch composition, the fixtures and the tests all take their rule from here."""
    n = int(nb_steps)
    if n < 1:
        raise ValueError("cc_weights: nb_steps must be >= 1")
    i = np.arange(n + 1, dtype=np.float64)
    nodes = np.cos(i * np.pi / n)
    nodes[np.abs(nodes) < 1e-16] = 0.0          # the middle node of an even rule
    series = np.ones(n + 1, dtype=np.float64)
    for j in range(1, n // 2 + 1):
        b = 1.0 if 2 * j == n else 2.0
        series -= b / (4.0 * j * j - 1.0) * np.cos(2.0 * j * i * np.pi / n)
    c = np.full(n + 1, 2.0)
    c[0] = c[-1] = 1.0
    weights = c / n * series
    weights = 0.5 * (weights + weights[::-1])    # symmetric to the last bit
    return nodes, weights


class ELUPlus(nn.Module):
    """ELU(x) + 1: positive everywhere."""

    def __init__(self):
        super().__init__()
        self.elu = nn.ELU()

    def forward(self, x):
        return self.elu(x) + 1.0


class IntegrandNet(nn.Module):
    """f(t, h): Linear / ReLU over ``[1 + cond_in] + hidden``, a final Linear to 1, ELU + 1 (``net.{0,2,4,..}``)."""

    def __init__(self, hidden, cond_in):
        super().__init__()
        widths = [1 + cond_in] + list(hidden)
        layers = []
        for a, b in zip(widths, widths[1:]):
            layers += [nn.Linear(a, b), nn.ReLU()]
        layers += [nn.Linear(widths[-1], 1), ELUPlus()]
        self.net = nn.Sequential(*layers)

    def forward(self, x, h):
        """``x`` [B, D], ``h`` [B, C * D] laid out [C][D] (embedding value c of feature d at c * D + d) -> f [B, D]."""
        batch, d = x.shape
        rows = torch.cat((x.unsqueeze(1), h.reshape(batch, -1, d)), dim=1).transpose(1, 2)     # [B, D, 1 + C]
        return self.net(rows).squeeze(-1)

    def linears(self):
        """The Linear layers in order, or None when ``net`` is not the plain Linear / ReLU ... Linear / ELUPlus stack
        (a user may have swapped a layer: then only the torch composition applies)."""
        mods = list(self.net)
        if len(mods) < 4 or len(mods) % 2 != 0 or type(mods[-1]) is not ELUPlus:
            return None
        lins = mods[0::2]
        acts = mods[1:-1:2]
        if not all(type(m) is nn.Linear and m.bias is not None for m in lins):
            return None
        if not all(type(m) is nn.ReLU for m in acts):
            return None
        return lins


class MonotonicNormalizer(nn.Module):
    """``forward(x, h) -> (z, jac)`` with ``z0 = h[:, :, 0]`` and every entry of ``h`` fed to the integrand;
    ``inverse_transform(z, h) -> x``.  ``"CC"`` and ``"CCParallel"`` are the same arithmetic here."""

    def __init__(self, integrand_net, cond_size, nb_steps=20, solver="CC"):
        super().__init__()
        if type(integrand_net) is list:
            self.integrand_net = IntegrandNet(integrand_net, cond_size)
        else:
            self.integrand_net = integrand_net
        self.solver = solver
        self.nb_steps = nb_steps
        self.cond_size = cond_size

    # ---- the rule ---------------------------------------------------------------------------------------------------
    def _rule(self, like):
        def build():
            nodes, weights = cc_weights(self.nb_steps)
            return (torch.as_tensor(nodes).to(device=like.device, dtype=like.dtype),
                    torch.as_tensor(weights).to(device=like.device, dtype=like.dtype))
        return ops.memo(self, "umnn_rule", (self.nb_steps, like.device, like.dtype), build)

    # ---- torch composition ------------------------------------------------------------------------------------------
    @staticmethod
    def _flat(h, rows):
        return h.permute(0, 2, 1).reshape(rows, -1)

    def _integral(self, x, hflat):
        """(x / 2) sum_i w_i f((x / 2)(s_i + 1), h) with the limits as given (no gradient rule of its own)."""
        nodes, weights = self._rule(x)
        n, d = x.shape
        pts = nodes.numel()
        half = x / 2
        t = half.unsqueeze(1) * (nodes + 1).view(1, pts, 1)                               # [N, S + 1, D]
        hrep = hflat.unsqueeze(1).expand(n, pts, hflat.shape[1]).reshape(n * pts, -1)
        f = self.integrand_net(t.reshape(n * pts, d), hrep).view(n, pts, d)
        return half * (f * weights.view(1, pts, 1)).sum(dim=1)

    def _compose(self, x, h):
        """(z, jac) in plain torch ops.  Leibniz: the gradient with respect to ``x`` is ``jac``; ``h`` and the integrand's
        parameters differentiate the quadrature with its limits held constant."""
        hflat = self._flat(h, x.shape[0])
        jac = self.integrand_net(x, hflat)
        xd = x.detach()
        z = h[:, :, 0] + self._integral(xd, hflat)
        if x.requires_grad and torch.is_grad_enabled():
            z = z + (x - xd) * jac.detach()
        return z, jac

    def _compose_inverse(self, z, h):
        """The reference's search: ``BISECTION_STEPS`` halvings of [-BRACKET, BRACKET]; a target outside the range of
        the map ends within BRACKET / 2^(steps - 1) of the bracket's end."""
        with torch.no_grad():
            hd = h.detach()
            zd = z.detach()
            hi = torch.full_like(zd, BRACKET)
            lo = -hi
            for _ in range(BISECTION_STEPS):
                mid = (hi + lo) / 2
                above = self._compose(mid, hd)[0] > zd
                hi = torch.where(above, mid, hi)
                lo = torch.where(above, lo, mid)
            return (hi + lo) / 2

    def _needs_grad(self, x, h):
        return torch.is_grad_enabled() and (x.requires_grad or h.requires_grad
                                            or any(p.requires_grad for p in self.integrand_net.parameters()))

    def _attached_inverse(self, z, h):
        """The search's root; under autograd with the implicit-function gradient attached and the value unchanged:
        x = x_d + (r - r.detach()) / J, r = z - F(x_d) with x_d a constant, so dx = (dz - dF|_x) / J."""
        xd = self._compose_inverse(z, h)
        if not self._needs_grad(z, h):
            return xd
        image, jac = self._compose(xd, h)
        r = z - image
        return xd + (r - r.detach()) / jac.detach()

    # ---- the kernel -------------------------------------------------------------------------------------------------
    def _hip_ok(self, x, h, training=False):
        """Whether the kernel takes the call: in inference (``training`` False: nothing needs a gradient), or -- with
        ``options`` ``umnn_training`` -- a call that does need one, under the same structural conditions and with the
        integrand's parameters float32 on the inputs' device."""
        if not (x.dim() == 2 and h.dim() == 3 and x.is_cuda and x.dtype == torch.float32 and h.dtype == torch.float32
                and h.device == x.device and h.shape[:2] == x.shape and h.shape[2] == self.cond_size
                and x.numel() > 0 and self.solver in ("CC", "CCParallel")):
            return False
        net = self.integrand_net
        if self._needs_grad(x, h) != training:
            return False
        if training and not (options.get("umnn_training")
                             and all(p.dtype == torch.float32 and p.device == x.device for p in net.parameters())):
            return False

        def structure_ok():
            lins = net.linears() if type(net) is IntegrandNet else None
            if lins is None:
                return False
            widths = [lin.out_features for lin in lins[:-1]]
            return (lins[0].in_features == 1 + self.cond_size and lins[-1].out_features == 1
                    and all(a.out_features == b.in_features for a, b in zip(lins, lins[1:]))
                    and all(lin.weight.dtype == torch.float32 for lin in lins)
                    and ops.umnn_fits(self.cond_size, widths, self.nb_steps))

        key = (self.cond_size, self.nb_steps, tuple(id(m) for m in getattr(net, "net", ())))
        return ops.static_memo(self, "umnn_hip_ok", key, structure_ok) and not ops.has_hooks(net)

    def _hip(self, x, h, inverse, lad_mode=ops.LAD_STORE):
        image = ops.umnn_image(self, self.integrand_net.linears(), self.nb_steps, x.device)
        return ops.umnn(x, h, image, self.cond_size, self.nb_steps, inverse=inverse, lad_mode=lad_mode)

    def _hip_autograd(self, x, h, inverse):
        return ops.umnn_autograd(x, h, self.integrand_net.linears(), self, self.cond_size, self.nb_steps, inverse=inverse)

    # ---- public -----------------------------------------------------------------------------------------------------
    def forward(self, x, h, context=None):
        if self.solver not in ("CC", "CCParallel"):
            return None
        if self._hip_ok(x, h):
            z, _, jac = self._hip(x, h, False)
            return z, jac
        if self._hip_ok(x, h, training=True):
            z, _, jac = self._hip_autograd(x, h, False)
            return z, jac
        return self._compose(x, h)

    def inverse_transform(self, z, h, context=None):
        if self._hip_ok(z, h):
            return self._hip(z, h, True)[0]
        if self._hip_ok(z, h, training=True):
            return self._hip_autograd(z, h, True)[0]
        return self._attached_inverse(z, h)

    def apply_with_logabsdet(self, inputs, h, inverse=False):
        """What the three transform classes call: ``(outputs, logabsdet [rows])``, logabsdet = +-sum_d log f(x, h).
        One ``fc_umnn`` launch where the kernel takes the call (and one ``fc_umnn_backward`` in its backward pass)."""
        if self._hip_ok(inputs, h):
            out, lad, _ = self._hip(inputs, h, inverse)
            return out, lad
        if self._hip_ok(inputs, h, training=True):
            out, lad, _ = self._hip_autograd(inputs, h, inverse)
            return out, lad
        if not inverse:
            z, jac = self._compose(inputs, h)
            return z, jac.log().sum(1)
        x = self._attached_inverse(inputs, h)
        return x, -self._compose(x, h)[1].log().sum(1)
