"""Transform protocol and composition (API of flowcon/transforms/base.py:10-231).

``forward(inputs, context=None) -> (outputs, logabsdet[N])``; ``inverse`` likewise.
``CompositeTransform`` defers the device error-word read to once per cascade instead of
the reference's host sync inside every spline call.
"""
import numpy as np
import torch
from torch import nn

from flowconductor_amd import ops
from flowconductor_amd.utils import typechecks as check
from flowconductor_amd.ops import InputOutsideDomain, InverseNotAvailable  # noqa: F401 (re-export)


def _guard_missing_backward(fn):
    """forward / inverse of a transform whose kernels have no backward: called with autograd on and trainable own
    parameters, its outputs would carry no gradient and those parameters would silently never train -- fail loudly."""
    import functools

    @functools.wraps(fn)
    def guarded(self, *args, **kwargs):
        self._check_autograd()
        return fn(self, *args, **kwargs)

    guarded._guarded = True
    return guarded


def own_autograd_check(fn):
    """Marks a forward / inverse that calls ``self._check_autograd()`` itself (after checks of its own)."""
    fn._guarded = True
    return fn


def divisor_if_hidden_features(net):
    """sqrt(hidden_features) of a conditioner that exposes it, else 1: only ``hidden_features`` triggers the scaling of the
    unnormalised widths / heights in the sibling-spline layers (coupling.py:438-440, :483-485; autoregressive.py:375-526)."""
    return float(np.sqrt(net.hidden_features)) if hasattr(net, "hidden_features") else 1.0


class Transform(nn.Module):
    """Base class for all transform objects."""

    # True for transforms whose HIP kernels sit behind torch.autograd (or that only delegate to children); every
    # other subclass with trainable parameters of its own refuses to run with autograd on (see the guard above)
    _HIP_AUTOGRAD = False

    def __init_subclass__(cls, **kwargs):
        super().__init_subclass__(**kwargs)
        if not cls.__module__.startswith("flowconductor_amd."):
            return      # a user's own Transform (plain torch ops, differentiable as it is) is none of our business
        for name in ("forward", "inverse"):
            fn = cls.__dict__.get(name)
            if fn is not None and not getattr(fn, "_guarded", False):
                setattr(cls, name, _guard_missing_backward(fn))

    def _check_autograd(self):
        if (not self._HIP_AUTOGRAD and torch.is_grad_enabled()
                and any(p.requires_grad for p in self.parameters(recurse=False))):
            raise RuntimeError(
                "flowconductor_amd: %s has no backward kernel; with autograd on its parameters would silently not "
                "train.  Wrap the call in torch.no_grad() (inference) or freeze the layer with requires_grad_(False)."
                % type(self).__name__)

    def forward(self, inputs, context=None):
        raise NotImplementedError()

    def inverse(self, inputs, context=None):
        raise InverseNotAvailable()

    def train(self, mode=True):
        """Packed-weight caches (kernel-layout copies of parameters) never survive a switch of the training mode:
        see ``ops.invalidate_hip_caches``."""
        ops.invalidate_hip_caches()
        return super().train(mode)

    def _apply(self, fn, *args, **kwargs):
        """``.to()`` / ``.float()`` / ``.cuda()`` replace parameter storage: the memoised fast-path predicates and packed
        images of every module go with them."""
        ops.invalidate_hip_caches()
        return super()._apply(fn, *args, **kwargs)


class CompositeTransform(Transform):
    """Composes several transforms into one, in the order they are given."""

    def __init__(self, transforms):
        super().__init__()
        self._transforms = nn.ModuleList(transforms)

    @staticmethod
    def _cascade(inputs, transforms, context, inverse):
        """base.py:44-60 of the reference.  A transform may offer ``_apply_accumulate(inputs, context, inverse,
        total)`` -> outputs, which adds its logabsdet onto the running total inside its own kernel (one
        element-wise pass over [N] saved per layer); everything else goes through forward / inverse."""
        outputs = inputs
        total_logabsdet = inputs.new_zeros(inputs.shape[0])
        with ops.deferred_errors():
            for t in transforms:
                fused = getattr(t, "_apply_accumulate", None)
                hooked = t._forward_hooks or t._forward_pre_hooks   # the fast path does not go through __call__
                if fused is not None and not hooked and total_logabsdet.dtype == torch.float32:
                    outputs = fused(outputs, context, inverse, total_logabsdet)
                else:
                    outputs, logabsdet = (t.inverse if inverse else t)(outputs, context)
                    total_logabsdet += logabsdet
        return outputs, total_logabsdet

    def forward(self, inputs, context=None):
        return self._cascade(inputs, self._transforms, context, False)

    def inverse(self, inputs, context=None):
        return self._cascade(inputs, self._transforms[::-1], context, True)


class MultiscaleCompositeTransform(Transform):
    """A multiscale composite transform as described in the RealNVP paper (host-level port of base.py:63-212).

    Splits the outputs along ``split_dim`` after every transform but the last, outputs one half (flattened) and passes
    the other half on.  Outputs are always ``[N, D]``; the inverse takes ``[N, D]``."""

    def __init__(self, num_transforms, split_dim=1):
        if not check.is_positive_int(split_dim):
            raise TypeError("Split dimension must be a positive integer.")
        super().__init__()
        self._transforms = nn.ModuleList()
        self._output_shapes = []
        self._num_transforms = num_transforms
        self._split_dim = split_dim

    def add_transform(self, transform, transform_output_shape):
        """Add a transform (exactly ``num_transforms`` times); ``transform_output_shape`` excludes the batch.  Returns
        the input shape of the next transform, or None after the last one."""
        assert len(self._transforms) <= self._num_transforms
        if len(self._transforms) == self._num_transforms:
            raise RuntimeError("Adding more than {} transforms is not allowed.".format(self._num_transforms))
        if (self._split_dim - 1) >= len(transform_output_shape):
            raise ValueError("No split_dim in output shape")
        if transform_output_shape[self._split_dim - 1] < 2:
            raise ValueError("Size of dimension {} must be at least 2.".format(self._split_dim))
        self._transforms.append(transform)
        if len(self._transforms) != self._num_transforms:  # unless last transform
            output_shape = list(transform_output_shape)
            output_shape[self._split_dim - 1] = (output_shape[self._split_dim - 1] + 1) // 2
            output_shape = tuple(output_shape)
            hidden_shape = list(transform_output_shape)
            hidden_shape[self._split_dim - 1] = hidden_shape[self._split_dim - 1] // 2
            hidden_shape = tuple(hidden_shape)
        else:
            output_shape = transform_output_shape
            hidden_shape = None
        self._output_shapes.append(output_shape)
        return hidden_shape

    def forward(self, inputs, context=None):
        if self._split_dim >= inputs.dim():
            raise ValueError("No split_dim in inputs.")
        if self._num_transforms != len(self._transforms):
            raise RuntimeError("Expecting exactly {} transform(s) to be added.".format(self._num_transforms))
        batch_size = inputs.shape[0]
        all_outputs = []
        total_logabsdet = inputs.new_zeros(batch_size)
        hiddens = inputs
        with ops.deferred_errors():
            for i, transform in enumerate(self._transforms):
                transform_outputs, logabsdet = transform(hiddens, context)
                if i < len(self._transforms) - 1:
                    outputs, hiddens = torch.chunk(transform_outputs, chunks=2, dim=self._split_dim)
                    assert outputs.shape[1:] == self._output_shapes[i]
                else:  # no splitting after the last transform
                    outputs = transform_outputs
                all_outputs.append(outputs.reshape(batch_size, -1))
                total_logabsdet += logabsdet
        return torch.cat(all_outputs, dim=-1), total_logabsdet

    def inverse(self, inputs, context=None):
        if inputs.dim() != 2:
            raise ValueError("Expecting NxD inputs")
        if self._num_transforms != len(self._transforms):
            raise RuntimeError("Expecting exactly {} transform(s) to be added.".format(self._num_transforms))
        batch_size = inputs.shape[0]
        split_indices = np.insert(np.cumsum([int(np.prod(shape)) for shape in self._output_shapes]), 0, 0)
        split_inputs = [inputs[:, split_indices[i]:split_indices[i + 1]].reshape(-1, *self._output_shapes[i])
                        for i in range(len(self._output_shapes))]
        total_logabsdet = inputs.new_zeros(batch_size)
        with ops.deferred_errors():
            # no splitting for the last (here first) transform
            hiddens, logabsdet = self._transforms[-1].inverse(split_inputs[-1], context)
            total_logabsdet += logabsdet
            for transform, input_chunk in zip(self._transforms[-2::-1], split_inputs[-2::-1]):
                hiddens, logabsdet = transform.inverse(torch.cat([input_chunk, hiddens], dim=self._split_dim), context)
                total_logabsdet += logabsdet
        return hiddens, total_logabsdet


class InverseTransform(Transform):
    """Creates a transform that is the inverse of a given transform."""

    def __init__(self, transform):
        super().__init__()
        self._transform = transform

    def forward(self, inputs, context=None):
        return self._transform.inverse(inputs, context)

    def inverse(self, inputs, context=None):
        return self._transform(inputs, context)
