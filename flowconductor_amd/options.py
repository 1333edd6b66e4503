"""Explicit switches of the fast paths.

Every dispatch decision in this package (which kernel serves a layer) is a function of the layer, its inputs and
these options -- never of the process environment: a stray environment variable cannot change what a benchmark
times.  The defaults are the product configuration; tools and tests flip a switch for A/B measurements with

    with options.override(fused_final_layer=False):
        flow.log_prob(x)

``override`` restores the previous values on exit (also on an exception) and nests.
"""
import contextlib

__all__ = ["get", "override", "snapshot"]

_DEFAULTS = {
    # conditioner's final Linear evaluated inside the RQ-spline kernel (fc_rq_spline_fused_linear / _general)
    "fused_final_layer": True,
    # conditioner's hidden layers in fc_resnet_hidden (one kernel instead of GEMMs + element-wise passes)
    "fused_hidden": True,
    # shared-parameter Sylvester / Householder / LU maps folded into dense matrices on the matrix cores
    "sylvester_mm": True,
    # autoregressive inverse: "auto" (column-d-only passes where they pay), "force", "off"
    "ar_incremental": "auto",
    # autoregressive inverse: all D passes inside one kernel (fc_made_inverse) where the MADE fits it
    "ar_device_loop": True,
    # fc_rq_spline: pin the LDS-tile kernel instead of the register / wave kernel (FC_RQ_FORCE_TILE)
    "rq_force_tile": False,
    # training: conditioner forward / backward in the HIP kernels (fc_resnet_hidden_backward, fused final-layer
    # backward) instead of PyTorch autograd through library GEMMs
    "fused_training": True,
    # Packed-weight caches (kernel-layout copies of parameters) are keyed on the parameters' version counters and storage
    # pointers; a write THROUGH ``.data`` (``p.data.copy_(ema)``) moves neither.  True: every call re-packs (one
    # fc_pack_fragments launch per layer, ~1 % of a cfg-3 log_prob) -- for code that edits ``.data`` of an eval-mode model
    # and cannot call ``ops.invalidate_hip_caches()`` after it.
    "paranoid_caches": False,
    # UMNN layers: a call that needs a gradient runs fc_umnn + fc_umnn_backward (the integrand recomputed in the kernel)
    # instead of the torch composition.  Off until a default can be moved on measured times.
    "umnn_training": False,
    # BatchNorm in training mode and the scale / shift gradients of ActNorm / PointwiseAffineTransform in the
    # batch-axis reduction kernels (fc_batchnorm_train, fc_batchnorm_train_backward, fc_column_sums) instead of torch
    # reductions; False selects the torch expressions for A/B measurements.
    "batch_statistics_kernels": True,
    # eval-mode continuous normalizing flows: the ODE function in fc_cnf_field (one launch per evaluation) and the
    # fixed-step solves in fc_cnf_integrate (one launch per solve) instead of the torch composition, for batches up to
    # ops.CNF_KERNEL_MAX_LANES lanes; "force" takes them at any batch size (measurements), False never
    "cnf_kernels": True,
    # continuous normalizing flows in training mode, and any evaluation that needs a gradient: one autograd node of
    # fc_cnf_field_train + fc_cnf_field_backward per evaluation of the ODE function instead of the torch composition
    # and its double backward, for batches up to ops.CNF_TRAIN_MAX_LANES lanes; "force" takes them at any batch
    # size (measurements, tests), False never.  Off by default: tests pin the default training route to the composition
    # ("CNF training", has the measured training steps).
    "cnf_training": False,
    # eval-mode continuous normalizing flows under dopri5: the whole adaptive solve in one fc_cnf_dopri5 launch with
    # per-row step control instead of the host loop of odeint over fc_cnf_field, for tolerances of at least 1e-6 and
    # batches up to ops.CNF_DOPRI5_MAX_LANES lanes; "force" takes it at any batch size (measurements, tests), False
    # never.  A row is judged by its own error there (the host loop judges the batch as one system) and a row that
    # cannot finish returns NaN where the host loop raises, so the results differ within the tolerance: off by default
    # ("dopri5 in one launch").
    "cnf_dopri5_kernel": False,
    # a fixed-step solve (euler / midpoint / rk4) of a continuous normalizing flow in training mode, or wherever a
    # gradient is needed, as ONE autograd node: fc_cnf_integrate_train forward, fc_cnf_integrate_backward (a reverse
    # sweep over a tape of stage inputs) backward, instead of a node per evaluation (cnf_training) or the torch
    # composition, for batches up to ops.CNF_TRAIN_MAX_LANES lanes; "force" takes it at any batch size (measurements,
    # tests), False never.  Off by default; a training step measured 1.07x to 1.13x faster than on the per-evaluation
    # route up to that size ("CNF training: the whole solve").
    "cnf_solve_training": False,
    # iResBlock: a forward call that needs a gradient and would compute the EXACT determinant (train() mode with
    # brute_force=True, eval mode with autograd on) runs as one autograd node, fc_iresnet_forward + fc_iresnet_backward
    # (streams recomputed in the kernel), instead of the torch composition and its double backward.  The power-series
    # estimators, inverse(), float64 modules and nets outside ops.iresnet_supported stay on the composition.  Off until
    # a default can be moved on measured times ("iResBlock training").
    "iresblock_training": False,
}

# options that take a few named values only: anything else is a mistake at the call site
_CHOICES = {
    "cnf_training": (False, True, "force"),
    "cnf_dopri5_kernel": (False, True, "force"),
    "cnf_solve_training": (False, True, "force"),
    "iresblock_training": (False, True),
}

_values = dict(_DEFAULTS)


def get(name):
    return _values[name]


def snapshot():
    """Current values (bench.py records them in its JSON line)."""
    return dict(_values)


@contextlib.contextmanager
def override(**kw):
    unknown = set(kw) - set(_DEFAULTS)
    if unknown:
        raise KeyError("unknown option(s): %s" % ", ".join(sorted(unknown)))
    for name, value in kw.items():
        if name in _CHOICES and not any(value is choice or (isinstance(value, str) and value == choice)
                                        for choice in _CHOICES[name]):
            raise ValueError("option %s takes one of %r, got %r" % (name, _CHOICES[name], value))
    saved = {k: _values[k] for k in kw}
    _values.update(kw)
    try:
        yield
    finally:
        _values.update(saved)
