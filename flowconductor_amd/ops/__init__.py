"""Functional host wrappers over the HIP kernels (tensor in -> tensor out).

The ``Transform`` modules in ``flowconductor_amd.transforms`` call these; they allocate the
outputs with torch, pass raw device pointers + the current HIP stream through the C ABI and
turn the device error word into the reference's Python exceptions.

One module per kernel family (DESIGN.md 1 has the table); this file only re-exports their names, so that every
call site says ``from flowconductor_amd import ops`` and ``ops.<name>``.
"""
from ._core import (  # noqa: F401
    InputOutsideDomain, InverseNotAvailable, KernelTimer, LAD_ACCUMULATE, LAD_ACCUMULATE_NEG, LAD_STORE, LAD_STORE_NEG,
    MSG_CHOLESKY_FAILED, MSG_DIAGONAL_NONPOSITIVE, MSG_NOT_LOWER_TRIANGULAR, MSG_NOT_POSITIVE_DEFINITE, MSG_NOT_SQUARE,
    MSG_NOT_SYMMETRIC, _aligned16, _as_cols, _call, _check_now, _err_word, _finish, _flag_for, _flags,
    _logabsdet_target, _pad_to, _prep_2d, _raise_for, _state, buffer_list, cache_key, cached, capture_mode,
    check_errors, deferred_errors, device_plan, drop_param_list, has_hooks, invalidate_hip_caches, memo, module_list,
    param_list, rq_param_count, static_memo, structure_key)
from .rq import (  # noqa: F401
    DEFAULT_MIN_BIN_HEIGHT, DEFAULT_MIN_BIN_WIDTH, DEFAULT_MIN_DERIVATIVE, _RQSplineFunction, _inverse_through_forward,
    _rq_config, rq_spline, rq_spline_autograd, rq_spline_backward)
from .packing import (  # noqa: F401
    DevicePack, FRAG_ELEMS, FRAG_KSTEP, FUSED_BINS, FUSED_DT, FUSED_HIDDEN, FUSED_ROWS, PACK_FINAL, PACK_FINAL_T,
    PACK_HIDDEN, PACK_HIDDEN_T, PACK_HIDDEN_T0, _a_fragments, _add_hidden_jobs, _bias_accumulator_order, _exact_pow2,
    _hb_perm, _hidden_image, _hidden_image_fragments, _hidden_layer_fragments, _hidden_linears, _made_pass_prefix,
    _pow2_scale, device_pack_affine_coupling, device_pack_final_layer, device_pack_made_affine,
    device_pack_resnet_hidden_backward, device_pack_resnet_hidden_forward, householder_matrix, pack_final_layer,
    pack_final_layer_general, pack_final_layer_transposed, pack_made_inverse, pack_made_inverse_context,
    pack_resnet_hidden, pack_resnet_hidden_backward, pack_resnet_hidden_wide, pack_sylvester)
from .fused_rq import (  # noqa: F401
    GENERAL_BINS, GENERAL_HIDDEN, fused_backward_supported, fused_general_supported, fused_linear_supported,
    general_hidden_width, rq_fused_linear_backward, rq_spline_fused_general, rq_spline_fused_linear)
from .affine import (  # noqa: F401
    AFFINE_ADDITIVE, AFFINE_MAF_SOFTPLUS, AFFINE_SCALE_GIVEN, AFFINE_SCALE_SOFTPLUS, AFFINE_SHIFT_TANH2,
    AFFINE_SIGMOID_PLUS2, AFFINE_SOFTPLUS_CLAMP3, _AffineFunction, _StdNormalLogProbFunction, _affine_coupling_nograd,
    _standard_normal_log_prob_nograd, affine_coupling, standard_normal_log_prob)
from .conditioner import (  # noqa: F401
    ACT_ELU, ACT_LEAKY_RELU, ACT_RELU, ACT_SIGMOID, ACT_SILU, ACT_TANH, CONTEXT_ADDITIVE, CONTEXT_GLU, HIDDEN_BWD_ROWS,
    HIDDEN_ROWS, MADE_AFFINE, MADE_RQ, MADE_SOS, MADE_SPLINE, WIDE_ROWS, activation_code, affine_coupling_resnet,
    affine_tail_activation, affine_tail_fits, made_inverse, made_inverse_context_fits, made_inverse_form_fits,
    made_inverse_param_limit, made_inverse_row_limit, resnet_hidden, resnet_hidden_backward, resnet_hidden_packed,
    resnet_hidden_wide)
from .mog import (  # noqa: F401
    MOG_MAX_COMPONENTS, _MoGLogProbFunction, _mog_log_prob_nograd, _mog_operands, made_mog_sample, mog_log_prob,
    mog_log_prob_backward)
from .pointwise import (  # noqa: F401
    EW_CAUCHY_CDF, EW_EXP, EW_EXTENDED_SOFTPLUS, EW_GLU, EW_LEAKY_RELU, EW_LOGTANH, EW_SIGMOID, EW_SOFTPLUS, EW_TANH,
    _ElementwiseFunction, _PermuteFunction, _PointwiseAffineFunction, _item_vector, _permute_nograd, batchnorm_eval,
    elementwise, elementwise_autograd, elementwise_expression, permute, pointwise_affine, pointwise_affine_autograd)
from .rowwave import (  # noqa: F401
    HDH_MAX_REFLECTIONS, LINEAR_DENSE, LINEAR_DENSE_SHIFTED, LINEAR_LU_FORWARD, LINEAR_LU_INVERSE, MAX_ROW_FEATURES,
    PER_SAMPLE_DENSE, PER_SAMPLE_DENSE_T, PER_SAMPLE_LU_FORWARD, PER_SAMPLE_LU_INVERSE, SYLVESTER_MM_ROWS,
    _DenseLinearFunction, _HDHLinearFunction, _HouseholderFunction, _LULinearFunction, _PlanarFunction, _SylvesterFunction,
    _UpperLinearFunction, _hdh_operands, _householder_backward, _param, _rows, dense_linear_autograd, dense_mm, hdh_linear,
    hdh_linear_autograd, householder, householder_autograd, linear, linear_per_sample, lu_linear_autograd, planar,
    planar_autograd, sylvester, sylvester_autograd, sylvester_mm, sylvester_mm_supported, upper_linear,
    upper_linear_autograd)
from .rowwave import (  # noqa: F401
    SYLVESTER_INVERSE_MAX_FEATURES, sylvester_inverse, sylvester_inverse_supported)
from .rowwave import (  # noqa: F401
    _HouseholderPerSampleFunction, _LinearPerSampleFunction, _PlanarPerSampleFunction, linear_per_sample_autograd)
from .rownorm import (  # noqa: F401
    _RadialFunction, _UnitVectorFunction, _radial_inverse_through_forward, radial, radial_autograd, unit_vector,
    unit_vector_autograd)
from .discrete import (  # noqa: F401
    _BernoulliLogProbFunction, bernoulli_log_prob, bernoulli_sample, box_log_prob)
from .colstats import (  # noqa: F401
    COLSTATS_MAX_PARTIALS, COLSTATS_ROWS_PER_ITERATION, _BatchNormTrainFunction, batch_statistics_route,
    batch_statistics_supported, batchnorm_train, batchnorm_train_autograd, column_sums)
from .sigmoids import (  # noqa: F401
    _DeepSigmoidFunction, _SoSFunction, deep_sigmoid, deep_sigmoid_autograd, deep_sigmoid_bound, deep_sigmoid_fits,
    sum_of_sigmoids, sum_of_sigmoids_autograd)
from .splines import (  # noqa: F401
    SPLINE_CUBIC, SPLINE_LINEAR, SPLINE_QUADRATIC, _PiecewiseSplineFunction, _spline_config, piecewise_spline,
    piecewise_spline_autograd, piecewise_spline_backward_supported, spline_multiplier)
from .spd import (  # noqa: F401
    SPD_MAX_DIM, _CholeskyOuterFunction, _DiagExtractFunction, _DiagReplaceFunction, _TrilPackFunction,
    _cholesky_outer_nograd, _diag_extract_nograd, _diag_replace_nograd, _matrices, _tril_pack_nograd, cholesky,
    cholesky_outer, fill_triangular, matrix_diagonal, matrix_replace_diagonal, tril_gather)
from .image import (  # noqa: F401
    CONV1X1_MAX_CHANNELS, _Conv1x1Function, _SqueezeFunction, _conv1x1_nograd, _conv1x1_operand, _squeeze_nograd,
    conv1x1, squeeze)
from .iresnet import (  # noqa: F401
    IRES_ACT_CLIPSWISH, IRES_ACT_CSIN, IRES_ACT_ELU, IRES_ACT_LEAKY_LSWISH, IRES_ACT_LIPSWISH, IRES_ACT_RELU,
    IRES_ACT_SIN, IRES_ACT_SWISH, IRES_ACT_TANH, IRES_CONCAT_ACTS, IRES_MAX_DEPTH, IRES_MAX_DIM, IRES_MAX_WIDTH,
    IRES_DOUBLE_BACKWARD_MSG, _IResNetFunction, _ires_operands, _pad4, iresnet_autograd, iresnet_backward, iresnet_forward,
    iresnet_image_floats, iresnet_inverse, iresnet_supported)
from .cnf import (  # noqa: F401
    CNF_ACT_ELU, CNF_ACT_IDENTITY, CNF_ACT_RELU, CNF_ACT_SOFTPLUS, CNF_ACT_SQUARE, CNF_ACT_SWISH, CNF_ACT_TANH,
    CNF_EULER, CNF_KERNEL_MAX_LANES, CNF_LAYER_CONCAT, CNF_LAYER_CONCATSQUASH, CNF_LAYER_CONCAT_V2, CNF_LAYER_IGNORE, CNF_LAYER_SQUASH,
    CNF_MAX_DIM, CNF_MAX_HIDDEN_LAYERS, CNF_MAX_WIDTH, CNF_METHODS, CNF_MIDPOINT, CNF_RK4, CNF_STAGES, _cnf_operands,
    _cnf_pad4, cnf_field, cnf_group_lanes, cnf_image_floats, cnf_integrate, cnf_rows_pay, cnf_supported)
from .cnf import (  # noqa: F401
    CNF_DOPRI5_MAX_ATTEMPTS, CNF_DOPRI5_MAX_LANES, CNF_DOPRI5_MIN_TOL, cnf_dopri5, cnf_dopri5_attempts, cnf_dopri5_fits,
    cnf_dopri5_rows_pay)
from .cnf import (  # noqa: F401
    CNF_BACKWARD_MAX_BLOCKS, CNF_DOUBLE_BACKWARD_MSG, CNF_TRAIN_MAX_HIDDEN_LAYERS, CNF_TRAIN_MAX_LANES, _CnfFieldFunction, cnf_backward_rows,
    cnf_field_backward, cnf_field_train, cnf_train_lanes, cnf_train_rows_pay, cnf_train_supported)
from .cnf import (  # noqa: F401
    CNF_SOLVE_DOUBLE_BACKWARD_MSG, CNF_SOLVE_TRAIN_MAX_TAPE_BYTES, _CnfSolveFunction, cnf_integrate_backward,
    cnf_integrate_train, cnf_solve_train_fits, cnf_solve_train_rows_pay)
from .umnn import (  # noqa: F401
    UMNN_DOUBLE_BACKWARD_MSG, UMNN_MAX_COND, UMNN_MAX_HIDDEN_LAYERS, UMNN_MAX_STEPS, UMNN_MAX_WIDTH, UMNN_POINTS,
    _UMNNFunction, pack_umnn, pack_umnn_backward, umnn, umnn_autograd, umnn_backward, umnn_backward_image, umnn_fits,
    umnn_grad_floats, umnn_image, umnn_image_floats, umnn_unpack_grads)
