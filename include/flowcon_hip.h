/* flowcon_hip.h -- C ABI of libflowcon_hip.so: MI355X (gfx950) bijector kernels.
 *
 * Every entry point
 *   - takes raw DEVICE pointers (f32 unless stated) and plain sizes; no torch types,
 *   - allocates nothing, is asynchronous on `stream` (a hipStream_t passed as void*),
 *   - returns a hipError_t as int (0 == hipSuccess),
 *   - never mutates its inputs (x may alias y where stated).
 * The reference (FlowConductor, pure Python on ATen) has no FFI; each function below names
 * the reference op sequence it stands in for (file:line under the reference tree).
 * INTEGRATION.md shows the ctypes binding a maintainer would add on the reference side.
 *
 * Common conventions
 *   x, y        [n, d] row-major; transformed columns are `cols[0..d_t)` (int32) or, when
 *               cols == NULL, d_t == d and dim j is column j.  Columns not listed in `cols`
 *               are copied x -> y unchanged (coupling identity half, coupling.py:96-98).
 *   params      per-sample parameters [n, rowlen]; shared_params != 0 means a single
 *               [rowlen] row used for the whole batch (nonlinearities.py:246-247).
 *   logabsdet   [n] or NULL. lad_mode: 0 store, 1 accumulate (+=), 2 store negated,
 *               3 accumulate negated.
 *   err_flag    device uint32 word or NULL; kernels OR in FC_ERR_* bits, the host reads it
 *               to raise the reference's exceptions (transforms/base.py:10-19).
 */
#ifndef FLOWCON_HIP_H_
#define FLOWCON_HIP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FC_ERR_OUTSIDE_DOMAIN 1u /* InputOutsideDomain, splines/rational_quadratic.py:81-82 */
#define FC_ERR_DISCRIMINANT 2u   /* assert (discriminant >= 0).all(), rational_quadratic.py:142 */
#define FC_ERR_NONFINITE 4u
/* flows on SPD matrices (transforms/matrix/cholesky.py:37-49; the checks run only under checkargs except the last) */
#define FC_ERR_NOT_LOWER_TRIANGULAR 8u   /* a strictly-upper entry of CholeskyOuterProduct's input is not 0 */
#define FC_ERR_DIAGONAL_NONPOSITIVE 16u  /* a diagonal entry of CholeskyOuterProduct's input is <= 0 */
#define FC_ERR_NOT_SYMMETRIC 32u         /* inverse input != its transpose */
#define FC_ERR_NOT_POSITIVE_DEFINITE 64u /* a Cholesky pivot <= 0 (stands in for the torch.linalg.eig test) */
#define FC_ERR_CHOLESKY_FAILED 128u      /* a Cholesky pivot <= 0 without checkargs (torch.linalg.LinAlgError) */

/* ABI version of this header; fc_abi_version() must return it.  Bumped whenever an exported entry, an accepted enum value
 * or a documented behaviour changes (2: round 4 -- fc_rq_fused_linear_backward is one launch, fc_comm_* entries of round 3,
 * FC_AFFINE_MAF_SOFTPLUS / FC_RQ_STREAMED_WEIGHTS; 3: the SPD-matrix entries fc_tril_pack, fc_matrix_diag,
 * fc_cholesky_outer(_backward), fc_cholesky and their FC_ERR_* bits).  The image-flow entries fc_squeeze / fc_conv1x1
 * were added under version 3: they change no existing entry, and a library without them fails to bind by name; the same
 * holds for the invertible-residual-block entries fc_iresnet_forward / fc_iresnet_inverse, for the conditional
 * device loop fc_made_inverse_context and for the mixture-of-Gaussians entries fc_mog_log_prob(_backward) /
 * fc_made_mog_sample(_context), for the Householder-diagonal-Householder entries fc_hdh_linear(_backward) and for the
 * deep-sigmoidal-flow entries fc_deep_sigmoid / fc_deep_sigmoid_backward(_rows), for the monotonic-integral entries
 * fc_umnn and fc_umnn_backward(_workspace), for the row-norm entries fc_radial(_backward) / fc_unit_vector(_backward) and for the discrete / uniform base
 * entries fc_bernoulli_log_prob(_backward), fc_bernoulli_sample and fc_box_log_prob, and for the batch-statistics entries
 * fc_batchnorm_train(_backward), fc_column_sums and fc_colstats_workspace), and for the device loops of the
 * sum-of-sigmoids and sibling-spline layers fc_made_inverse_sos / fc_made_inverse_spline, and for the Sylvester
 * back substitution fc_sylvester_inverse, and for the per-sample backward entries fc_linear_per_sample_backward,
 * fc_householder_backward_per_sample and fc_planar_backward_per_sample, and for the continuous-normalizing-flow
 * entries fc_cnf_field / fc_cnf_integrate / fc_cnf_dopri5). */
#define FC_ABI_VERSION 3

int fc_abi_version(void);

/* ---- rational-quadratic spline ------------------------------------------------------- */
#define FC_RQ_ACCUMULATE_LOGABSDET 1 /* fc_rq_spline_fused_linear: logabsdet[n] += sum (the caller's running
                                       total of CompositeTransform._cascade, transforms/base.py:45-52) */
#define FC_RQ_FORCE_TILE 2 /* fc_rq_spline: always the LDS-tile kernel, never the register / wave kernel (A/B
                              measurements; the results are the same) */
#define FC_RQ_RAW_WEIGHTS 4 /* fc_rq_spline_fused_linear: w_pad / bias_pad are the final nn.Linear's tensors as they
                               are, [d_t * 23, 64] and [d_t * 23] (no padding rows; same results) */
#define FC_RQ_STREAMED_WEIGHTS 8 /* fc_rq_spline_fused_general: always the streamed-weight kernel, never the
                                    resident-weight instances of fc_rq_fused4 (A/B measurements and tests) */

typedef struct fc_rq_config {
  int32_t num_bins;       /* K */
  int32_t tails;          /* 0: none, 1: "linear" (rational_quadratic.py:32-42) */
  int32_t inverse;        /* 0 forward, 1 inverse */
  int32_t flags;          /* FC_RQ_* bits */
  float left, right, bottom, top; /* linear tails: -B, B, -B, B */
  double min_bin_width, min_bin_height, min_derivative; /* python floats of the reference */
  float wh_divisor;       /* sqrt(hidden_features) or 1 (coupling.py:554-559) */
  float softplus_beta;    /* 1, or ln2/(1-min_derivative) (rational_quadratic.py:100-103) */
  float tail_constant;    /* (float)log(exp(1-min_derivative)-1) (rational_quadratic.py:34) */
  float reserved2;
} fc_rq_config;

/* Replaces unconstrained_rational_quadratic_spline / rational_quadratic_spline
 * (splines/rational_quadratic.py:13-181) together with the reshape + in-place scaling +
 * sum_except_batch of PiecewiseRationalQuadraticCouplingTransform (coupling.py:279-293,
 * 549-582), the masked AR variant (autoregressive/autoregressive.py:583-621) and
 * PiecewiseRationalQuadraticCDF (nonlinearities.py:429-487).
 * params row layout per transformed dim: [K widths | K heights | K-1 (linear tails) or K+1
 * derivatives]; rowlen = d_t * (3K -/+ 1). */
int fc_rq_spline(const float* x, float* y, const float* params, const int32_t* cols,
                 float* logabsdet, uint32_t* err_flag, int64_t n, int32_t d, int32_t d_t,
                 int32_t shared_params, int32_t lad_mode, const fc_rq_config* cfg, void* stream);

/* Final conditioner layer fused with the RQ-spline coupling bijector: the [n, d_t*(3K-1)] parameter
 * tensor  h @ W^T + b  (flowcon/nn/nets/resnet.py:91,99 final_layer) is produced on the matrix cores (three-term
 * scaled f16 splits, f32-GEMM accuracy) straight into the registers of the lanes that evaluate the spline
 * (coupling.py:279-293, 549-582); it never reaches HBM.  cfg->flags: FC_RQ_ACCUMULATE_LOGABSDET, FC_RQ_RAW_WEIGHTS.  Specialised: hidden == 64, 1 <= d_t <= 32, K == 8, linear tails, d <= 128,
 * n % 32 == 0 (callers route other shapes / the leftover rows through fc_rq_spline).
 *   h        [n, 64]  last hidden activation of the conditioner (input of its final Linear)
 *   w_pad    [dp*24, 64]  the weight, zero-padded from 23 to 24 rows per dim (row j*24+i = W row j*23+i, i < 23)
 *                         and from d_t to dp = ceil(d_t / 4) * 4 dims
 *   bias_pad [dp*24]      bias with the same padding */
int fc_rq_spline_fused_linear(const float* x, float* y, const float* h, const float* w_pad,
                              const float* bias_pad, const int32_t* cols, float* logabsdet,
                              uint32_t* err_flag, int64_t n, int32_t d, int32_t d_t, int32_t hidden,
                              const fc_rq_config* cfg, void* stream);

/* The same fusion for general layer shapes -- the reference's DEFAULT coupling layer has num_bins = 10
 * (coupling.py:507), any hidden_features (nn/nets/resnet.py:62) and allows tails = None (coupling.py:543-547):
 * K = 4..16, cfg->tails 0 or 1, hidden in {64, 128, 256} (narrower activations zero-padded), 1 <= d_t <= 32, d <= 128,
 * n % 32 == 0.  The weights are not resident in registers here: the host packs them once per parameter version into
 * matrix-core fragment order (scaled by a power of two per group of 4 dims, split into two f16 pieces) and every wave
 * streams the fragments of its dims from L2.
 *   h         [n, hidden]
 *   w_frag    f16 [groups][hidden/32][T][2][64][8], groups = ceil(d_t/4), T = ceil(P/4), P = 3K -/+ 1: fragment
 *             (group, k-step, tile t, piece hi/lo): lane l holds 2^S W[dim 4 group + ((l&15)>>2)][param 4t + (l&3)]
 *             [k = 32 kstep + 8 (l>>4) + j], j < 8
 *   w_unscale f32 [groups] = 2^-S;  bias_pad f32 [groups][4][4T]
 * cfg->flags: FC_RQ_ACCUMULATE_LOGABSDET, FC_RQ_STREAMED_WEIGHTS.  Without tails, inputs outside [left, right] set
 * FC_ERR_OUTSIDE_DOMAIN.  hidden == 64 with K = 4..7, 9..11 (linear tails) or 4..10 (no tails) -- K = 10 is the
 * reference's default num_bins -- runs with both weight pieces resident in registers and a hand-scheduled evaluation
 * (fc_rq_fused4_body.h), same results contract. */
int fc_rq_spline_fused_general(const float* x, float* y, const float* h, const void* w_frag,
                               const float* w_unscale, const float* bias_pad, const int32_t* cols,
                               float* logabsdet, uint32_t* err_flag, int64_t n, int32_t d, int32_t d_t,
                               int32_t hidden, const fc_rq_config* cfg, void* stream);

/* Backward of the fused layer above (forward direction, hidden == 64): what torch.autograd yields for the reference's
 * final Linear + spline (nn/nets/resnet.py:99 + rational_quadratic.py:13-181; the reference trains through them,
 * examples/toy_2d.py:57-68) WITHOUT the [n, d_t P] parameter / parameter-gradient tensors: the parameters are recomputed
 * on the matrix cores from the saved h, the closed-form spline backward runs on them in registers.
 * One launch (role must be FC_RQ_BACKWARD_ONE_LAUNCH; ABI 1 ran two launches, roles 0 "dx" and 1 "dw", each recomputing G):
 *   grad_x [n, d] (= grad_y on the other columns), grad_h [n, 64] = W^T G              (deterministic)
 *   grad_bias_pad [groups][4][4T] += sum_n G,  grad_w_pad [groups][4][4T][64] += sum_n G (x) h
 *                                              (both accumulate with float atomics: zero them first)
 * grad_x / grad_h must not alias grad_y (they serve as scratch between the kernel's sweeps over groups of 16 dims).
 * w_frag / w_unscale / bias_pad as for fc_rq_spline_fused_general with hidden == 64; wt_frag f16
 * [groups][4 hidden tiles][KK][2][64][8], KK = ceil(4T / 8): fragment (hidden tile ht, k-step kk, piece): lane l holds
 * 2^S W[dim 4 group + (l>>4)][param 8 kk + j][hidden 16 ht + (l&15)].  n % 32 == 0; cfg->inverse must be 0; 4T <= 32. */
#define FC_RQ_BACKWARD_ONE_LAUNCH 3
int fc_rq_fused_linear_backward(int32_t role, const float* x, const float* h, const float* grad_y,
                                const float* grad_logabsdet, const void* w_frag, const float* w_unscale,
                                const float* bias_pad, const void* wt_frag, const int32_t* cols, float* grad_x,
                                float* grad_h, float* grad_bias_pad, float* grad_w_pad, int64_t n, int32_t d,
                                int32_t d_t, const fc_rq_config* cfg, void* stream);

/* Autoregressive INVERSE of a MADE-conditioned layer with the D passes on the device (the reference's sampling loop,
 * flowcon/transforms/autoregressive/autoregressive.py:44-53: D conditioner passes, pass d fixing column d): a wave keeps 16
 * rows, the pre-masked hidden stack (made.py:205-283: initial layer + residual blocks, mask * weight) in LDS, and per pass
 * runs the stack, the params_per_dim final-layer rows of dim d and the element-wise inverse of that column.
 *   z, y [n, d] (d <= 64, n % 16 == 0); logabsdet [n] = sum over the columns (added onto it with FC_RQ_ACCUMULATE_LOGABSDET
 *   in cfg->flags).
 *   hidden_frag / hidden_unscale / hidden_bias: the image of fc_resnet_hidden_packed made from the MASKED weights
 *   (rows 64-padded, in_features = d, 1 k-step for d <= 32 else 2), num_blocks <= 3 ReLU residual blocks.
 *   final_frag: f16 [d][2 k-steps][PT][2 pieces][64 lanes][8], PT = ceil(params_per_dim / 16): lane l of fragment
 *   (dim, ks, t, piece) holds 2^S_dim Wmasked[dim * P + 16 t + (l & 15)][32 ks + 8 (l >> 4) + j] (zero rows beyond P);
 *   final_unscale [d] = 2^-S_dim; final_bias [d][16 PT].
 *   kind FC_MADE_AFFINE (params_per_dim 2: unconstrained scale, shift -- autoregressive.py:97-129; cfg may be NULL) or
 *   FC_MADE_RQ (cfg: the spline, any K <= 16 and tail mode, autoregressive.py:529-621; cfg->inverse is ignored).
 *   units_needed [d] or NULL: pass c reads only the first units_needed[c] hidden units (in feature order 0..63 of EVERY
 *   hidden layer: the caller renumbers the units so that each pass's units form a prefix -- for the reference's degrees,
 *   made.py:13-24, the units of degree <= c) and the kernel computes just the 16-unit product tiles and 32-unit k-steps
 *   that hold them; the other units may then hold any finite value (they meet zeroed weights only).  NULL: all 64.
 *   err_flag: FC_ERR_* bits of the spline inverse. */
#define FC_MADE_AFFINE 0
#define FC_MADE_RQ 1
int fc_made_inverse(const float* z, float* y, float* logabsdet, const void* hidden_frag, const float* hidden_unscale,
                    const float* hidden_bias, const void* final_frag, const float* final_unscale, const float* final_bias,
                    const int32_t* units_needed, uint32_t* err_flag, int64_t n, int32_t d, int32_t num_blocks, int32_t params_per_dim, int32_t kind,
                    const fc_rq_config* cfg, void* stream);

/* fc_made_inverse for a CONDITIONAL MADE: the same D passes with the additive context terms of made.py:153-162 (initial
 * layer: h = W0 x + b0 + relu(Wc[0] c + bc[0])) and made.py:108-118 (block i: Wc[1 + i] c + bc[1 + i] joins the first masked
 * Linear's output before the second activation) -- the FC_CONTEXT_ADDITIVE form of fc_resnet_hidden_context.  The terms do
 * not change from pass to pass: the 16 context rows of a block become one matrix-core operand (two f16 pieces, their OWN
 * power-of-two row scale) before pass 0, and every pass redoes only the products for the unit tiles it computes.
 * Everything fc_made_inverse takes means the same here (same element-wise inverses, units_needed prefix scheme,
 * FC_RQ_ACCUMULATE_LOGABSDET, err_flag bits, n % 16 == 0); dim 0 reads no hidden unit, so its column does not depend on
 * the context.  In addition:
 *   context [n, context_features] row-major f32, 1 <= context_features <= 32.
 *   context_frag: f16 [1 + num_blocks][4 tiles][2 pieces][64 lanes][8]: lane l of fragment (layer, t, piece) holds
 *   2^S_layer Wc[layer][unit of row 16 t + (l & 15)][8 (l >> 4) + j] (zero beyond context_features / hidden), the rows in
 *   the unit order of hidden_frag (the caller's units_needed renumbering applies to them as to every hidden layer);
 *   context_unscale [1 + num_blocks] = 2^-S_layer; context_bias [1 + num_blocks][64] in the order of hidden_bias.
 * Shapes whose LDS image (hidden stack + context layers + parameter strips) exceeds 160 KB have no instantiation and
 * return hipErrorInvalidValue: num_blocks == 3 with params_per_dim > 32, or with d > 32 and params_per_dim > 16. */
int fc_made_inverse_context(const float* z, const float* context, float* y, float* logabsdet, const void* hidden_frag,
                            const float* hidden_unscale, const float* hidden_bias, const void* context_frag,
                            const float* context_unscale, const float* context_bias, const void* final_frag,
                            const float* final_unscale, const float* final_bias, const int32_t* units_needed,
                            uint32_t* err_flag, int64_t n, int32_t d, int32_t context_features, int32_t num_blocks,
                            int32_t params_per_dim, int32_t kind, const fc_rq_config* cfg, void* stream);

/* ---- mixture-of-Gaussians MADE (flowcon/nn/nde/made.py:284-426, distributions/mixture.py) --------------------------------- */
/* Density on the final layer's output (nn/nde/made.py:328-353):
 *   logp[i] = sum_j logsumexp_k( log_softmax(logit_ij.)_k - 0.5 (log 2 pi + 2 log std_ijk + ((x_ij - mean_ijk) / std_ijk)^2) ),
 *   std = softplus(ustd) + epsilon.
 * x [n, d]; params [n, d * 3c], per element the c components interleaved as (logit, mean, ustd) -- the reference's
 * outputs.reshape(n, d, c, 3); logp [n], added onto with FC_RQ_ACCUMULATE_LOGABSDET in flags.  1 <= c <= 16, d >= 1, n >= 0.
 * Maxima are taken before every exponential (logits and summed terms). */
int fc_mog_log_prob(const float* x, const float* params, float* logp, int64_t n, int32_t d, int32_t c, float epsilon,
                    int32_t flags, void* stream);

/* Backward of fc_mog_log_prob: grad_x [n, d] and grad_params (layout of params) of sum_i grad_logp[i] logp[i]; the
 * responsibilities are recomputed from x and params.  grad_params must not alias params. */
int fc_mog_log_prob_backward(const float* grad_logp, const float* x, const float* params, float* grad_x, float* grad_params,
                             int64_t n, int32_t d, int32_t c, float epsilon, void* stream);

/* Ancestral sampler of a MixtureOfGaussiansMADE (nn/nde/made.py:355-388) as ONE kernel: fc_made_inverse with a mixture
 * column step (3c parameters per dim).  Pass j picks component k = min{k : uniform_ij S < sum_{l <= k} e_l},
 * e_l = exp(logit_l - max logit), S = sum_l e_l (the last component when no partial sum exceeds uniform_ij S) and sets
 * x_ij = mean_k + std_k normal_ij; logp [n] = the log mixture density of the finished row (the sum over the columns of
 * fc_mog_log_prob's term at the draw).  normal, uniform, x [n, d]; 1 <= c <= 16; the image, final-layer fragments
 * (params_per_dim = 3c) and units_needed as for fc_made_inverse; n % 16 == 0, d <= 64, num_blocks <= 3. */
#define FC_MADE_MOG 2
int fc_made_mog_sample(const float* normal, const float* uniform, float* x, float* logp, const void* hidden_frag,
                       const float* hidden_unscale, const float* hidden_bias, const void* final_frag, const float* final_unscale,
                       const float* final_bias, const int32_t* units_needed, int64_t n, int32_t d, int32_t num_blocks, int32_t c,
                       float epsilon, void* stream);

/* The conditional form: context arguments as for fc_made_inverse_context, but the initial layer's context term enters
 * WITHOUT an activation (nn/nde/made.py:274-281: temps = initial_layer(inputs) + context_layer(context)).  Shapes whose LDS
 * image exceeds 160 KB (fc_made_inverse_context's rule with params_per_dim = 3c) return hipErrorInvalidValue. */
int fc_made_mog_sample_context(const float* normal, const float* uniform, const float* context, float* x, float* logp,
                               const void* hidden_frag, const float* hidden_unscale, const float* hidden_bias,
                               const void* context_frag, const float* context_unscale, const float* context_bias,
                               const void* final_frag, const float* final_unscale, const float* final_bias,
                               const int32_t* units_needed, int64_t n, int32_t d, int32_t context_features, int32_t num_blocks,
                               int32_t c, float epsilon, void* stream);

/* Backward of fc_affine in the forward direction, per-sample parameters (coupling.py:234-252,
 * autoregressive.py:97-129 under torch.autograd): grad_x[n, cols[j]] = gy s; grad_params in the layout of
 * `params` for the same `activation`.  Other columns of grad_x are NOT written. */
int fc_affine_backward(const float* x, const float* params, const int32_t* cols, const float* grad_y,
                       const float* grad_logabsdet, float* grad_x, float* grad_params, int64_t n,
                       int32_t d, int32_t d_t, int32_t activation, void* stream);

/* Backward of fc_rq_spline in the forward direction (what torch.autograd yields for the reference's op
 * sequence, rational_quadratic.py:13-181; the reference trains through it, examples/toy_2d.py:57-68):
 *   grad_x[n, cols[j]]            = gy dy/dx + gl dlogabsdet/dx      (the other columns: grad_x = grad_y, the
 *                                                                      bijector copies them)
 *   grad_params[n, j*P .. j*P+P)  = gy dy/dp + gl dlogabsdet/dp      for the P = 3K-1 (3K+1) raw values of dim j
 * x [n, d], params [n, d_t*P] (per-sample rows only), grad_y [n, d], grad_logabsdet [n] or NULL (zeros).
 * cfg->inverse must be 0; num_bins <= 32. */
int fc_rq_spline_backward(const float* x, const float* params, const int32_t* cols, const float* grad_y,
                          const float* grad_logabsdet, float* grad_x, float* grad_params, int64_t n,
                          int32_t d, int32_t d_t, const fc_rq_config* cfg, void* stream);

/* Hidden layers of the ResidualNet conditioner (flowcon/nn/nets/resnet.py:39-53, 93-99) as one kernel:
 *   h = W0 x[:, id_cols] + b0;  per block: h += W2 relu(W1 relu(h) + b1) + b2          -> h [n, 64]
 * Products on the f16 matrix cores as three-term scaled two-piece splits (f32-GEMM accuracy); a wave carries
 * 16 samples through all layers in registers; the only HBM traffic is x in and h out.
 * `activation` (FC_ACT_*) is the blocks' activation: ReLU kernels carry nothing but a v_max; the others share one
 * kernel family with a uniform switch (tanh, SiLU, ELU, LeakyReLU, sigmoid as ATen computes them in float32).
 * Specialised: hidden == 64, num_blocks <= 4, no batch norm / active dropout (context: next entry),
 * in_features <= 64, n % 16 == 0, h 16-byte aligned.
 * Weights are the nn.Linear tensors as they are, row-major f32: w0 [64, in_features]; wb [blocks][2][64][64]
 * (linear_layers[0], linear_layers[1] of each block); b0 [64]; bb [blocks][2][64]. */
#define FC_ACT_RELU 0
#define FC_ACT_TANH 1
#define FC_ACT_SILU 2
#define FC_ACT_ELU 3        /* activation_param = alpha */
#define FC_ACT_LEAKY_RELU 4 /* activation_param = negative slope */
#define FC_ACT_SIGMOID 5
int fc_resnet_hidden(const float* x, float* h, const int32_t* id_cols, const float* w0,
                     const float* b0, const float* wb, const float* bb, int64_t n, int32_t d,
                     int32_t in_features, int32_t hidden, int32_t num_blocks, int32_t activation,
                     float activation_param, void* stream);

/* fc_resnet_hidden with the weights prepared ahead of time (same results, bit for bit): w_frag = the layers' f16
 * fragment images back to back ([layer][k-step][tile][piece][lane][8], FC_PACK_HIDDEN jobs of fc_pack_fragments: the
 * initial layer with nks = 1 (in_features <= 32) or 2, every block layer with nks = 2, nt = 4), w_unscale [L] and
 * bias_acc [L][64] from the same jobs, L = 1 + 2 num_blocks.  The kernel then starts with a copy of the image into LDS
 * instead of two rounds of weight loads, the scaling / splitting arithmetic and two barriers (~19 us per launch at
 * 2 blocks).  No context. */
int fc_resnet_hidden_packed(const float* x, float* h, const int32_t* id_cols, const void* w_frag,
                            const float* w_unscale, const float* bias_acc, int64_t n, int32_t d,
                            int32_t in_features, int32_t hidden, int32_t num_blocks, int32_t activation,
                            float activation_param, void* stream);

/* One kernel per AFFINE coupling layer (flowcon/transforms/coupling.py:73-100 + :212-269 with a ResidualNet conditioner,
 * nn/nets/resnet.py:55-100): hidden stack, final Linear and the affine / additive bijector; neither h nor the [n, 2 d_t]
 * parameter tensor reaches memory.  y [n, d] (must not alias x) receives the identity columns unchanged and the transformed
 * ones; logabsdet [n] is written, or added to when accumulate != 0 (CompositeTransform's running total).
 *   w_frag / w_unscale / bias_acc: the image of fc_resnet_hidden_packed with ONE MORE 64 x 64 layer, the final Linear
 *   re-ordered as rows 0..31 = its shift rows of dims 0..31, rows 32..63 = its scale rows (zero rows beyond d_t; additive:
 *   no scale rows), i.e. L = 2 + 2 num_blocks layers.
 * scale_activation: FC_AFFINE_SIGMOID_PLUS2, FC_AFFINE_SOFTPLUS_CLAMP3, FC_AFFINE_ADDITIVE, or FC_AFFINE_MAF_SOFTPLUS (the density
 * direction of a masked-autoregressive affine layer, autoregressive.py:97-129: id_cols = tr_cols = all columns, weights pre-masked,
 * final-layer rows in the same [shift 32 | scale 32] order).  ReLU conditioner, hidden == 64
 * (narrower: zero-padded), num_blocks <= 3, in_features <= 64, d_t <= 32, d <= 128, n % 16 == 0; the weight image and the
 * waves' row tiles (8 x 16 x (d | 1) floats) must fit the CU's 160 KB of LDS (else hipErrorInvalidConfiguration). */
int fc_affine_coupling_resnet(const float* x, float* y, const int32_t* id_cols, const int32_t* tr_cols,
                              const void* w_frag, const float* w_unscale, const float* bias_acc, float* logabsdet,
                              int64_t n, int32_t d, int32_t in_features, int32_t d_t, int32_t hidden, int32_t num_blocks,
                              int32_t scale_activation, int32_t inverse, int32_t accumulate, void* stream);

/* Backward of fc_resnet_hidden (what torch.autograd yields for resnet.py:39-53, 93-99): the activations are recomputed
 * from x; grad_h [n, 64] in -> grad_x_id [n, 32 K0S] (gradient wrt x[:, id_cols], K0S = 1 for in_features <= 32 else 2),
 * and, ACCUMULATED with atomics (zero them first): grad_w0 [64][32 K0S], grad_wb [2 num_blocks][64][64], grad_b [L][64],
 * L = 1 + 2 num_blocks.  hidden == 64, num_blocks <= 2, ReLU, no context, n % 128 == 0.  The weight gradients contract
 * over samples on the exact-f32 matrix instruction (v_mfma_f32_16x16x4_f32).
 *   w_frag   forward fragments, f16: layer 0 [K0S][4][2][64][8], then per layer [2][4][2][64][8]; rows of tile t in
 *            accumulator order: row rho <-> feature 32 (t >> 1) + 8 (rho >> 2) + 4 (t & 1) + (rho & 3)
 *   wt_frag  fragments of the transposed weights: per hidden layer [2][4][2][64][8] (rows = in-features in the same order,
 *            k = out-features), last: W0^T [2][2 K0S][2][64][8] (rows = identity features, natural order)
 *   w_unscale [L];  bias_acc [L][4][16]: bias_acc[l][g][4 t + r] = bias_l[32 (t >> 1) + 8 g + 4 (t & 1) + r] */
int fc_resnet_hidden_backward(const float* x, const float* grad_h, const int32_t* id_cols, const void* w_frag,
                              const void* wt_frag, const float* w_unscale, const float* bias_acc, float* grad_x_id,
                              float* grad_w0, float* grad_wb, float* grad_b, int64_t n, int32_t d, int32_t in_features,
                              int32_t hidden, int32_t num_blocks, int32_t activation, void* stream);

/* The same, with the gradient wrt the identity columns ADDED into the full-width gradient of the layer input instead of
 * written to its own [n, 32 K0S] tensor: grad_x_full[:, id_cols] += ... (every (row, identity column) is owned by one
 * lane).  Saves the index_add pass over [n, d] that follows in a coupling layer's backward. */
int fc_resnet_hidden_backward_accum(const float* x, const float* grad_h, const int32_t* id_cols, const void* w_frag,
                                    const void* wt_frag, const float* w_unscale, const float* bias_acc, float* grad_x_full,
                                    float* grad_w0, float* grad_wb, float* grad_b, int64_t n, int32_t d, int32_t in_features,
                                    int32_t hidden, int32_t num_blocks, int32_t activation, void* stream);

/* The same stack for WIDE conditioners: hidden in {128, 256} (hidden_features is a free constructor argument,
 * resnet.py:62; narrower widths zero-padded by the host), any num_blocks <= 16, no context.  The activations of a
 * 64-sample tile live in LDS as matrix-core B operands shared by the workgroup's 8 waves; wave w owns the output
 * features [w hidden/8, (w+1) hidden/8) of every layer and streams their weight fragments from L2.  n % 64 == 0.
 *   w_frag    f16: layer 0 [hidden/16][K0S][2][64][8] (K0S = 1 for in_features <= 32, else 2), then per layer
 *             [hidden/16][hidden/32][2][64][8]: fragment (tile t, k-step, piece hi/lo): lane l holds
 *             2^S_layer W[16 t + (l & 15)][32 kstep + 8 (l >> 4) + j], j < 8
 *   w_unscale f32 [1 + 2 num_blocks] = 2^-S_layer;  bias f32 [1 + 2 num_blocks][hidden] */
int fc_resnet_hidden_wide(const float* x, float* h, const int32_t* id_cols, const void* w_frag,
                          const float* w_unscale, const float* bias, int64_t n, int32_t d, int32_t in_features,
                          int32_t hidden, int32_t num_blocks, int32_t activation, float activation_param,
                          void* stream);

/* The same with a context (resnet.py:48-49, 94-97): the initial layer sees [x[:, id_cols] | context]
 * (w0 [64, in_features + context_features]) and every block gates its output,
 *   h += (W2 relu(W1 relu(h) + b1) + b2) * sigmoid(Wc context + bc)      (F.glu of the concatenation),
 * wc [blocks][64][context_features] / bc [blocks][64] = blocks[i].context_layer.  context [n, context_features]
 * row-major; context_features <= 32, in_features + context_features <= 64, num_blocks <= 3. */
#define FC_CONTEXT_GLU 1      /* ResidualNet: as above */
#define FC_CONTEXT_ADDITIVE 2 /* MADE (transforms/made.py:100-140, 239-246): w0 [64, in_features] only;
                                 h = W0 x + b0 + act(Wc[0] c + bc[0]); per block h += W2 act(W1 act(h) + b1 + Wc[1+i] c
                                 + bc[1+i]) + b2;  wc [blocks + 1][64][context_features], bc [blocks + 1][64] */
int fc_resnet_hidden_context(const float* x, const float* context, float* h, const int32_t* id_cols,
                             const float* w0, const float* b0, const float* wb, const float* bb,
                             const float* wc, const float* bc, int64_t n, int32_t d, int32_t in_features,
                             int32_t context_features, int32_t hidden, int32_t num_blocks, int32_t context_mode,
                             int32_t activation, float activation_param, void* stream);

/* ---- linear / quadratic / cubic splines ------------------------------------------------------ */
#define FC_SPLINE_LINEAR 0    /* row per dim: [K pdf]                          (splines/linear.py:38-105) */
#define FC_SPLINE_QUADRATIC 1 /* row per dim: [K widths | K-1 or K+1 heights]  (splines/quadratic.py:55-159) */
#define FC_SPLINE_CUBIC 2     /* row per dim: [K widths | K heights | dl | dr] (splines/cubic.py:63-267) */

typedef struct fc_spline_config {
  int32_t kind;           /* FC_SPLINE_* */
  int32_t num_bins;
  int32_t tails;          /* 0 none, 1 "linear" */
  int32_t inverse;
  float left, right, bottom, top;      /* linear tails: -B, B, -B, B */
  double min_bin_width, min_bin_height; /* python floats of the reference */
  float width_divisor, height_divisor;  /* sqrt(hidden_features) or 1 (coupling.py:438-440,
                                           autoregressive.py:430-432: AR quadratic scales widths only) */
  float cubic_eps;                      /* 1e-5 */
  float cubic_quadratic_threshold;      /* 1e-3 */
} fc_spline_config;

/* Sibling piecewise bijectors of the RQ spline, same conventions as fc_rq_spline.  Replaces
 * {linear,quadratic,cubic}_spline and their unconstrained_* wrappers behind
 * Piecewise{Linear,Quadratic,Cubic}CouplingTransform (coupling.py:299-499),
 * MaskedPiecewise{Linear,Quadratic,Cubic}AutoregressiveTransform (autoregressive.py:321-526) and
 * Piecewise{Linear,Quadratic,Cubic}CDF (nonlinearities.py:250-427). */
int fc_piecewise_spline(const float* x, float* y, const float* params, const int32_t* cols,
                        float* logabsdet, uint32_t* err_flag, int64_t n, int32_t d, int32_t d_t,
                        int32_t shared_params, int32_t lad_mode, const fc_spline_config* cfg,
                        void* stream);

/* fc_made_inverse (above) for the sibling splines: the D passes of MaskedPiecewise{Linear,Quadratic,Cubic}
 * AutoregressiveTransform.inverse (autoregressive.py:321-526) in ONE kernel.  z, y, logabsdet, the hidden-stack image, the
 * final-layer fragments, units_needed, err_flag, n % 16 == 0, d <= 64 and num_blocks <= 3 mean what they mean for
 * fc_made_inverse; the parameters per dim follow from cfg: K (linear), 2K - 1 / 2K + 1 (quadratic with / without linear
 * tails), 2K + 2 (cubic), at most 48.  Pass c hands the raw final-layer rows of dim c to one lane per sample, which derives
 * widths / heights in place and evaluates the inverse exactly as fc_piecewise_spline does (cfg->inverse is ignored).
 * Without tails an input outside [bottom, top] sets FC_ERR_OUTSIDE_DOMAIN.  lad_flags: FC_RQ_ACCUMULATE_LOGABSDET or 0.
 * Shapes out of range return hipErrorInvalidValue.  Added under ABI version 3 (it changes no existing entry). */
int fc_made_inverse_spline(const float* z, float* y, float* logabsdet, const void* hidden_frag, const float* hidden_unscale,
                           const float* hidden_bias, const void* final_frag, const float* final_unscale,
                           const float* final_bias, const int32_t* units_needed, uint32_t* err_flag, int64_t n, int32_t d,
                           int32_t num_blocks, const fc_spline_config* cfg, int32_t lad_flags, void* stream);

/* Backward of fc_piecewise_spline in the forward direction (cfg->inverse == 0), per-sample rows: grad_x [n, d] (the
 * d_t transformed columns are written; the caller owns the identity columns) and grad_params [n, d_t P] from grad_y
 * [n, d] and grad_logabsdet [n] (NULL = zeros).  What torch.autograd yields for splines/linear.py:38-105,
 * quadratic.py:55-159, cubic.py:63-267: the kernel differentiates the forward evaluation in forward mode, one thread per
 * (element, parameter).  P <= 32 parameters per element. */
int fc_piecewise_spline_backward(const float* x, const float* params, const int32_t* cols, const float* grad_y,
                                 const float* grad_logabsdet, float* grad_x, float* grad_params, int64_t n,
                                 int32_t d, int32_t d_t, const fc_spline_config* cfg, void* stream);

/* ---- affine / additive with per-sample parameters ------------------------------------------ */
#define FC_AFFINE_SIGMOID_PLUS2 0   /* row [shift d_t | u d_t], s = sigmoid(u+2)+1e-3 (coupling.py:224) */
#define FC_AFFINE_SOFTPLUS_CLAMP3 1 /* row [shift | u], s = clamp(softplus(u)+1e-3, 0, 3) (coupling.py:225) */
#define FC_AFFINE_SCALE_GIVEN 2     /* row [shift | s]: scale already activated by the caller */
#define FC_AFFINE_ADDITIVE 3        /* row [shift d_t], s = 1, logabsdet = 0 (coupling.py:255-269) */
#define FC_AFFINE_MAF_SOFTPLUS 4    /* row [d_t, 2] interleaved (u, shift), s = softplus(u)+1e-3
                                       (autoregressive/autoregressive.py:97-129) */

#define FC_AFFINE_SHIFT_TANH2 5     /* row [p d_t], shift = 2*tanh(p), s = 1 (autoregressive.py:164-175;
                                       the reference's inverse subtracts raw p: use ADDITIVE) */

#define FC_AFFINE_SCALE_SOFTPLUS 6   /* row [p d_t], shift = 0, s = softplus(p)+1e-5 (conditional.py:212-272) */

/* y = x*s + shift (forward) or (x - shift)/s (inverse) on the `cols` columns, logabsdet =
 * +/- sum_j log s.  Replaces AffineCouplingTransform / AdditiveCouplingTransform
 * (coupling.py:212-269) incl. the split/merge of coupling.py:82-98, and
 * MaskedAffineAutoregressiveTransform._elementwise_{forward,inverse}
 * (autoregressive/autoregressive.py:97-129). */
int fc_affine(const float* x, float* y, const float* params, const int32_t* cols,
              float* logabsdet, int64_t n, int32_t d, int32_t d_t, int32_t activation,
              int32_t inverse, int32_t shared_params, int32_t lad_mode, void* stream);

/* ---- base-distribution epilogue ---------------------------------------------------------- */
/* out[i] = -0.5 * sum_j z[i,j]^2 - log_z (+ add[i] when add != NULL).  Replaces
 * StandardNormal._log_prob (distributions/normal.py:23-33) and the `log_prob + logabsdet` of
 * Flow._log_prob (flows/base.py:48). */
int fc_standard_normal_log_prob(const float* z, const float* add, float* out, int64_t n,
                                int32_t d, float log_z, void* stream);

/* ---- discrete and uniform bases (any d >= 1: the lanes loop over their row) ------------------ */
/* out[i] = sum_j ( inputs[i,j] * logits[i,j] - softplus(logits[i,j]) ) (+ add[i] when add != NULL), with
 * softplus(l) = max(l, 0) + log1p(exp(-|l|)): ConditionalIndependentBernoulli._log_prob (distributions/discrete.py:41-56,
 * -x softplus(-l) - (1 - x) softplus(l) summed over the event) for every real x, not only 0 / 1. */
int fc_bernoulli_log_prob(const float* inputs, const float* logits, const float* add, float* out, int64_t n, int32_t d,
                          void* stream);

/* Backward of fc_bernoulli_log_prob from the row gradient grad_out [n]: grad_logits [n, d] = g (x - sigmoid(l)),
 * grad_inputs [n, d] = g l.  Either output may be NULL (inputs may be NULL when grad_logits is); the gradient of add is
 * grad_out itself. */
int fc_bernoulli_log_prob_backward(const float* inputs, const float* logits, const float* grad_out, float* grad_logits,
                                   float* grad_inputs, int64_t n, int32_t d, void* stream);

/* out[r, j] = noise[r, j] < sigmoid(logits[r / num_samples, j]) ? 1 : 0 for logits [contexts, d] and noise / out
 * [contexts * num_samples, d] (distributions/discrete.py:58-68 without the repeated probability rows). */
int fc_bernoulli_sample(const float* logits, const float* noise, float* out, int64_t contexts, int32_t num_samples,
                        int32_t d, void* stream);

/* out[i] = -sum_j log(high[j] - low[j]) when low[j] <= inputs[i,j] < high[j] for every j, -inf otherwise (a NaN input
 * fails both comparisons): torch.distributions.Uniform.log_prob summed over the event dimension, as BoxUniform
 * (distributions/uniform.py:7-29) evaluates it.  low and high are [d]. */
int fc_box_log_prob(const float* inputs, const float* low, const float* high, float* out, int64_t n, int32_t d,
                    void* stream);

/* ---- batch statistics: reductions over the batch axis (fc_colstats.hip) -------------------------- */
/* All of these take [n, d] row-major float32 rows with 2 <= n and 1 <= d <= FC_COLSTATS_MAX_FEATURES and return
 * hipErrorInvalidValue otherwise.  Every reduction runs in two stages without atomics: at most FC_COLSTATS_MAX_PARTIALS
 * workgroups each reduce a contiguous slice of rows into one row of `workspace` (fc_colstats_workspace(d) floats, the
 * caller's, no alignment beyond the 16 bytes of a device allocation needed), one workgroup merges the rows in a fixed
 * order: the bits of a result depend on (n, d) and on whether the pointers are 16-byte aligned, nothing else.  A stage-1
 * workgroup walks its slice FC_COLSTATS_ROWS_PER_ITERATION rows at a time when d <= 4 (fewer for wider rows). */
#define FC_COLSTATS_MAX_FEATURES 512
#define FC_COLSTATS_MAX_PARTIALS 512
#define FC_COLSTATS_ROWS_PER_ITERATION 2048

/* Floats of workspace the entries below need for rows of d features (0 for a d out of range). */
int fc_colstats_workspace(int32_t d);

/* BatchNorm.forward in training mode (transforms/normalization.py:98-141): mean[d] and var[d] = the batch mean and the
 * unbiased variance of every column (Chan's pairwise merge of per-lane moments, never sum x^2), invstd[d] =
 * 1 / sqrt(var + eps), half_log_sum[1] = sum_j -0.5 log(var_j + eps), y = weight ((x - mean) invstd) + bias.  When
 * running_mean / running_var [d] are given (both or neither) they move in place: r += momentum (stat - r). */
int fc_batchnorm_train(const float* x, const float* weight, const float* bias, float* y, float* mean, float* var,
                       float* invstd, float* half_log_sum, float* running_mean, float* running_var, float* workspace,
                       int64_t n, int32_t d, float eps, float momentum, void* stream);

/* s1[j] = sum_i g[i,j], s2[j] = sum_i g[i,j] vh[i,j] with vh = (v - mean) invstd, or v itself when mean and invstd are
 * NULL (both or neither); gl_sum[1] = sum_i gl[i] when gl [n] is given. */
int fc_column_sums(const float* g, const float* v, const float* mean, const float* invstd, const float* gl, float* s1,
                   float* s2, float* gl_sum, float* workspace, int64_t n, int32_t d, void* stream);

/* Backward of fc_batchnorm_train for upstream gradients grad_y [n, d] and grad_logabsdet [n] (or NULL) of
 * logabsdet[i] = sum_j log weight_j - 0.5 log(var_j + eps):  s1, s2, gl_sum = fc_column_sums(grad_y, x, mean, invstd,
 * grad_logabsdet) (so grad_bias = s1, grad_weight = s2 + gl_sum / weight), and, unless grad_x is NULL, with
 * xh = (x - mean) invstd:
 *   grad_x = weight invstd (grad_y - s1 / n - xh s2 / (n - 1)) - gl_sum invstd xh / (n - 1). */
int fc_batchnorm_train_backward(const float* x, const float* grad_y, const float* grad_logabsdet, const float* mean,
                                const float* invstd, const float* weight, float* grad_x, float* s1, float* s2,
                                float* gl_sum, float* workspace, int64_t n, int32_t d, void* stream);

/* ---- permutation ------------------------------------------------------------------------- */
/* y[o, j, i] = x[o, perm[j], i] for a tensor viewed as [outer, d, inner]; bit-exact.  x != y.
 * Replaces Permutation._permute (transforms/permutations.py:27-46, torch.index_select). */
int fc_permute(const float* x, float* y, const int32_t* perm, int64_t outer, int32_t d,
               int64_t inner, void* stream);

/* ---- flows on symmetric positive definite matrices ---------------------------------------- */
/* All matrices are [batch, m, m] row-major float32, d = m (m + 1) / 2; x != y everywhere.
 * fc_tril_pack     mode 0: y[b] = the m x m matrix with x[b, :] on and below the diagonal in np.tril_indices(m)
 *                  order, zeros above (FillTriangular.forward, permutations.py:97-106); mode 1: the gather back,
 *                  y[b, :] = x[b][tril_indices] (FillTriangular.inverse, :108-113).  Bit-exact; each mode is the
 *                  other's backward.
 * fc_matrix_diag   mode 0: diag[b, i] = x[b, i, i] (torch.diagonal); mode 1: y = x with its diagonal replaced by
 *                  diag (torch.diagonal_scatter, matrix/diagonal.py:37-45); x == NULL reads as zeros (the
 *                  backward of mode 0).  Bit-exact.
 * fc_cholesky_outer  y = 0.5 (L L^T + (L L^T)^T) over the FULL input (upper part included),
 *                  logabsdet[b] = m log 2 + sum_i (m - i) log L_ii (CholeskyOuterProduct.forward,
 *                  matrix/cholesky.py:18-25).  checkargs != 0 ORs FC_ERR_NOT_LOWER_TRIANGULAR /
 *                  FC_ERR_DIAGONAL_NONPOSITIVE into err_flag (:37-43).  logabsdet may be NULL.
 * fc_cholesky_outer_backward  grad_inputs = (G + G^T) L + diag((m - i) grad_logabsdet[b] / L_ii), the autograd of
 *                  the forward over the full m x m input; grad_outputs or grad_logabsdet may be NULL (zero).
 * fc_cholesky      L = chol(A + eps I) with exact zeros above the diagonal, the jitter added in float32 first;
 *                  logabsdet[b] = -(m log 2 + sum_i (m - i) log L_ii) (CholeskyOuterProduct.inverse, :27-35).
 *                  checkargs != 0: FC_ERR_NOT_SYMMETRIC when A != A^T, FC_ERR_NOT_POSITIVE_DEFINITE on a pivot
 *                  <= 0; checkargs == 0: FC_ERR_CHOLESKY_FAILED on a pivot <= 0.  err_flag is required.
 * 1 <= m <= FC_SPD_MAX_DIM for the three matrix entries (hipErrorInvalidValue otherwise). */
#define FC_SPD_MAX_DIM 128
int fc_tril_pack(const float* x, float* y, int64_t batch, int32_t m, int32_t mode, void* stream);
int fc_matrix_diag(const float* x, float* diag, float* y, int64_t batch, int32_t m, int32_t mode, void* stream);
int fc_cholesky_outer(const float* L, float* y, float* logabsdet, uint32_t* err_flag, int64_t batch, int32_t m,
                      int32_t checkargs, void* stream);
int fc_cholesky_outer_backward(const float* L, const float* grad_outputs, const float* grad_logabsdet,
                               float* grad_inputs, int64_t batch, int32_t m, void* stream);
int fc_cholesky(const float* A, float* L, float* logabsdet, uint32_t* err_flag, int64_t batch, int32_t m, float eps,
                int32_t checkargs, void* stream);

/* ---- flows on images ------------------------------------------------------------------------ */
/* Contiguous NCHW float32 tensors; x != y.
 * fc_squeeze   planes = B C of the un-squeezed tensor, h / w its spatial size (both divisible by factor >= 2).
 *              mode 0: x [planes, h, w] -> y [planes, f^2, h/f, w/f] in the order of
 *              view(B, C, h/f, f, w/f, f).permute(0, 1, 3, 5, 2, 4) (SqueezeTransform.forward, reshape.py:28-48);
 *              mode 1: the inverse (reshape.py:50-66).  Bit-exact; each mode is the other's backward.
 * fc_conv1x1   per image b and pixel p: y[b, :, p] = weight (x[b, :, p] - pre) + post, weight [c, c] row-major,
 *              pre / post [c] or NULL (zero); hw = H W.  The forward of OneByOneConvolution (conv.py) is the
 *              permutation folded into the columns of weight and post = bias; its inverse is the permutation folded
 *              into the rows of weight^-1 and pre = bias (the bias is subtracted BEFORE the product).
 *              1 <= c <= FC_CONV1X1_MAX_CHANNELS (hipErrorInvalidValue otherwise). */
#define FC_CONV1X1_MAX_CHANNELS 128
int fc_squeeze(const float* x, float* y, int64_t planes, int32_t h, int32_t w, int32_t factor, int32_t mode,
               void* stream);
int fc_conv1x1(const float* x, const float* weight, const float* pre, const float* post, float* y, int64_t batch,
               int32_t c, int64_t hw, void* stream);

/* ---- invertible residual blocks over Lipschitz DenseNets (eval mode) -------------------------- */
/* iResBlock (transforms/lipschitz/iresblock.py:96-153) over a _DenseNet (nn/nets/invertible_densenet.py:68-95,
 * lipschitz_dense.py:53-56) in eval mode: g(x) = final(h_depth), h_0 = [x | extra],
 * h_{l+1} = cat(eta1_l h_l, eta2_l act(W_l h_l + b_l)), growth channels per layer.
 *   image   float32 [image_floats], the net with the spectral normalisation applied (the eval-mode weights):
 *           [p0, p1, 0, 0]; per dense layer [eta1, eta2, 0, 0] bias[op] wt[w_in][op] with op = out_ch rounded up to 4,
 *           wt[k][o] = W[o][k], w_in = d + e + l growth, out_ch = growth (growth / 2 for the concatenating
 *           activations); final layer bias[dp] wt[wtot][dp], dp = d rounded up to 4, wtot = d + e + depth growth.
 *           Padding entries are zero.  p0 / p1: softplus(beta) of the Swish family, w0 of the sine family, alpha of
 *           ELU; p1 = sigmoid(alpha) of LeakyLSwish.  image_floats must equal the length this layout gives.
 *   extra   [n, e] or NULL (e == 0): per-row constant input channels appended to x (tangent zero) -- the context
 *           embedding of InputConditionalDenseNet (invertible_densenet.py:211-216)
 *   scale   [n] or NULL: per-row factor on g and its Jacobian -- tanh(factor_net) of the Multiplicative* nets (:263-269)
 * fc_iresnet_forward  y [n, d] = x + scale g(x), logabsdet [n] = log|det(I + scale dg/dx)| (what the brute-force
 *           estimator yields, iresblock.py:290-295): exact forward-mode Jacobian, LU with partial pivoting; a singular
 *           matrix gives -inf.  x != y.
 * fc_iresnet_inverse  x [n, d] with x + scale g(x) = y by x <- y - scale g(x) from x_0 = y - scale g(y)
 *           (iresblock.py:111-134); a row stops when |x - x_prev| <= atol + rtol |y| for all its elements or after
 *           max_iterations.  max_iters: device word or NULL; the launch max-reduces its largest iteration count into
 *           it (zero it first).  x != y.
 * 1 <= d <= FC_IRES_MAX_DIM, 1 <= depth <= FC_IRES_MAX_DEPTH, wtot <= FC_IRES_MAX_WIDTH (hipErrorInvalidValue
 * otherwise). */
#define FC_IRES_MAX_DIM 16
#define FC_IRES_MAX_DEPTH 4
#define FC_IRES_MAX_WIDTH 128
#define FC_IRES_ACT_RELU 0
#define FC_IRES_ACT_TANH 1
#define FC_IRES_ACT_ELU 2
#define FC_IRES_ACT_SWISH 3        /* t sigmoid(p0 t) / 1.1 (activations.py:84-91) */
#define FC_IRES_ACT_LIPSWISH 4     /* swish / 1.004 (:143-150) */
#define FC_IRES_ACT_CLIPSWISH 5    /* lipswish(cat(t, -t)) (:131-140) */
#define FC_IRES_ACT_SIN 6          /* sin(p0 t) / p0 (:94-100) */
#define FC_IRES_ACT_CSIN 7         /* sin(p0 cat(t, -t)) / (p0 sqrt 2) (:105-113) */
#define FC_IRES_ACT_LEAKY_LSWISH 8 /* p1 t + (1 - p1) swish(t) (:119-128) */
int fc_iresnet_forward(const float* x, const float* extra, const float* scale, const float* image, float* y,
                       float* logabsdet, int64_t n, int32_t d, int32_t e, int32_t depth, int32_t growth,
                       int32_t activation, int32_t image_floats, void* stream);
int fc_iresnet_inverse(const float* y, const float* extra, const float* scale, const float* image, float* x,
                       uint32_t* max_iters, int64_t n, int32_t d, int32_t e, int32_t depth, int32_t growth,
                       int32_t activation, int32_t image_floats, int32_t max_iterations, float atol, float rtol,
                       void* stream);
/* fc_iresnet_backward  the reverse sweep of fc_iresnet_forward for the cotangents gy [n, d] of y and gl [n] of logabsdet.
 *           Nothing but x, extra, scale and the image is read from the forward call: a block recomputes the value and
 *           tangent streams in LDS (the forward's lane groups and rounding points), inverts I + scale J inside the lane
 *           group (Gauss-Jordan with partial pivoting, float64) and sweeps the layers from the last.
 *   dx      [n, d], dextra [n, e] (NULL when e == 0), dscale [n] (NULL when scale is NULL): written once per row
 *   dimage  [image_floats]: the gradient of every image entry (weights in the image's transposed padded layout, biases,
 *           eta1 / eta2, p0 / p1; padding entries zero).  Every block sums its rows into one image-shaped float64
 *           partial of ws in a fixed order and a second kernel adds the partials in block order: no atomics, the same
 *           bits on every run.
 *   ws      float64 [fc_iresnet_backward_workspace(...)]; max_blocks caps the grid (<= 0: the default of 256 blocks;
 *           the blocks stride over the row tiles).
 * fc_iresnet_backward_workspace  the number of float64 entries of ws, or -1 for a shape outside the limits. */
int fc_iresnet_backward(const float* x, const float* extra, const float* scale, const float* image, const float* gy,
                        const float* gl, float* dx, float* dextra, float* dscale, float* dimage, double* ws, int64_t n,
                        int32_t d, int32_t e, int32_t depth, int32_t growth, int32_t activation, int32_t image_floats,
                        int32_t max_blocks, void* stream);
int fc_iresnet_backward_workspace(int64_t n, int32_t d, int32_t e, int32_t depth, int32_t growth, int32_t activation,
                                  int32_t max_blocks);

/* ---- continuous normalizing flows (eval mode) ------------------------------------------------- */
/* ODEfunc over an ODEnet of time-conditioned linear layers (CNF/neural_odes/odefunc.py:98-182,
 * diffeq_layers/basic.py:36-94): f(t, y) = scale_output * net(t, y) (- y with residual), every layer
 *     pre = W x + b + w_t t,  out = pre * gate + w_b t,  gate = sigmoid(w_g t + b_g) or 1,
 * the activation between layers, none after the last.  layers = hidden layers + 1; hidden[layers - 1] their widths
 * (host memory, NULL when layers == 1).
 *   image   float32 [image_floats]; per layer b[op] w_t[op] w_g[op] b_g[op] w_b[op] wt[in][op], op = out rounded
 *           up to 4, wt[k][o] = W[o][k], zero padding; vectors a layer kind does not have are zero.  layer_kind
 *           says whether the gate is evaluated (SQUASH, CONCATSQUASH) or is 1.  image_floats must equal the length
 *           this layout gives.
 *   p0      alpha of ELU
 *   evals   float32 device word or NULL
 * fc_cnf_field      dy [n, d] = f(t, y), negdiv [n] = -sum_j df_j/dy_j (exact, forward mode), t = t_dev[0] when
 *           t_dev is not NULL, else the argument t; adds 1 to *evals.  y != dy.
 * fc_cnf_integrate  (z_out [n, d], logp_out [n]) = (z, logp) + int_{t0}^{t1} (f, -div f) dt in `steps` equal steps of
 *           Euler, the explicit midpoint rule or the classical Runge-Kutta method, every row on its own; logp NULL
 *           means zeros; max-reduces steps * stages into *evals.  t1 < t0 integrates backwards.  z != z_out.
 * 1 <= d <= FC_CNF_MAX_DIM, layers <= FC_CNF_MAX_HIDDEN_LAYERS + 1, widths <= FC_CNF_MAX_WIDTH
 * (hipErrorInvalidValue otherwise). */
#define FC_CNF_MAX_DIM 16
#define FC_CNF_MAX_HIDDEN_LAYERS 4
#define FC_CNF_MAX_WIDTH 64
#define FC_CNF_LAYER_IGNORE 0
#define FC_CNF_LAYER_CONCAT 1
#define FC_CNF_LAYER_CONCAT_V2 2
#define FC_CNF_LAYER_SQUASH 3
#define FC_CNF_LAYER_CONCATSQUASH 4
#define FC_CNF_ACT_TANH 0
#define FC_CNF_ACT_RELU 1
#define FC_CNF_ACT_SOFTPLUS 2      /* beta 1, threshold 20 */
#define FC_CNF_ACT_ELU 3
#define FC_CNF_ACT_SWISH 4         /* t sigmoid(t) */
#define FC_CNF_ACT_SQUARE 5
#define FC_CNF_ACT_IDENTITY 6
#define FC_CNF_EULER 0
#define FC_CNF_MIDPOINT 1
#define FC_CNF_RK4 2
int fc_cnf_field(const float* y, const float* image, float* dy, float* negdiv, float* evals, int64_t n, int32_t d,
                 int32_t layers, const int32_t* hidden, int32_t layer_kind, int32_t activation, int32_t residual,
                 float scale_output, float p0, int32_t image_floats, float t, const float* t_dev, void* stream);
int fc_cnf_integrate(const float* z, const float* logp, const float* image, float* z_out, float* logp_out,
                     float* evals, int64_t n, int32_t d, int32_t layers, const int32_t* hidden, int32_t layer_kind,
                     int32_t activation, int32_t residual, float scale_output, float p0, int32_t image_floats,
                     double t0, double t1, int32_t steps, int32_t method, void* stream);

/* fc_cnf_dopri5  (z_out [n, d], logp_out [n]) = (z, logp) + int_{t0}^{t1} (f, -div f) dt with the Dormand-Prince 5(4)
 *           pair, one launch, no host sync, the same net description and limits as above.  EVERY ROW ON ITS OWN: a
 *           row has its own t, step size, accept / reject decisions and attempt count, and its error ratio is the
 *           root mean square over its own d + 1 entries (z and logp) of
 *               h sum_j e_j k_j / (atol + rtol max(|y0|, |y1|)),
 *           accepted when <= 1; step factor clip(0.9 ratio^(-1/5), 0.2, 10) (10 at ratio 0, at most 1 after a
 *           rejection); first same as last; the last step is shortened to end on t1; t1 < t0 integrates backwards.
 *           first_step > 0 is the first step size (one evaluation before the first attempt); 0 selects the initial
 *           step of Hairer, Norsett & Wanner II.4 in the row's own norm (two evaluations).  t, h, the state, the
 *           slopes, the error and the controller are float64; a stage state is rounded to float32 where it enters
 *           the net.
 *   attempts      int32 [n]: the attempts the row made, accepted plus rejected
 *   max_attempts  1 .. FC_CNF_DOPRI5_MAX_ATTEMPTS (hipErrorInvalidValue otherwise).  A row that has made
 *           max_attempts attempts without reaching t1, whose error ratio is not finite, or whose step no longer
 *           moves t stops at once and returns NaN in z_out and logp_out: the kernel cannot raise.
 *   evals         max-reduces (2 + 6 attempts) over the rows (1 + 6 attempts with first_step) into *evals.
 *           logp NULL means zeros.  atol, rtol >= 0, not both 0; t0, t1 finite.  z != z_out. */
#define FC_CNF_DOPRI5_MAX_ATTEMPTS 4096
int fc_cnf_dopri5(const float* z, const float* logp, const float* image, float* z_out, float* logp_out,
                  int32_t* attempts, float* evals, int64_t n, int32_t d, int32_t layers, const int32_t* hidden,
                  int32_t layer_kind, int32_t activation, int32_t residual, float scale_output, float p0,
                  int32_t image_floats, double t0, double t1, double atol, double rtol, double first_step,
                  int32_t max_attempts, void* stream);

/* Training: one evaluation of the ODE function as an autograd node (same net description as above, at most
 * FC_CNF_TRAIN_MAX_HIDDEN_LAYERS hidden layers; hipErrorInvalidValue otherwise).
 * fc_cnf_field_train     e NULL: fc_cnf_field's kernel (the exact divergence).  e float32 [n, d]: Hutchinson's estimate
 *           negdiv = -(scale_output e^T (d net / dy) e  (- d with residual)) from a group of 2 lanes per row, the
 *           value stream and one tangent stream seeded with e.  Adds 1 to *evals.
 * fc_cnf_field_backward  from g_dy [n, d] and g_negdiv [n], the forward recomputed in the kernel: g_y [n, d] and
 *           g_image [image_floats], the gradient of every image entry in the image's own layout (padding entries
 *           zero; the vectors a layer kind does not have receive the gradient their zeros would have).  e as in the
 *           forward call; it gets no gradient.  The sums over rows are float64, in a fixed order inside a block, then
 *           over the blocks' partial images in block order (a second kernel): no atomics, bitwise reproducible.
 *           workspace: at least fc_cnf_field_backward_workspace(...) floats, 8-byte aligned.
 * fc_cnf_field_backward_rows       rows a block of the backward kernel carries (-1 outside the limits)
 * fc_cnf_field_backward_workspace  floats of workspace for n rows (-1 outside the limits) */
#define FC_CNF_TRAIN_MAX_HIDDEN_LAYERS 3
int fc_cnf_field_train(const float* y, const float* e, const float* image, float* dy, float* negdiv, float* evals,
                       int64_t n, int32_t d, int32_t layers, const int32_t* hidden, int32_t layer_kind,
                       int32_t activation, int32_t residual, float scale_output, float p0, int32_t image_floats,
                       float t, const float* t_dev, void* stream);
int fc_cnf_field_backward(const float* y, const float* e, const float* image, const float* g_dy,
                          const float* g_negdiv, float* g_y, float* g_image, void* workspace, int64_t n, int32_t d,
                          int32_t layers, const int32_t* hidden, int32_t layer_kind, int32_t activation,
                          int32_t residual, float scale_output, float p0, int32_t image_floats, float t,
                          const float* t_dev, void* stream);
int fc_cnf_field_backward_rows(int32_t d, int32_t layers, const int32_t* hidden, int32_t with_e);
int fc_cnf_field_backward_workspace(int64_t n, int32_t d, int32_t layers, const int32_t* hidden, int32_t with_e);

/* Training: a whole fixed-step solve as an autograd node (the nets of fc_cnf_field_train, the step sequence of
 * fc_cnf_integrate: stage i of step s at t0 + s h + a_i h, h = (t1 - t0) / steps; t1 < t0 integrates backwards).
 * fc_cnf_integrate_train     fc_cnf_integrate with e as in fc_cnf_field_train (NULL: the exact divergence; float32
 *           [n, d]: Hutchinson's estimate with that one e in every evaluation) and an optional tape, float32
 *           [steps * stages, n, d]: tape[s * stages + i][row] is the float32 state stage i of step s handed to the net.
 *           NULL stores nothing.  With e NULL and tape NULL the outputs are bitwise fc_cnf_integrate's.  Max-reduces
 *           steps * stages into *evals.  z != z_out.
 * fc_cnf_integrate_backward  from the tape, e as in the forward call, g_z_out [n, d] and g_logp_out [n]: g_z [n, d] and
 *           g_image [image_floats] (laid out and summed as fc_cnf_field_backward does, over the rows and over the
 *           evaluations of a row in reverse order), the exact gradient of the solve that wrote the tape.  The
 *           gradient of logp is g_logp_out itself.  The adjoint of the state is carried in float64 and rounded to
 *           float32 where it enters an evaluation's backward.  No atomics, bitwise reproducible; g_z of a row does not
 *           depend on the other rows.  workspace: at least fc_cnf_integrate_backward_workspace(...) floats, 8-byte
 *           aligned.  The rows a block carries are fc_cnf_field_backward_rows(...).
 * fc_cnf_integrate_backward_workspace  floats of workspace for n rows (-1 outside the limits) */
int fc_cnf_integrate_train(const float* z, const float* logp, const float* e, const float* image, float* z_out,
                           float* logp_out, float* tape, float* evals, int64_t n, int32_t d, int32_t layers,
                           const int32_t* hidden, int32_t layer_kind, int32_t activation, int32_t residual,
                           float scale_output, float p0, int32_t image_floats, double t0, double t1, int32_t steps,
                           int32_t method, void* stream);
int fc_cnf_integrate_backward(const float* tape, const float* e, const float* image, const float* g_z_out,
                              const float* g_logp_out, float* g_z, float* g_image, void* workspace, int64_t n,
                              int32_t d, int32_t layers, const int32_t* hidden, int32_t layer_kind, int32_t activation,
                              int32_t residual, float scale_output, float p0, int32_t image_floats, double t0,
                              double t1, int32_t steps, int32_t method, void* stream);
int fc_cnf_integrate_backward_workspace(int64_t n, int32_t d, int32_t layers, const int32_t* hidden, int32_t with_e);

/* ---- batch-shared point-wise affine maps ---------------------------------------------------- */
/* x, y viewed as [n, m] (m = elements of one batch item); scale/shift have 1 or m entries.
 * mode 0: y = x*scale + shift                    (standard.py:54-60, normalization.py:171-187)
 * mode 1: y = (x - shift)/scale                  (standard.py:62-68, normalization.py:189-204)
 * mode 2: y = weight*((x - mean)/scale) + shift  (BatchNorm eval forward, normalization.py:98-118;
 *         scale = sqrt(var + eps), shift = bias; aux_mean/aux_weight have m entries)
 * mode 3: y = scale*((x - shift)/weight) + mean  (BatchNorm eval inverse, normalization.py:120-141)
 * The logabsdet of these maps is a per-call constant the host computes, as in the reference. */
int fc_pointwise_affine(const float* x, float* y, const float* scale, const float* shift,
                        const float* aux_mean, const float* aux_weight, int64_t n, int64_t m,
                        int32_t scale_len, int32_t shift_len, int32_t mode, void* stream);

/* ---- element-wise non-linearities -------------------------------------------------------------- */
#define FC_EW_EXP 0              /* nonlinearities.py:18-32 */
#define FC_EW_TANH 1             /* :35-48 */
#define FC_EW_LOGTANH 2          /* :51-112   p0 cut_point, p1 alpha, p2 beta, p3 tanh(cut_point) */
#define FC_EW_LEAKY_RELU 3       /* :115-136  p0 slope, p1 1/slope, aux[0] = log_negative_slope */
#define FC_EW_SIGMOID 4          /* :139-169  p0 eps, aux[0] = temperature */
#define FC_EW_SOFTPLUS 5         /* :172-189  p0 threshold, p1 eps */
#define FC_EW_CAUCHY_CDF 6       /* :212-231 */
#define FC_EW_EXTENDED_SOFTPLUS 7 /* :519-552 aux[m] = raw shift; logabsdet_elem = log diag-jacobian */
#define FC_EW_GLU 8              /* :197-209  aux[n, m] = context; gate = sigmoid(context) */

/* x, y viewed as [n, m].  logabsdet_row[i] = sum over the m elements of row i (NULL to skip);
 * logabsdet_elem [n, m] receives the un-summed values (NULL to skip).  Domain violations of the
 * inverses OR FC_ERR_OUTSIDE_DOMAIN into err_flag (InputOutsideDomain, nonlinearities.py:26,43,158,224). */
int fc_elementwise(const float* x, float* y, float* logabsdet_row, float* logabsdet_elem,
                   const float* aux, uint32_t* err_flag, int64_t n, int64_t m, int32_t kind,
                   int32_t inverse, float p0, float p1, float p2, float p3, void* stream);

/* ---- sum of sigmoids ------------------------------------------------------------------------ */
/* Monotone bijector y = sum_k w_k sigmoid(a_k (x - s_k)) / sum_k w_k + extended_softplus(x) - offset
 * with per-(sample, dim) raw rows [S shift | S log_scale | S raw_softmax | 1 softplus shift]
 * (rowlen = d_t * (3S + 1)); logabsdet = sum_j logaddexp(log-jac sigmoids, log-jac softplus).
 * inverse != 0: x = f^-1(y + offset): per-element bracket from [-lim, lim], then a safeguarded Newton search inside the
 * bracket (at most `bisection_iterations` steps; it converges in 5-9 where the reference's bisection spends all 50),
 * then the reference's 2 closing Newton steps; logabsdet = -log f'(x).  A NEGATIVE `bisection_iterations` runs the
 * reference's plain bisection with that many steps instead (A/B measurements only).
 * Replaces SumOfSigmoids.forward (adaptive_sigmoids.py:108-142) with ExtendedSoftplus
 * (nonlinearities.py:519-552), MonotonicTransform.inverse (no_analytic_inv/base.py:23-103) and
 * MaskedSumOfSigmoidsTransform._elementwise_{forward,inverse} (autoregressive.py:301-318). */
int fc_sum_of_sigmoids(const float* x, float* y, const float* params, const int32_t* cols,
                       float* logabsdet, uint32_t* err_flag, int64_t n, int32_t d, int32_t d_t,
                       int32_t n_sigmoids, int32_t inverse, int32_t bisection_iterations,
                       float bisection_lim, float offset, float log_scale_postact,
                       int32_t shared_params, int32_t lad_mode, void* stream);

/* fc_made_inverse for the sum-of-sigmoids layer: the D passes of MaskedSumOfSigmoidsTransform.inverse
 * (autoregressive.py:266-318) in ONE kernel.  z, y, logabsdet, the hidden-stack image, the final-layer fragments,
 * units_needed, err_flag, n % 16 == 0, d <= 64 and num_blocks <= 3 mean what they mean for fc_made_inverse, with
 * params_per_dim = 3 n_sigmoids + 1 <= 96 (PT <= 6 parameter tiles: n_sigmoids <= 31, the reference's default is 30).  Pass c
 * hands the raw final-layer rows of dim c to one lane per sample, which derives the parameters in place and runs the
 * numerical inverse exactly as fc_sum_of_sigmoids does with the same bisection_iterations, bisection_lim, offset (the AR
 * layer: 0.5) and log_scale_postact.  lad_flags: FC_RQ_ACCUMULATE_LOGABSDET or 0.  d > 32 with num_blocks == 3 and more
 * than 80 parameters per dim exceeds the 160 KB of LDS; that and every other shape out of range return
 * hipErrorInvalidValue.  Added under ABI version 3 (it changes no existing entry). */
int fc_made_inverse_sos(const float* z, float* y, float* logabsdet, const void* hidden_frag, const float* hidden_unscale,
                        const float* hidden_bias, const void* final_frag, const float* final_unscale, const float* final_bias,
                        const int32_t* units_needed, uint32_t* err_flag, int64_t n, int32_t d, int32_t num_blocks,
                        int32_t n_sigmoids, int32_t bisection_iterations, float bisection_lim, float offset,
                        float log_scale_postact, int32_t lad_flags, void* stream);

/* Backward of fc_sum_of_sigmoids in the forward direction, all d columns transformed, per-sample rows (what
 * torch.autograd yields for adaptive_sigmoids.py:108-142 + nonlinearities.py:519-552): grad_x [n, d] and grad_params
 * [n, d * (3S + 1)] from grad_y [n, d] and grad_logabsdet [n] (NULL = zeros); closed-form derivatives, the chain through
 * tanh / sigmoid / the renormalised softmax / softplus included. */
int fc_sum_of_sigmoids_backward(const float* x, const float* params, const float* grad_y,
                                const float* grad_logabsdet, float* grad_x, float* grad_params, int64_t n, int32_t d,
                                int32_t n_sigmoids, float log_scale_postact, void* stream);

/* ---- deep sigmoidal flow ----------------------------------------------------------------------- */
/* Monotone bijector of Neural Autoregressive Flows with per-(sample, dim) raw rows [S raw_a | S raw_b | S raw_w]
 * (rowlen = d_t * 3S).  With r = prescale * raw:  a_k = softplus(r_a_k) (1 - mollify) + mollify,
 * b_k = r_b_k (1 - mollify), w = softmax(r_w), pre_k = a_k x + b_k, s = sum_k w_k sigmoid(pre_k),
 * c = (1 - eps) s + eps / 2 (1 - c is formed from sum_k w_k sigmoid(-pre_k), not by subtraction):
 *   y = log c - log(1 - c)
 *   logabsdet = sum_j [logsumexp_k(log w_k + log a_k + logsigmoid(pre_k) + logsigmoid(-pre_k)) - 2 eps + log(1 - eps)
 *                      - log c - log(1 - c)]          (the -2 eps is the reference's: its logsigmoid carries -eps)
 * inverse != 0: x = f^-1(y) per element: |y| >= log((1 - eps / 2) / (eps / 2)) (the range of the map; eps as the
 * float passed in) sets the outside-domain bit; otherwise a bracket doubled out from [-lim, lim], a safeguarded Newton
 * search on f(x) = y (at most `inverse_iterations` steps), two closing Newton steps; logabsdet = -logabsdet_f(x); a
 * non-finite result sets the non-finite bit.  prescale multiplies every raw value first (1 for DeepSigmoid, 0.2 for the
 * MADE form).  cols / shared_params / lad_mode / err_flag as for fc_sum_of_sigmoids.
 * Replaces DeepSigmoidModule.forward_given_params (adaptive_sigmoids.py:177-210) and
 * MaskedDeepSigmoidTransform._elementwise_forward (autoregressive/deep_sigmoid.py:69-72); the reference has no inverse. */
int fc_deep_sigmoid(const float* x, float* y, const float* params, const int32_t* cols, float* logabsdet,
                    uint32_t* err_flag, int64_t n, int32_t d, int32_t d_t, int32_t n_sigmoids, int32_t inverse,
                    int32_t inverse_iterations, float inverse_lim, float mollify, float eps, float prescale,
                    int32_t shared_params, int32_t lad_mode, void* stream);

/* Backward of fc_deep_sigmoid in the forward direction, all d columns transformed: grad_x [n, d] and grad_raw from
 * grad_y [n, d] and grad_logabsdet [n] (NULL = zeros); closed-form derivatives, the chain through softplus, the mollifier,
 * the softmax and the pre-scale included.
 * shared_params == 0: raw and grad_raw are [n, d * 3S].
 * shared_params != 0: raw is one row [d * 3S]; its gradient is summed over the batch inside the kernel (workgroup
 * partial sums, then a second kernel: no atomics, bit-identical from run to run).  grad_raw must then hold
 * (1 + fc_deep_sigmoid_backward_rows(n, d, S)) * d * 3S floats: the first d * 3S receive the gradient, the rest is
 * workspace.  Returns hipErrorInvalidConfiguration when fc_deep_sigmoid_backward_rows is 0. */
int fc_deep_sigmoid_backward(const float* x, const float* raw, const float* grad_y, const float* grad_logabsdet,
                             float* grad_x, float* grad_raw, int64_t n, int32_t d, int32_t n_sigmoids, float mollify,
                             float eps, float prescale, int32_t shared_params, void* stream);

/* Workspace rows of the shared-row mode above (a count, not an error code); 0: the row does not fit the reduction's
 * LDS plan, expand it to per-sample rows instead. */
int fc_deep_sigmoid_backward_rows(int64_t n, int32_t d, int32_t n_sigmoids);

/* ---- launch route of the tile bijectors ---------------------------------------------------------- */
/* What fc_affine, fc_rq_spline (its LDS-tile path), fc_sum_of_sigmoids, fc_piecewise_spline and fc_deep_sigmoid launch
 * for a batch of n rows of d floats with d_t transformed columns and `rowlen` parameter floats per row (d_t times the
 * entry's parameters per dim), decided by the very host function those entries call.  aligned16: whether x, y and params
 * are all 16-byte aligned.  Touches no device and makes no HIP call.  out[8]:
 *   out[0]  persistent prefetching launch over the full tiles: 0 none, 1 the <6, 1> instance (up to 6 parameter and 1
 *           input float4 per thread and tile), 2 the <8, 2> instance
 *   out[1]  its samples per tile S          out[2]  its number of full tiles
 *   out[3]  rows left over after it (< S; 0 without a persistent launch)
 *   out[4]  one-tile-per-workgroup launch (everything without a persistent launch, else the leftover rows):
 *           0 none, 1 the 16-byte vector copy kernel, 2 the scalar copy kernel
 *   out[5]  its S      out[6]  its grid      out[7]  its block
 * Returns 0, hipErrorInvalidValue for a shape the entries refuse, or hipErrorInvalidConfiguration where a single row
 * exceeds the LDS plan -- what the entries return for that shape before they launch.  n == 0: 0 with nothing to launch.
 * Added under ABI version 3 (it changes no existing entry). */
int fc_tile_route(int64_t n, int32_t d, int32_t d_t, int32_t rowlen, int32_t shared_params, int32_t aligned16,
                  int64_t* out);

/* ---- launch route of the hidden-stack kernels ----------------------------------------------------- */
/* What fc_resnet_hidden / fc_resnet_hidden_packed (FC_ROUTE_HIDDEN), fc_resnet_hidden_context (FC_ROUTE_HIDDEN_GLU,
 * FC_ROUTE_HIDDEN_ADDITIVE), fc_affine_coupling_resnet (FC_ROUTE_COUPLING_TAIL) and fc_resnet_hidden_wide
 * (FC_ROUTE_HIDDEN_WIDE) launch for n rows of d floats, decided by the very host functions those entries call.  The
 * arguments are those of the entry: in_features identity columns, context_features (0 for the kinds without a context),
 * num_blocks, hidden (64; 128 or 256 for the wide kernel).  No kernel runs; the only device query is the CU count of the
 * current device (256 without one).  out[8]:
 *   out[0]  16-row blocks a wave pushes through the layers together: 1 or 2 (wide kernel: the 4 blocks of a 64-row tile)
 *   out[1]  coupling tail: 16-byte pieces of a 16-row chunk of x per lane (8 at one block per wave; 2 at d <= 32 and 4 at
 *           d <= 64 at two), 0 for the other kinds
 *   out[2]  grid (512-thread workgroups)      out[3]  waves = 8 grid
 *   out[4]  dynamic LDS bytes per workgroup
 *   out[5]  passes: the largest number of groups of out[0] blocks any wave walks (wide kernel: tiles any workgroup walks)
 *   out[6]  1 where the last group repeats a block (two blocks per wave, odd number of blocks)
 *   out[7]  the return value
 * Returns 0, hipErrorInvalidValue for a shape the entry refuses, or hipErrorInvalidConfiguration where the LDS of the
 * route exceeds 160 KB -- what the entry returns for that shape before it launches.  n == 0: 0 with nothing to launch.
 * Added under ABI version 3 (it changes no existing entry). */
#define FC_ROUTE_HIDDEN 0
#define FC_ROUTE_HIDDEN_GLU 1
#define FC_ROUTE_HIDDEN_ADDITIVE 2
#define FC_ROUTE_COUPLING_TAIL 3
#define FC_ROUTE_HIDDEN_WIDE 4
int fc_hidden_route(int32_t kind, int64_t n, int32_t d, int32_t in_features, int32_t context_features,
                    int32_t num_blocks, int32_t hidden, int64_t* out);

/* ---- unconstrained monotonic neural networks (Clenshaw-Curtis integral of an MLP) --------------- */
/* z[n, j] = h[n, j, 0] + int_0^x f(t, h[n, j, :]) dt with f = ELU(MLP(t, h)) + 1 and the quadrature
 *   z = h_0 + (x / 2) sum_i w_i f((x / 2)(s_i + 1), h),  s_i = cos(i pi / nb_steps), i = 0..nb_steps,
 * jac[n, j] = f(x, h) at the x of the element, logabsdet[n] = sum_j log jac[n, j].  One matrix-core kernel: no
 * intermediate of size n * d * nb_steps exists.  Replaces MonotonicNormalizer.forward / inverse_transform
 * (transforms/UMNN/MonotonicNormalizer.py:51-82) with the third-party NeuralIntegral restated, and the jac.log().sum(1)
 * of its three callers (autoregressive.py:251-261, coupling.py:187-203, conditional.py:593-603).
 *   x       [n, d]; h [n, d, cond_size], 1 <= cond_size <= FC_UMNN_MAX_COND, all of it (element 0 included) feeds f
 *   MLP     Linear(1 + cond_size -> w_1) ReLU ... Linear(w_L -> 1), L = hidden_layers in 1..FC_UMNN_MAX_HIDDEN_LAYERS,
 *           widths <= 64 (zero-padded to 64), given as an image in two parts:
 *   w_frag  f16, 16-byte aligned: v_mfma_f32_16x16x32_f16 A fragments [layer][k-step][tile][piece (hi, lo)][lane][8] of
 *           the first layer (64 x 32, one k-step: column 0 -- the weight of t -- ZEROED, columns 1..cond_size the
 *           embedding) and of the L - 1 hidden 64 x 64 layers (two k-steps); each layer scaled by a power of two that
 *           lifts its largest entry into [2^14, 2^15); tile t, row 4 g + r holds unit 32 (t >> 1) + 8 g + 4 (t & 1) + r
 *   aux     f32 [64 L + 128 + 4 + 2 FC_UMNN_POINTS]: biases of the L fragment layers, [g][4 t + r] order; the first
 *           layer's t column and the last layer's row in the same order; the L inverse scales (padded to 3) and the last
 *           bias; the tables (s_i + 1) / 2 continued with 1 and w_i continued with 0
 * inverse != 0: x is the target z; per element a Newton search with f as the slope inside [0, 20] or [-20, 0] (F(0) = h_0
 * picks the side), stopping at a step below 2^-23 max(|x|, 1, 4 max(|z|, |h_0|) / f); a target beyond F(+-20) returns +-20 (the reference:
 * 25 bisections of [-20, 20], MonotonicNormalizer.py:67-82); y = the root, jac = f there, logabsdet = -sum log jac.
 * lad_mode as above, applied to that sign; logabsdet may be NULL.  x != y.  A row's results do not depend on its position
 * in the batch.  hipErrorInvalidValue for shapes outside the limits. */
#define FC_UMNN_MAX_COND 31
#define FC_UMNN_MAX_HIDDEN_LAYERS 3
#define FC_UMNN_MAX_STEPS 63
#define FC_UMNN_POINTS 68
int fc_umnn(const float* x, const float* h, const void* w_frag, const float* aux, float* y, float* jac,
            float* logabsdet, int64_t n, int32_t d, int32_t cond_size, int32_t hidden_layers, int32_t nb_steps,
            int32_t inverse, int32_t lad_mode, void* stream);

/* Backward of fc_umnn with the integrand recomputed in the kernel (Leibniz' rule: the limits of the quadrature are
 * constants, dz/dx = jac).  The caller folds logabsdet's gradient into jac's: grad_jac = gjac +- glad / jac.
 *   inverse == 0: x is the forward call's input, grad_out = gz; grad_in = gx = gz jac + grad_jac df/dt(x, h)
 *   inverse != 0: x is the ROOT the inverse call returned, grad_out = gx; grad_in = gz = (gx + grad_jac df/dt(x, h)) / jac,
 *                 and h / the parameters receive the implicit-function gradient through F(x) = z
 *   grad_h  [n, d, cond_size]
 *   w_frag, aux  the image of fc_umnn
 *   wt_frag f16, 16-byte aligned: the same fragment packing applied to the TRANSPOSED weights -- the L - 1 hidden layers
 *           (W_l^T, 64 x 64, [k-step][tile][piece][lane][8], rows in the unit order above), then W1[:, 1:]^T with slot 0
 *           zero (32 x 64: two tiles, tile t row 4 g + r holds input slot 8 g + 4 t + r); each shares the power-of-two
 *           scale of its layer in w_frag
 *   grad_params f32 [64 * 32 + (L - 1) * 64 * 64 + 64 L + 64 + 4], natural unit order, widths zero-padded to 64:
 *           gW1 [64][32] (column 0: t, columns 1..: the embedding), gW_l [L - 1][64][64], gb [L][64], the last layer's
 *           row [64], the last bias [1] (+ 3 of padding).  WRITTEN, not accumulated.
 *   workspace f32, fc_umnn_backward_workspace(n, d, hidden_layers) entries: per-workgroup partial sums.
 * Two launches: the recompute + backward, then a fixed-order sum of the workspace rows -- no atomics; grad_params are
 * bit-identical from run to run, grad_in and grad_h of a row do not depend on its position in the batch.  Limits and
 * errors as fc_umnn. */
int fc_umnn_backward(const float* x, const float* h, const void* w_frag, const float* aux, const void* wt_frag,
                     const float* grad_out, const float* grad_jac, float* grad_in, float* grad_h, float* grad_params,
                     float* workspace, int64_t n, int32_t d, int32_t cond_size, int32_t hidden_layers, int32_t nb_steps,
                     int32_t inverse, void* stream);

/* float32 entries of fc_umnn_backward's workspace on the current device (a count, not an error code; -1: outside the
 * limits). */
int fc_umnn_backward_workspace(int64_t n, int32_t d, int32_t hidden_layers);

/* ---- row-per-wavefront bijectors with dense parameters (d <= 512) ------------------------------ */
/* K Householder reflections out -= (out.q_k)(2/|q_k|^2) q_k, k = 0..K-1 (reverse != 0: K-1..0).
 * q: [K, d] shared, or [n, K, d] when per_sample != 0.  logabsdet is identically 0.
 * Replaces _apply_batchwise_transforms[_nodet] (transforms/orthogonal.py:144-194) behind
 * HouseholderSequence / ParametrizedHouseHolder forward/inverse (orthogonal.py:63-141). */
int fc_householder(const float* x, float* y, const float* q, int64_t n, int32_t d,
                   int32_t num_transforms, int32_t per_sample, int32_t reverse, void* stream);

/* y = x + u_hat * tanh(x.w + b); logabsdet = log(1e-7 + |1 + sum_j u_hat_j (1 - tanh^2) w_j|).
 * u_hat is the constrained u (host computes it from w, u: a [1, d] expression); b is a device scalar.
 * per_sample != 0: w, u_hat are [n, d] and b is [n] (ConditionalPlanarTransform, conditional.py:824-838).
 * Replaces PlanarTransform.forward / forward_logabsdet (no_analytic_inv/planar.py:30-49). */
int fc_planar(const float* x, float* y, float* logabsdet, const float* w, const float* u_hat,
              const float* b, int64_t n, int32_t d, int32_t per_sample, void* stream);

/* Backward of fc_planar with batch-shared parameters (per_sample == 0): grad_x [n, d] is written, grad_w [d],
 * grad_u_hat [d] and grad_b [1] are ACCUMULATED (atomic adds of per-wave partial sums: zero them first).
 * grad_logabsdet may be NULL (zeros).  What torch.autograd yields for no_analytic_inv/planar.py:30-49 from u_hat on;
 * the constraint u -> u_hat stays a host-side torch expression on [1, d]. */
int fc_planar_backward(const float* x, const float* grad_y, const float* grad_logabsdet, const float* w,
                       const float* u_hat, const float* b, float* grad_x, float* grad_w, float* grad_u_hat,
                       float* grad_b, int64_t n, int32_t d, void* stream);

/* Backward of fc_householder with batch-shared q [K, d] (per_sample == 0), from the saved OUTPUT y of the forward
 * call (each reflection is its own inverse, so the intermediates are recovered by walking back): grad_x [n, d] is
 * written, grad_q [K, d] is ACCUMULATED (zero it first).  `reverse` as in the forward call.
 * What torch.autograd yields for orthogonal.py:144-194. */
int fc_householder_backward(const float* y, const float* grad_y, const float* q, float* grad_x, float* grad_q,
                            int64_t n, int32_t d, int32_t num_transforms, int32_t reverse, void* stream);

/* Householder - diagonal - Householder linear map with batch-shared parameters, one launch:
 *   y = post + H_b( scale o H_a( x - pre ) )
 * H_a / H_b: the reflections of q_a [ka, d] / q_b [kb, d] in index order (reverse_* != 0: last row first), the
 * arithmetic of fc_householder; scale [d]; pre / post [d] or NULL (zeros).  ka and kb may be 0 (q NULL then);
 * ka + kb <= 4096.  Both directions of SVDLinear (transforms/svd.py:56-95): forward a = orthogonal_2, b = orthogonal_1,
 * scale = diagonal, post = bias; inverse a = orthogonal_1 reversed, b = orthogonal_2 reversed, scale = 1 / diagonal,
 * pre = bias (subtracted before anything else).  The 2 / |q|^2 factors are computed once per workgroup. */
int fc_hdh_linear(const float* x, float* y, const float* q_a, const float* q_b, const float* scale, const float* pre,
                  const float* post, int64_t n, int32_t d, int32_t ka, int32_t kb, int32_t reverse_a, int32_t reverse_b,
                  void* stream);

/* Backward of fc_hdh_linear from its saved OUTPUT y (every stage is invertible: post comes off, H_b is walked back, the
 * row is divided by scale, H_a is walked back).  grad_x [n, d] is written; grad_q_a [ka, d], grad_q_b [kb, d],
 * grad_scale [d], grad_pre [d] (= -sum grad_x) and grad_post [d] (= sum grad_y) are ACCUMULATED (zero them first);
 * grad_pre / grad_post may be NULL.  reverse_* as in the forward call. */
int fc_hdh_linear_backward(const float* y, const float* grad_y, const float* q_a, const float* q_b, const float* scale,
                           const float* post, float* grad_x, float* grad_q_a, float* grad_q_b, float* grad_scale,
                           float* grad_pre, float* grad_post, int64_t n, int32_t d, int32_t ka, int32_t kb,
                           int32_t reverse_a, int32_t reverse_b, void* stream);

/* ---- row-norm bijectors: radial flow and the stereographic unit-vector map (row width <= 512) --- */
/* Radial flow (no_analytic_inv/planar.py:199-211), z0 [d] shared, a and b DEVICE scalars (a = |alpha|,
 * b = softplus(beta) - |alpha|: host-side torch expressions on the parameters, b >= -a).  inverse == 0:
 *   dz = x - z0, r = |dz|, h = b / (a + r), k = -b r / (a + r)^2;  y = x + h dz;
 *   logabsdet = (d - 1) log(1 + h) + log(1 + h + k).
 * inverse != 0 (the reference has none): rho = |y - z0|, r the non-negative root of r^2 + (a + b - rho) r - a rho = 0 --
 * with q = a + b - rho: 2 a rho / (q + sqrt(q^2 + 4 a rho)) for q > 0, (-q + sqrt(q^2 + 4 a rho)) / 2 otherwise --,
 * x = z0 + (y - z0) / (1 + b / (a + r)), logabsdet = minus the forward's at that r.  logabsdet may be NULL.  x != y. */
int fc_radial(const float* x, float* y, float* logabsdet, const float* z0, const float* a, const float* b, int64_t n,
              int32_t d, int32_t inverse, void* stream);

/* Backward of fc_radial's forward direction: grad_x [n, d] is written, grad_z0 [d], grad_a [1] and grad_b [1] are
 * ACCUMULATED (atomic adds of per-wave partial sums: zero them first).  grad_logabsdet may be NULL (zeros).  A row exactly
 * on z0 (r = 0): the reference's autograd yields NaN through the norm's gradient; here the norm's subgradient is taken as
 * 0 and every gradient stays finite. */
int fc_radial_backward(const float* x, const float* grad_y, const float* grad_logabsdet, const float* z0, const float* a,
                       const float* b, float* grad_x, float* grad_z0, float* grad_a, float* grad_b, int64_t n, int32_t d,
                       void* stream);

/* Stereographic map R^d -> S^d (unitvector.py:18-53); d is the R^d side, d + 1 <= 512.  inverse == 0: x [n, d],
 * s = |x|^2, y [n, d + 1] = (2 x, s - 1) / (s + 1), logabsdet = d (log 2 - log1p(s)).  inverse != 0: x [n, d + 1] on the
 * sphere, y [n, d] = x[:d] / (1 - x[d]), logabsdet = -d (log 2 - log1p(|y|^2)); EVERY row with | |x|^2 - 1 | > 1e-4 ORs
 * FC_ERR_OUTSIDE_DOMAIN into err_flag (the reference tests the batch maximum only).  logabsdet and err_flag may be NULL.
 * x != y. */
int fc_unit_vector(const float* x, float* y, float* logabsdet, uint32_t* err_flag, int64_t n, int32_t d, int32_t inverse,
                   void* stream);

/* Backward of fc_unit_vector in either direction: x_or_y is that direction's INPUT ([n, d] forward, [n, d + 1] inverse),
 * grad_out the gradient of its output, grad_logabsdet [n] or NULL (zeros); grad_in (the input's shape) is written. */
int fc_unit_vector_backward(const float* x_or_y, const float* grad_out, const float* grad_logabsdet, float* grad_in,
                            int64_t n, int32_t d, int32_t inverse, void* stream);

/* Element-wise middle of the backward of fc_sylvester with batch-shared parameters (no_analytic_inv/planar.py:144-166):
 * pre [n, d] = R1 Q^T z + b (recomputed by the caller), grad_act_inout [n, d] = gradient wrt tanh(pre) coming from the
 * R2 / Q product, grad_logabsdet [n] or NULL, r_diag_prod [d] = diag R1 * diag R2.  In place: grad_act_inout becomes the
 * gradient wrt pre including the log-determinant's share; grad_bias [d] and grad_r_diag_prod [d] are ACCUMULATED (zero
 * them first).  The matrix products around it are plain GEMMs and the two Householder sequences use
 * fc_householder / fc_householder_backward (flowconductor_amd.ops._SylvesterFunction). */
int fc_sylvester_mid_backward(const float* pre, float* grad_act_inout, const float* grad_logabsdet,
                              const float* r_diag_prod, float* grad_bias, float* grad_r_diag_prod, int64_t n, int32_t d,
                              void* stream);

/* ---- backward with PER-SAMPLE parameters (a hyper-network's output) ------------------------------
 * One wavefront owns one sample row and that sample's parameter block, so a parameter gradient is WRITTEN once per row
 * (nothing to zero first): no batch reduction, no atomics, bitwise reproducible.  d <= 512; n == 0 launches nothing.
 * Added under ABI version 3 (they change no existing entry).
 *
 * fc_linear_per_sample_backward: the four modes of fc_linear_per_sample, m [n, d, d] raw, sp = offdiag_scale,
 * dg_j = softplus(M_jj) + eps.  grad_logabsdet [n] may be NULL (zeros; unused in modes 0 and 1), grad_sp_rows [n] may be NULL.
 *   mode 0 (y = M x):    x_or_out = x;  grad_in = M^T grad_out,  grad_m_ij = grad_out_i x_j
 *   mode 1 (y = M^T x):  x_or_out = x;  grad_in = M grad_out,    grad_m_ij = x_i grad_out_j
 *   mode 2 (y = L U x, logabsdet = sum log dg):  x_or_out = x;  with t = U x, g_t = L^T grad_out:  grad_in = U^T g_t,
 *     grad_m_ij = sp grad_out_i t_j (j < i), sp g_t_i x_j (j > i), (g_t_i x_i + grad_logabsdet / dg_i) sigmoid(M_ii) (j = i),
 *     grad_sp_rows = sum_{j<i} M_ij grad_out_i t_j + sum_{j>i} M_ij g_t_i x_j  (d / d offdiag_scale of this row's terms)
 *   mode 3 (x = U^-1 L^-1 y, logabsdet = -sum log dg):  x_or_out = the saved OUTPUT x;  grad_in = L^-T U^-T grad_out,
 *     grad_m / grad_sp_rows = mode 2's expressions at the input x with upstream -grad_in and -grad_logabsdet.
 *   Modes 0 / 1 write grad_sp_rows = 0.  Modes 2 / 3 read m twice and write grad_m once; d <= 16 runs four samples per
 *   wavefront with the matrix in registers.
 *
 * fc_householder_backward_per_sample: fc_householder_backward with q [n, K, d] indexed per row, from the saved OUTPUT y;
 * grad_q [n, K, d] is written per row and reflection.  num_transforms == 0: grad_x = grad_y (q, grad_q may be NULL).
 *
 * fc_planar_backward_per_sample: fc_planar_backward with w, u_hat [n, d] and b [n] per row (per_sample != 0 of fc_planar);
 * grad_w, grad_u_hat [n, d] and grad_b [n] are written per row.  grad_logabsdet may be NULL (zeros). */
int fc_linear_per_sample_backward(const float* x_or_out, const float* grad_out, const float* grad_logabsdet,
                                  const float* m, float* grad_in, float* grad_m, float* grad_sp_rows, int64_t n, int32_t d,
                                  int32_t mode, float offdiag_scale, float eps, void* stream);

int fc_householder_backward_per_sample(const float* y, const float* grad_y, const float* q, float* grad_x, float* grad_q,
                                       int64_t n, int32_t d, int32_t num_transforms, int32_t reverse, void* stream);

int fc_planar_backward_per_sample(const float* x, const float* grad_y, const float* grad_logabsdet, const float* w,
                                  const float* u_hat, const float* b, float* grad_x, float* grad_w, float* grad_u_hat,
                                  float* grad_b, int64_t n, int32_t d, void* stream);

/* Dense linear maps with batch-shared [d, d] matrices given TRANSPOSED (a_t[j*d + i] = A[i][j]).
 * mode 0: y = A x + bias                        (linear.py:45-52 cached weight; bias may be NULL)
 * mode 1: y = B (A x) + bias, A = U, B = L      (lu.py:56-68, two F.linear)
 * mode 2: y = A^-1 B^-1 (x - bias), A = U upper, B = L unit-lower (lu.py:70-91, solve_triangular)
 * mode 3: y = A (x - bias)                      (linear.py:62-76 cached inverse, A = W^-1: the bias comes off first;
 *                                                b_t unused, bias may be NULL) */
int fc_linear(const float* x, float* y, const float* a_t, const float* b_t, const float* bias,
              int64_t n, int32_t d, int32_t mode, void* stream);

/* Per-sample dense [d, d] matrices M [n, d, d] (row-major, as a hyper-network emits them), d <= 512.
 * mode 0: y = M x                 mode 1: y = M^T x          (ConditionalRotationTransform, conditional.py:374-401)
 * mode 2: y = L (U x), mode 3: y = U^-1 L^-1 x with, as in ConditionalLUTransform (conditional.py:300-346),
 *   L = sp * tril(M, -1) + I,  U = sp * triu(M, 1) + diag(softplus(diag M) + eps),  sp = softplus(scale)
 *   given as `offdiag_scale`; logabsdet (may be NULL) = +/- sum_i log U_ii.
 * HBM-bound: every matrix element is read exactly once, rows coalesced. */
int fc_linear_per_sample(const float* x, float* y, float* logabsdet, const float* m, int64_t n,
                         int32_t d, int32_t mode, float offdiag_scale, float eps, void* stream);

/* Sylvester flow, fused: y = z + Q R2 tanh(R1 Q^T z + bias), Q = num_householder reflections q,
 * logabsdet = sum_j log(1 + (1 - tanh^2(.)_j) * r_diag_prod_j), r_diag_prod = diag(R1)*diag(R2).
 * Shared parameters: r1_t / r2_t are the upper-triangular matrices TRANSPOSED.  per_sample != 0: q [n, M, d],
 * r1_t / r2_t [n, d, d] ROW-MAJOR AND UNTRANSPOSED, as a hyper-network emits them (only the upper triangle of every
 * row is read: half the bytes), bias / r_diag_prod [n, d] (the D-general conditional form, conditional.py:936-953).
 * Replaces SylvesterTransform.forward (no_analytic_inv/planar.py:144-166). */
int fc_sylvester(const float* x, float* y, float* logabsdet, const float* q, const float* r1_t,
                 const float* r2_t, const float* bias, const float* r_diag_prod, int64_t n, int32_t d,
                 int32_t num_householder, int32_t per_sample, void* stream);

/* Inverse of the Sylvester flow's triangular middle with batch-shared parameters, in the coordinates rotated by Q (the
 * reference has no inverse; the caller applies Q^T before and Q after, flowconductor_amd.ops.sylvester_inverse):
 * given c [n, d] = Q^T y, finds v [n, d] with c = v + R2 tanh(R1 v + bias) by back substitution, j = d-1 .. 0:
 *   s = bias_j + sum_{k>j} R1[j][k] v_k,  t = c_j - sum_{k>j} R2[j][k] th_k,
 *   v_j the root of v + r2 tanh(r1 v + s) = t in [t - |r2|, t + |r2|] (r1 = R1[j][j], r2 = R2[j][j], |r1 r2| < 1:
 *   unique), th_j = tanh(r1 v_j + s),
 * by a bracketed Newton search of at most 16 evaluations (the Newton point where it lies in the closed bracket, else
 * the midpoint; stops early once the step no longer changes v), and
 *   logabsdet[n] = -sum_j log(1 + r1_j r2_j (1 - th_j^2)).
 * r1_t / r2_t are the upper-triangular matrices TRANSPOSED (r1_t[k*d + j] = R1[j][k]), as for fc_sylvester.  One lane
 * per row, 64 rows per wavefront, v and th of a wavefront in LDS: d <= 128, anything else returns
 * hipErrorInvalidValue.  A NaN row yields NaN in that row only.  c != v.  Added under ABI version 3 (it changes no
 * existing entry). */
int fc_sylvester_inverse(const float* c, float* v, float* logabsdet, const float* r1_t, const float* r2_t,
                         const float* bias, int64_t n, int32_t d, void* stream);

/* Shared-weight Sylvester flow as two dense products on the matrix cores (planar.py:144-166 with the batch-
 * independent chains folded into W1 = R1 Q^T and W2 = Q R2, both [d, d] row-major):
 *   y = x + W2 tanh(W1 x + bias),  logabsdet[n] = sum_i log(1 + (1 - tanh^2(.)_i) r_diag_prod_i).
 * d % 32 == 0, d <= 128, n % 16 == 0, x / y / w1 / w2 16-byte aligned.  Products: three-term scaled f16 splits. */
int fc_sylvester_mm(const float* x, float* y, float* logabsdet, const float* w1, const float* w2,
                    const float* bias, const float* r_diag_prod, int64_t n, int32_t d, void* stream);

/* y = W x + bias for a batch-independent dense [d, d] matrix on the matrix cores (same split-f16 products):
 * LULinear / Linear forward with W = L U (lu.py:56-68, linear.py:45-60), a HouseholderSequence folded into its
 * orthogonal matrix (orthogonal.py:63-85).  bias may be NULL.  d % 32 == 0, d <= 128, n % 16 == 0; x / y / w 16-byte aligned. */
int fc_dense_mm(const float* x, float* y, const float* w, const float* bias, int64_t n, int32_t d, void* stream);

/* y = W (x - pre) + post: fc_dense_mm with a shift subtracted from every row in f32 before the product (LULinear's
 * inverse U^-1 L^-1 (x - bias) with W = W^-1 formed once, lu.py:70-91; W^-1 x - W^-1 bias would cancel when the bias
 * dominates).  pre / post may be NULL; the same shape and alignment rules as fc_dense_mm. */
int fc_dense_mm_shifted(const float* x, float* y, const float* w, const float* pre, const float* post, int64_t n,
                        int32_t d, void* stream);

/* ---- weight packing on the device ------------------------------------------------------------------------- */
/* f32 nn.Linear tensors -> the scaled two-piece f16 matrix-core fragments the kernels above take (w_frag / wt_frag),
 * their power-of-two unscale factors and the packed biases: one workgroup per scale group, one launch per weight set
 * (training re-packs every step).  `jobs` is a DEVICE array of fc_pack_job. */
#define FC_PACK_FINAL 0      /* fc_rq_spline_fused_general w_frag + bias_pad of one group of 4 dims */
#define FC_PACK_FINAL_T 1    /* fc_rq_fused_linear_backward wt_frag of one group */
#define FC_PACK_HIDDEN 2     /* fc_resnet_hidden_backward w_frag + bias_acc of one layer */
#define FC_PACK_HIDDEN_T 3   /* its wt_frag of one hidden layer */
#define FC_PACK_HIDDEN_T0 4  /* its wt_frag of the initial layer (W0^T) */
typedef struct fc_pack_job {
  const float* w;       /* source matrix [rows, cols], row-major */
  const float* b;       /* source bias or NULL */
  void* frag;           /* f16 fragments of this group: [nks * nt][2 pieces][64 lanes][8] */
  float* unscale;       /* 2^-S of this group */
  float* bias_out;      /* packed bias or NULL */
  int32_t rows, cols;   /* valid extent of w (everything outside reads as 0) */
  int32_t mode;         /* FC_PACK_* */
  int32_t p, pp;        /* FINAL*: parameters per dim P and its padding 4T */
  int32_t nks, nt;      /* fragment image [nks][nt] (FINAL_T: [nt hidden tiles][nks k-steps]) */
  int32_t group;        /* FINAL*: group of 4 dims */
} fc_pack_job;
int fc_pack_fragments(const void* jobs, int32_t num_jobs, void* stream);
int fc_pack_job_bytes(void);

/* ---- multi-GPU: the one collective of the path ------------------------------------------------------ */
/* Batch-sharded log_prob (one process per GPU, contiguous row shards, replicated weights) exchanges
 * only {sum of log_prob, row count}: 16 bytes per evaluation.  The reference has no distributed code; these entries
 * are what SURVEY.md 8b names for the N > 1 path.  RCCL is resolved at run time (the process' already loaded
 * librccl.so.1 first); without it these return hipErrorNotSupported.  Return value: 0, a hipError_t, or
 * 10000 + ncclResult_t.
 *   fc_comm_unique_id   rank 0 fills a 128-byte id and hands it to the other ranks by any host channel
 *   fc_comm_init_rank   collective over all ranks; binds the calling thread's CURRENT device to `rank`
 *   fc_allreduce_loglik sum_count: DEVICE pointer to two float64 {sum, count}, reduced in place (sum) across the
 *                       ranks of `comm`, asynchronous on `stream` (ncclAllReduce, RCCL over xGMI)
 *   fc_comm_init_rank_on_device  the same after hipSetDevice(device) in the calling thread (the current device is per
 *                       host thread: use this one when the set-up runs off the thread that owns the device)
 *   fc_comm_destroy     releases the communicator (collective: every rank's outstanding work must have finished)
 *   fc_comm_abort       tears a communicator down without waiting for the other ranks (failed set-up on a peer) */
#define FC_COMM_UNIQUE_ID_BYTES 128
int fc_comm_unique_id(void* id_out128);
int fc_comm_init_rank(void** comm_out, int32_t nranks, const void* id128, int32_t rank);
int fc_comm_init_rank_on_device(void** comm_out, int32_t nranks, const void* id128, int32_t rank, int32_t device);
int fc_comm_destroy(void* comm);
int fc_comm_abort(void* comm);
int fc_allreduce_loglik(double* sum_count, void* comm, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FLOWCON_HIP_H_ */
