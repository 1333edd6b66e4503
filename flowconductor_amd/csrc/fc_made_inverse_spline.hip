// fc_made_inverse_spline: the D passes of a piecewise linear / quadratic / cubic autoregressive inverse in one kernel
// (fc_made_inverse.h with the kMiForm column step on the ops of fc_spline_ops.h); the instantiations of each form sit in
// fc_made_inverse_spline_{linear,quadratic,cubic}.hip.
#include "fc_made_inverse.h"

extern "C" int fc_made_inverse_spline(const float* z, float* y, float* logabsdet, const void* hidden_frag,
                                      const float* hidden_unscale, const float* hidden_bias, const void* final_frag,
                                      const float* final_unscale, const float* final_bias, const int32_t* units_needed,
                                      uint32_t* err_flag, int64_t n, int32_t d, int32_t num_blocks, const fc_spline_config* cfg,
                                      int32_t lad_flags, void* stream) {
  if (!cfg || cfg->num_bins < 1 || cfg->num_bins > 48) return hipErrorInvalidValue;
  const int32_t k = cfg->num_bins;
  int32_t per_dim;
  switch (cfg->kind) {
    case FC_SPLINE_LINEAR: per_dim = k; break;
    case FC_SPLINE_QUADRATIC: per_dim = cfg->tails ? 2 * k - 1 : 2 * k + 1; break;
    case FC_SPLINE_CUBIC: per_dim = 2 * k + 2; break;
    default: return hipErrorInvalidValue;
  }
  bool run;
  const hipError_t e = fc::made_form_prepare(z, y, logabsdet, hidden_frag, hidden_unscale, hidden_bias, final_frag, final_unscale,
                                             final_bias, n, d, num_blocks, per_dim, 48, &run);
  if (e != hipSuccess || !run) return e;
  fc::SplineParams q = fc::spline_params_from_config(*cfg);
  q.inverse = 1;
  hipStream_t s = static_cast<hipStream_t>(stream);
#define FC_FORM_ARGS(OP) \
  fc::made_form_args(z, y, logabsdet, hidden_frag, hidden_unscale, hidden_bias, final_frag, final_unscale, final_bias, units_needed, \
                     err_flag, n, d, per_dim, lad_flags, OP)
  switch (cfg->kind) {
    case FC_SPLINE_LINEAR: return fc::dispatch_made_spline_linear(FC_FORM_ARGS(fc::LinearSplineOp{q}), num_blocks, s);
    case FC_SPLINE_QUADRATIC: return fc::dispatch_made_spline_quadratic(FC_FORM_ARGS(fc::QuadraticSplineOp{q}), num_blocks, s);
    default: return fc::dispatch_made_spline_cubic(FC_FORM_ARGS(fc::CubicSplineOp{q}), num_blocks, s);
  }
#undef FC_FORM_ARGS
}
