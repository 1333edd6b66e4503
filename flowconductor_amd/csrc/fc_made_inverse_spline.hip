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
  const int32_t per_dim = fc::spline_params_per_dim(cfg->kind, cfg->num_bins, cfg->tails);
  if (per_dim < 0) return hipErrorInvalidValue;
  fc::SplineParams q = fc::spline_params_from_config(*cfg);
  q.inverse = 1;
  // the form's unit's dispatcher, behind the shared checks
  auto run = [&](auto op, auto dispatch) -> int {
    fc::MadeFormArgs<decltype(op)> a{{}, op};
    bool rows;
    const hipError_t e = fc::made_args_prepare(a, z, y, logabsdet, hidden_frag, hidden_unscale, hidden_bias, final_frag, final_unscale,
                                               final_bias, units_needed, err_flag, n, d, num_blocks, per_dim, 48,
                                               lad_flags & FC_RQ_ACCUMULATE_LOGABSDET, &rows);
    return (e != hipSuccess || !rows) ? e : dispatch(a, num_blocks, static_cast<hipStream_t>(stream));
  };
  switch (cfg->kind) {
    case FC_SPLINE_LINEAR: return run(fc::LinearSplineOp{q}, fc::dispatch_made_spline_linear);
    case FC_SPLINE_QUADRATIC: return run(fc::QuadraticSplineOp{q}, fc::dispatch_made_spline_quadratic);
    case FC_SPLINE_CUBIC: return run(fc::CubicSplineOp{q}, fc::dispatch_made_spline_cubic);
    default: return hipErrorInvalidValue;
  }
}
