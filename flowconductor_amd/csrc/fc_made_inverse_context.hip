// fc_made_inverse_context: the D passes of a CONDITIONAL autoregressive inverse in one kernel -- the body of
// fc_made_inverse.h with the additive context terms of made.py:153-162 / 108-118 (kCtx); fc_made_inverse's host path with
// made_context_prepare in it.
#include "fc_made_inverse.h"

extern "C" int fc_made_inverse_context(const float* z, const float* context, float* y, float* logabsdet, const void* hidden_frag,
                                       const float* hidden_unscale, const float* hidden_bias, const void* context_frag,
                                       const float* context_unscale, const float* context_bias, const void* final_frag,
                                       const float* final_unscale, const float* final_bias, const int32_t* units_needed,
                                       uint32_t* err_flag, int64_t n, int32_t d, int32_t context_features, int32_t num_blocks,
                                       int32_t params_per_dim, int32_t kind, const fc_rq_config* cfg, void* stream) {
  fc::RQOp<0> op{};
  if (!fc::made_rq_prepare(kind, params_per_dim, cfg, n, op)) return hipErrorInvalidValue;
  fc::MadeInvCtxArgs a{};
  bool run;
  hipError_t e = fc::made_args_prepare(a, z, y, logabsdet, hidden_frag, hidden_unscale, hidden_bias, final_frag, final_unscale,
                                       final_bias, units_needed, err_flag, n, d, num_blocks, params_per_dim, 48,
                                       n != 0 && cfg && (cfg->flags & FC_RQ_ACCUMULATE_LOGABSDET), &run);
  if (e == hipSuccess && !fc::made_context_prepare(a, context, context_frag, context_unscale, context_bias, context_features, run))
    e = hipErrorInvalidValue;
  if (e != hipSuccess || !run) return e;
  return fc::dispatch_made_inverse(a, op, num_blocks, kind, static_cast<hipStream_t>(stream));
}
