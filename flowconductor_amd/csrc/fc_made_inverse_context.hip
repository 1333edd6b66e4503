// fc_made_inverse_context: the D passes of a CONDITIONAL autoregressive inverse in one kernel -- the body of
// fc_made_inverse.h with the additive context terms of made.py:153-162 / 108-118 (kCtx).
#include "fc_made_inverse.h"

extern "C" int fc_made_inverse_context(const float* z, const float* context, float* y, float* logabsdet, const void* hidden_frag,
                                       const float* hidden_unscale, const float* hidden_bias, const void* context_frag,
                                       const float* context_unscale, const float* context_bias, const void* final_frag,
                                       const float* final_unscale, const float* final_bias, const int32_t* units_needed,
                                       uint32_t* err_flag, int64_t n, int32_t d, int32_t context_features, int32_t num_blocks,
                                       int32_t params_per_dim, int32_t kind, const fc_rq_config* cfg, void* stream) {
  if (context_features < 1 || context_features > 32) return hipErrorInvalidValue;
  fc::RQOp<0> op{};
  bool run;
  const hipError_t e = fc::made_inverse_prepare(z, y, logabsdet, hidden_frag, hidden_unscale, hidden_bias, final_frag, final_unscale,
                                                final_bias, n, d, num_blocks, params_per_dim, kind, cfg, op, &run);
  if (e != hipSuccess || !run) return e;
  if (!context || !context_frag || !context_unscale || !context_bias || ((uintptr_t)context_frag & 15u) != 0) return hipErrorInvalidValue;
  fc::MadeInvCtxArgs a{{z, y, logabsdet, static_cast<const fc::f16x8*>(hidden_frag), hidden_unscale, hidden_bias,
                        static_cast<const fc::f16x8*>(final_frag), final_unscale, final_bias, err_flag, units_needed, n / 16, d,
                        params_per_dim, (cfg && (cfg->flags & FC_RQ_ACCUMULATE_LOGABSDET)) ? 1 : 0},
                       context, static_cast<const fc::f16x8*>(context_frag), context_unscale, context_bias, context_features};
  return fc::dispatch_made_inverse(a, op, num_blocks, kind, static_cast<hipStream_t>(stream));
}
