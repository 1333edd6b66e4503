// fc_made_inverse: the D passes of an autoregressive inverse in one kernel, without a context (fc_made_inverse.h).
#include "fc_made_inverse.h"

extern "C" int fc_made_inverse(const float* z, float* y, float* logabsdet, const void* hidden_frag,
                               const float* hidden_unscale, const float* hidden_bias, const void* final_frag,
                               const float* final_unscale, const float* final_bias, const int32_t* units_needed,
                               uint32_t* err_flag, int64_t n, int32_t d, int32_t num_blocks, int32_t params_per_dim, int32_t kind,
                               const fc_rq_config* cfg, void* stream) {
  fc::RQOp<0> op{};
  if (!fc::made_rq_prepare(kind, params_per_dim, cfg, n, op)) return hipErrorInvalidValue;
  fc::MadeInvArgs a{};
  bool run;
  const hipError_t e = fc::made_args_prepare(a, z, y, logabsdet, hidden_frag, hidden_unscale, hidden_bias, final_frag, final_unscale,
                                             final_bias, units_needed, err_flag, n, d, num_blocks, params_per_dim, 48,
                                             n != 0 && cfg && (cfg->flags & FC_RQ_ACCUMULATE_LOGABSDET), &run);
  if (e != hipSuccess || !run) return e;
  return fc::dispatch_made_inverse(a, op, num_blocks, kind, static_cast<hipStream_t>(stream));
}
