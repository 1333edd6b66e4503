// fc_made_mog_sample_context: the one-kernel sampler of a CONDITIONAL mixture-of-Gaussians MADE -- fc_made_mog_sample with
// the additive context terms of nn/nde/made.py:274-281 / 190-203 (no activation on the initial layer's term).
#include "fc_made_inverse.h"

extern "C" int fc_made_mog_sample_context(const float* normal, const float* uniform, const float* context, float* x, float* logp,
                                          const void* hidden_frag, const float* hidden_unscale, const float* hidden_bias,
                                          const void* context_frag, const float* context_unscale, const float* context_bias,
                                          const void* final_frag, const float* final_unscale, const float* final_bias,
                                          const int32_t* units_needed, int64_t n, int32_t d, int32_t context_features,
                                          int32_t num_blocks, int32_t c, float epsilon, void* stream) {
  if (c < 1 || c > fc::kMogMaxComponents || (n != 0 && !uniform)) return hipErrorInvalidValue;
  fc::MadeMogCtxArgs a{{}, {uniform, epsilon, c}};
  bool run;
  hipError_t e = fc::made_args_prepare(a, normal, x, logp, hidden_frag, hidden_unscale, hidden_bias, final_frag, final_unscale,
                                       final_bias, units_needed, nullptr, n, d, num_blocks, 3 * c, 48, false, &run);
  if (e == hipSuccess && !fc::made_context_prepare(a, context, context_frag, context_unscale, context_bias, context_features, run))
    e = hipErrorInvalidValue;
  if (e != hipSuccess || !run) return e;
  return fc::dispatch_made_tiles<1, 3, fc::kMiMog>(a, num_blocks, static_cast<hipStream_t>(stream));
}
