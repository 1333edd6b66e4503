// fc_made_mog_sample_context: the one-kernel sampler of a CONDITIONAL mixture-of-Gaussians MADE -- fc_made_mog_sample with
// the additive context terms of nn/nde/made.py:274-281 / 190-203 (no activation on the initial layer's term).
#include "fc_made_inverse.h"

extern "C" int fc_made_mog_sample_context(const float* normal, const float* uniform, const float* context, float* x, float* logp,
                                          const void* hidden_frag, const float* hidden_unscale, const float* hidden_bias,
                                          const void* context_frag, const float* context_unscale, const float* context_bias,
                                          const void* final_frag, const float* final_unscale, const float* final_bias,
                                          const int32_t* units_needed, int64_t n, int32_t d, int32_t context_features,
                                          int32_t num_blocks, int32_t c, float epsilon, void* stream) {
  if (context_features < 1 || context_features > 32) return hipErrorInvalidValue;
  bool run;
  const hipError_t e = fc::made_mog_prepare(normal, uniform, x, logp, hidden_frag, hidden_unscale, hidden_bias, final_frag,
                                            final_unscale, final_bias, n, d, num_blocks, c, &run);
  if (e != hipSuccess || !run) return e;
  if (!context || !context_frag || !context_unscale || !context_bias || ((uintptr_t)context_frag & 15u) != 0) return hipErrorInvalidValue;
  fc::MadeMogCtxArgs a{{{normal, x, logp, static_cast<const fc::f16x8*>(hidden_frag), hidden_unscale, hidden_bias,
                         static_cast<const fc::f16x8*>(final_frag), final_unscale, final_bias, nullptr, units_needed, n / 16, d, 3 * c, 0},
                        context, static_cast<const fc::f16x8*>(context_frag), context_unscale, context_bias, context_features},
                       {uniform, epsilon, c}};
  return fc::dispatch_made_mog(a, num_blocks, static_cast<hipStream_t>(stream));
}
