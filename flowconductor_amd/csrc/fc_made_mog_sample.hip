// fc_made_mog_sample: the D passes of a mixture-of-Gaussians MADE's ancestral sampler in one kernel, without a context
// (fc_made_inverse.h with the FC_MADE_MOG column step).
#include "fc_made_inverse.h"

extern "C" int fc_made_mog_sample(const float* normal, const float* uniform, float* x, float* logp, const void* hidden_frag,
                                  const float* hidden_unscale, const float* hidden_bias, const void* final_frag,
                                  const float* final_unscale, const float* final_bias, const int32_t* units_needed, int64_t n,
                                  int32_t d, int32_t num_blocks, int32_t c, float epsilon, void* stream) {
  bool run;
  const hipError_t e = fc::made_mog_prepare(normal, uniform, x, logp, hidden_frag, hidden_unscale, hidden_bias, final_frag,
                                            final_unscale, final_bias, n, d, num_blocks, c, &run);
  if (e != hipSuccess || !run) return e;
  fc::MadeMogArgs a{{normal, x, logp, static_cast<const fc::f16x8*>(hidden_frag), hidden_unscale, hidden_bias,
                     static_cast<const fc::f16x8*>(final_frag), final_unscale, final_bias, nullptr, units_needed, n / 16, d, 3 * c, 0},
                    {uniform, epsilon, c}};
  return fc::dispatch_made_mog(a, num_blocks, static_cast<hipStream_t>(stream));
}
