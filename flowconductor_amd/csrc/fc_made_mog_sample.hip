// fc_made_mog_sample: the D passes of a mixture-of-Gaussians MADE's ancestral sampler in one kernel, without a context
// (fc_made_inverse.h with the FC_MADE_MOG column step; its own check: 1 <= c <= 16 components, 3 c parameters per dim).
#include "fc_made_inverse.h"

extern "C" int fc_made_mog_sample(const float* normal, const float* uniform, float* x, float* logp, const void* hidden_frag,
                                  const float* hidden_unscale, const float* hidden_bias, const void* final_frag,
                                  const float* final_unscale, const float* final_bias, const int32_t* units_needed, int64_t n,
                                  int32_t d, int32_t num_blocks, int32_t c, float epsilon, void* stream) {
  if (c < 1 || c > fc::kMogMaxComponents || (n != 0 && !uniform)) return hipErrorInvalidValue;
  fc::MadeMogArgs a{{}, {uniform, epsilon, c}};
  bool run;
  const hipError_t e = fc::made_args_prepare(a, normal, x, logp, hidden_frag, hidden_unscale, hidden_bias, final_frag, final_unscale,
                                             final_bias, units_needed, nullptr, n, d, num_blocks, 3 * c, 48, false, &run);
  if (e != hipSuccess || !run) return e;
  return fc::dispatch_made_tiles<1, 3, fc::kMiMog>(a, num_blocks, static_cast<hipStream_t>(stream));
}
