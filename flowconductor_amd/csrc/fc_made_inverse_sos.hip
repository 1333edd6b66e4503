// fc_made_inverse_sos: the D passes of a sum-of-sigmoids autoregressive inverse in one kernel (fc_made_inverse.h with the
// kMiForm column step on SoSOp), up to three parameter tiles (S <= 15); fc_made_inverse_sos_wide.hip holds four to six.
#include "fc_made_inverse.h"

extern "C" int fc_made_inverse_sos(const float* z, float* y, float* logabsdet, const void* hidden_frag, const float* hidden_unscale,
                                   const float* hidden_bias, const void* final_frag, const float* final_unscale,
                                   const float* final_bias, const int32_t* units_needed, uint32_t* err_flag, int64_t n, int32_t d,
                                   int32_t num_blocks, int32_t n_sigmoids, int32_t bisection_iterations, float bisection_lim,
                                   float offset, float log_scale_postact, int32_t lad_flags, void* stream) {
  if (n_sigmoids < 1 || n_sigmoids > 31) return hipErrorInvalidValue;
  fc::MadeFormArgs<fc::SoSOp> a{};
  bool run;
  const hipError_t e = fc::made_args_prepare(a, z, y, logabsdet, hidden_frag, hidden_unscale, hidden_bias, final_frag, final_unscale,
                                             final_bias, units_needed, err_flag, n, d, num_blocks, 3 * n_sigmoids + 1, 96,
                                             lad_flags & FC_RQ_ACCUMULATE_LOGABSDET, &run);
  if (e != hipSuccess || !run) return e;
  fc::SoSOp& op = a.form;      // as fc_sum_of_sigmoids fills it
  op.S = n_sigmoids;
  op.inverse = 1;
  op.iterations = bisection_iterations < 0 ? -bisection_iterations : bisection_iterations;
  op.bisect = bisection_iterations < 0 ? 1 : 0;
  op.lim = bisection_lim;
  op.ratio_mult = 1.5f;
  op.offset = offset;
  op.log_post = log_scale_postact;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (a.P > 48) return fc::dispatch_made_sos_wide(a, num_blocks, s);
  return fc::dispatch_made_tiles<1, 3, fc::kMiForm>(a, num_blocks, s);
}
