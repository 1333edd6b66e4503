// Sum-of-sigmoids monotone bijector (+ extended softplus), forward and numerical inverse, gfx950.
//
// Restates (not copies):
//   flowcon/transforms/adaptive_sigmoids.py:108-142   sum_of_sigmoids / get_params / forward
//   flowcon/transforms/nonlinearities.py:519-552      ExtendedSoftplus
//   flowcon/transforms/no_analytic_inv/base.py:23-83  bracket -> bisection -> 2 Newton steps
// Row layout per dim: [S shift | S log_scale | S raw_softmax | 1 softplus shift] = 3S + 1 raw
// values.  They are turned into derived parameters (10 tanh, 0.1 + 9.9 sigmoid, renormalised
// softmax + 1e-6, softplus + 0.1) once, in place in LDS, so the function evaluations of the inverse (a bracket, a
// safeguarded Newton search: ~8-12 evaluations; the reference spends ~55) read ready values.  The inverse brackets per element (the reference expands one
// batch-global bracket, base.py:46-60, which makes its result depend on batch composition);
// both converge to the same root.
#include "fc_tile.h"
#include "fc_math.h"
#include "../../include/flowcon_hip.h"
#include "fc_sos_op.h"

extern "C" int fc_sum_of_sigmoids(const float* x, float* y, const float* params, const int32_t* cols,
                                  float* logabsdet, uint32_t* err_flag, int64_t n, int32_t d, int32_t d_t,
                                  int32_t n_sigmoids, int32_t inverse, int32_t bisection_iterations,
                                  float bisection_lim, float offset, float log_scale_postact,
                                  int32_t shared_params, int32_t lad_mode, void* stream) {
  if (n < 0 || d <= 0 || d_t <= 0 || d_t > d || n_sigmoids <= 0) return hipErrorInvalidValue;
  if (n > 0 && (!x || !y || !params)) return hipErrorInvalidValue;
  fc::SoSOp op;
  op.S = n_sigmoids;
  op.inverse = inverse;
  op.iterations = bisection_iterations < 0 ? -bisection_iterations : bisection_iterations;
  op.bisect = bisection_iterations < 0 ? 1 : 0;
  op.lim = bisection_lim;
  op.ratio_mult = 1.5f;
  op.offset = offset;
  op.log_post = log_scale_postact;
  fc::TileArgs a{};
  a.x = x; a.y = y; a.params = params; a.cols = cols; a.logabsdet = logabsdet; a.err = err_flag;
  a.N = n; a.D = d; a.d_t = d_t;
  a.rowlen = d_t * (3 * n_sigmoids + 1);
  a.shared_params = shared_params;
  a.lad_mode = lad_mode;
  return fc::launch_tile(op, a, static_cast<hipStream_t>(stream));
}
