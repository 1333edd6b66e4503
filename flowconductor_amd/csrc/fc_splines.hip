// Piecewise linear / quadratic / cubic spline bijectors (the RQ spline's siblings), gfx950.
//
// Restates (not copies):
//   flowcon/transforms/splines/linear.py:38-105      softmax pdf, uniform bins, cdf by cumsum
//   flowcon/transforms/splines/quadratic.py:55-159   trapezoid-normalised heights, quadratic segments
//   flowcon/transforms/splines/cubic.py:63-267       Steffen-style monotone cubic, Blinn's inverse
// and their `unconstrained_*` wrappers (identity outside [-B, B]).
// Same tile machinery as the RQ kernel; bins are walked with runtime-K loops over LDS.  Each
// op's `prepare` turns the raw conditioner outputs of one (sample, dim) into widths / heights
// in place in LDS, once, so the evaluation passes read ready values.
#include "fc_tile.h"
#include "fc_math.h"
#include "../../include/flowcon_hip.h"
#include "fc_spline_ops.h"

extern "C" int fc_piecewise_spline(const float* x, float* y, const float* params, const int32_t* cols,
                                   float* logabsdet, uint32_t* err_flag, int64_t n, int32_t d, int32_t d_t,
                                   int32_t shared_params, int32_t lad_mode, const fc_spline_config* cfg,
                                   void* stream) {
  if (!cfg || n < 0 || d <= 0 || d_t <= 0 || d_t > d || cfg->num_bins <= 0) return hipErrorInvalidValue;
  if (n > 0 && (!x || !y || !params)) return hipErrorInvalidValue;
  const int per_dim = fc::spline_params_per_dim(cfg->kind, cfg->num_bins, cfg->tails);
  if (per_dim < 0) return hipErrorInvalidValue;
  const fc::SplineParams q = fc::spline_params_from_config(*cfg);

  fc::TileArgs a{};
  a.x = x; a.y = y; a.params = params; a.cols = cols; a.logabsdet = logabsdet; a.err = err_flag;
  a.N = n; a.D = d; a.d_t = d_t;
  a.rowlen = d_t * per_dim;
  a.shared_params = shared_params;
  a.lad_mode = lad_mode;
  hipStream_t s = static_cast<hipStream_t>(stream);
  switch (cfg->kind) {
    case FC_SPLINE_LINEAR: return fc::launch_tile(fc::LinearSplineOp{q}, a, s);
    case FC_SPLINE_QUADRATIC: return fc::launch_tile(fc::QuadraticSplineOp{q}, a, s);
    case FC_SPLINE_CUBIC: return fc::launch_tile(fc::CubicSplineOp{q}, a, s);
    default: return hipErrorInvalidValue;
  }
}
