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
  fc::SplineParams q;
  q.K = cfg->num_bins;
  q.tails = cfg->tails;
  q.inverse = cfg->inverse;
  q.left = cfg->left; q.right = cfg->right; q.bottom = cfg->bottom; q.top = cfg->top;
  q.min_w = (float)cfg->min_bin_width;
  q.min_h = (float)cfg->min_bin_height;
  q.cw = (float)(1.0 - cfg->min_bin_width * q.K);
  q.ch = (float)(1.0 - cfg->min_bin_height * q.K);
  q.w_div = cfg->width_divisor > 0.f ? cfg->width_divisor : 1.f;
  q.h_div = cfg->height_divisor > 0.f ? cfg->height_divisor : 1.f;
  q.eps = cfg->cubic_eps;
  q.quad_thresh = cfg->cubic_quadratic_threshold;

  fc::TileArgs a{};
  a.x = x; a.y = y; a.params = params; a.cols = cols; a.logabsdet = logabsdet; a.err = err_flag;
  a.N = n; a.D = d; a.d_t = d_t;
  a.shared_params = shared_params;
  a.lad_mode = lad_mode;
  hipStream_t s = static_cast<hipStream_t>(stream);
  switch (cfg->kind) {
    case FC_SPLINE_LINEAR: {
      a.rowlen = d_t * q.K;
      return fc::launch_tile(fc::LinearSplineOp{q}, a, s);
    }
    case FC_SPLINE_QUADRATIC: {
      a.rowlen = d_t * (q.tails ? 2 * q.K - 1 : 2 * q.K + 1);
      return fc::launch_tile(fc::QuadraticSplineOp{q}, a, s);
    }
    case FC_SPLINE_CUBIC: {
      a.rowlen = d_t * (2 * q.K + 2);
      return fc::launch_tile(fc::CubicSplineOp{q}, a, s);
    }
    default:
      return hipErrorInvalidValue;
  }
}
