// Deep sigmoidal flow (the element-wise bijector of Neural Autoregressive Flows), forward and numerical inverse, gfx950.
//
// Restates (not copies):
//   flowcon/transforms/adaptive_sigmoids.py:145-235        DeepSigmoidModule.forward_given_params / _forward_logabsdet
//   flowcon/transforms/autoregressive/deep_sigmoid.py      the MADE form: dsparams = made_output / 5, eps = 3e-5
// Row layout per dim: [S raw_a | S raw_b | S raw_w] = 3S raw values.  They are turned into (a, b, w) once, in place in LDS:
//   a_k = softplus(p raw_a_k) (1 - mollify) + mollify,  b_k = p raw_b_k (1 - mollify),  w = softmax(p raw_w)
// (p: the parameter pre-scale, 1 for DeepSigmoid and 0.2 for the MADE form), so the evaluations of the inverse read ready values.
//   pre_k = a_k x + b_k,  s = sum_k w_k sigmoid(pre_k),  t = sum_k w_k sigmoid(-pre_k)
//   c = (1 - eps) s + eps / 2,   1 - c = (1 - eps) t + eps / 2        (formed from t: no cancellation where c -> 1)
//   y = log c - log(1 - c)
//   logabsdet = logsumexp_k(log(w_k a_k) + logsigmoid(pre_k) + logsigmoid(-pre_k)) - 2 eps + log(1 - eps) - log c - log(1 - c)
// The -2 eps is the reference's: its logsigmoid is -(softplus(-t) + eps), twice per term.
// The reference has no inverse (both `inverse` methods raise NotImplementedError); the one here solves f(x) = y per element.
#include <math.h>
#include "fc_tile.h"
#include "fc_math.h"
#include "../../include/flowcon_hip.h"

namespace fc {

struct DeepSigmoidOp {
  static constexpr bool kHasPrepare = true;
  int S;
  int inverse;
  int iterations;      // cap on the root-search steps
  float lim;           // initial bracket half-width
  float mollify;
  float one_m_moll;    // 1 - mollify
  float prescale;
  float one_m_eps;     // 1 - eps
  float half_eps;      // eps / 2
  float lad_const;     // log(1 - eps) - 2 eps
  float bound;         // log((1 - eps / 2) / (eps / 2)): the range of the map is |y| < bound

  __device__ __forceinline__ void prepare(float* __restrict__ prow, int j, int d_t) const {
    float* p = prow + j * (3 * S);
    for (int k = 0; k < S; ++k) p[k] = softplus_lean(p[k] * prescale, 1.f) * one_m_moll + mollify;
    for (int k = 0; k < S; ++k) p[S + k] = (p[S + k] * prescale) * one_m_moll;
    float m = -INFINITY;
    for (int k = 0; k < S; ++k) m = fmaxf(m, p[2 * S + k]);
    float sum = 0.f;
    for (int k = 0; k < S; ++k) {
      const float e = exp_lean((p[2 * S + k] - m) * prescale);      // (prescale > 0: the maximum stays the maximum)
      p[2 * S + k] = e;
      sum += e;
    }
    for (int k = 0; k < S; ++k) p[2 * S + k] = div_lean(p[2 * S + k], sum);
  }

  // value and derivative of f(x) = log c - log(1 - c) for the root search:
  //   f' = (1 - eps) (1 / c + 1 / (1 - c)) sum_k w_k a_k sigmoid'(pre_k)
  __device__ __forceinline__ void value_deriv(const float* __restrict__ p, float x, float& f, float& df) const {
    float s = 0.f, t = 0.f, dacc = 0.f;
    for (int k = 0; k < S; ++k) {
      const float a = p[k], w = p[2 * S + k];
      const float pre = a * x + p[S + k];
      const float e = exp_lean(-fabsf(pre));                 // in [0, 1]
      const float r = div_lean(1.f, 1.f + e);
      const float er = e * r;
      s += w * (pre >= 0.f ? r : er);                        // w sigmoid(pre)
      t += w * (pre >= 0.f ? er : r);                        // w sigmoid(-pre)
      dacc += (w * a) * (er * r);                            // sigmoid'(pre) = e / (1 + e)^2
    }
    const float c = one_m_eps * s + half_eps, q = one_m_eps * t + half_eps;
    f = log_lean(c) - log_lean(q);
    df = (one_m_eps * dacc) * (div_lean(1.f, c) + div_lean(1.f, q));
  }

  // value and log-derivative in ONE pass over the sigmoids: logsumexp with a running maximum (one exponential per term: the
  // partial sum is rescaled when the maximum moves, the term otherwise)
  __device__ __forceinline__ void value_lad(const float* __restrict__ p, float x, float& val, float& lad) const {
    float s = 0.f, t = 0.f, m = -1e30f, se = 0.f;            // (a finite floor: exp_lean(-inf) is not defined)
    for (int k = 0; k < S; ++k) {
      const float a = p[k], w = p[2 * S + k];
      const float pre = a * x + p[S + k];
      const float e = exp_lean(-fabsf(pre));
      const float r = div_lean(1.f, 1.f + e);
      const float er = e * r;
      s += w * (pre >= 0.f ? r : er);
      t += w * (pre >= 0.f ? er : r);
      // logsigmoid(pre) + logsigmoid(-pre) = -|pre| - 2 log1p(exp(-|pre|)); a weight or a scale that underflowed to zero
      // stays a finite, negligible term
      const float lj = log_lean(fmaxf(w * a, 1e-37f)) - fabsf(pre) - 2.f * log1p_lean_pos(e);
      const float d = lj - m;
      const float ex = exp_lean(-fabsf(d));
      se = d > 0.f ? se * ex + 1.f : se + ex;
      m = fmaxf(m, lj);
    }
    const float c = one_m_eps * s + half_eps, q = one_m_eps * t + half_eps;
    const float lc = log_lean(c), lq = log_lean(q);
    val = lc - lq;
    lad = (m + log_lean(se)) + lad_const - (lc + lq);
  }

  __device__ __forceinline__ void eval(const float* __restrict__ prow, int j, int d_t, float x,
                                       float& y, float& lad, uint32_t& err) const {
    const float* p = prow + j * (3 * S);
    if (!inverse) {
      value_lad(p, x, y, lad);
      return;
    }
    const float z = x;
    if (!(fabsf(z) < bound)) {                   // outside the range of the map (NaN included)
      err |= kErrOutsideDomain;
      y = z;
      lad = 0.f;
      return;
    }
    // bracket per element: double the half-width until f(hi) >= z and f(lo) <= z (a bounded number of expansions: where
    // float32 saturates below a target within an ulp of the bound the search ends at the bracket's edge)
    float hi = lim, lo = -lim, fhi, flo, fv, dv;
    for (int it = 0; it < 40; ++it) {
      value_deriv(p, hi, fhi, dv);
      if (!(fhi < z)) break;
      hi *= 2.f;
    }
    for (int it = 0; it < 40; ++it) {
      value_deriv(p, lo, flo, dv);
      if (!(flo > z)) break;
      lo *= 2.f;
    }
    // Safeguarded Newton on f(x) = z in OUTPUT space (f is close to linear between its saturations -- exactly a x + b for
    // S = 1, eps -> 0 -- where s space loses the conditioning): every evaluation tightens the bracket by the sign of f - z; the
    // Newton iterate is taken when it falls strictly inside, the midpoint otherwise.  The start is the chord of the bracket.
    float xg = lo + (z - flo) * div_lean(hi - lo, fhi - flo);
    if (!(xg > lo && xg < hi)) xg = 0.5f * (lo + hi);
    for (int it = 0; it < iterations; ++it) {
      value_deriv(p, xg, fv, dv);
      const float r = fv - z;
      if (r > 0.f) hi = xg;
      else if (r < 0.f) lo = xg;
      else break;
      float xn = xg - div_lean(r, dv);
      if (!(xn > lo && xn < hi)) xn = 0.5f * (lo + hi);
      const bool done = fabsf(xn - xg) <= 2e-7f * fmaxf(1.f, fabsf(xg));
      xg = xn;
      if (done) break;
    }
    // two closing Newton steps, x -= (f - z) / (f' + 1e-7), as the project's other numerical inverses end
#pragma unroll 1
    for (int it = 0; it < 2; ++it) {
      value_deriv(p, xg, fv, dv);
      xg = xg - div_lean(fv - z, dv + 1e-7f);
    }
    float v, l;
    value_lad(p, xg, v, l);
    if (!isfinite(xg) || !isfinite(l)) err |= kErrNonFinite;
    y = xg;
    lad = -l;
  }
};

}  // namespace fc

extern "C" int fc_deep_sigmoid(const float* x, float* y, const float* params, const int32_t* cols, float* logabsdet,
                               uint32_t* err_flag, int64_t n, int32_t d, int32_t d_t, int32_t n_sigmoids,
                               int32_t inverse, int32_t inverse_iterations, float inverse_lim, float mollify, float eps,
                               float prescale, int32_t shared_params, int32_t lad_mode, void* stream) {
  if (n < 0 || d <= 0 || d_t <= 0 || d_t > d || n_sigmoids <= 0 || inverse_iterations < 0) return hipErrorInvalidValue;
  if (!(eps > 0.f && eps < 1.f) || !(mollify >= 0.f && mollify <= 1.f) || !(prescale > 0.f)) return hipErrorInvalidValue;
  if (inverse && !(inverse_lim > 0.f)) return hipErrorInvalidValue;
  if (n > 0 && (!x || !y || !params)) return hipErrorInvalidValue;
  if ((int64_t)d_t * 3 * n_sigmoids > 0x7fffffffLL) return hipErrorInvalidValue;
  fc::DeepSigmoidOp op;
  op.S = n_sigmoids;
  op.inverse = inverse;
  op.iterations = inverse_iterations;
  op.lim = inverse_lim;
  op.mollify = mollify;
  op.one_m_moll = 1.f - mollify;
  op.prescale = prescale;
  const double e = (double)eps;
  op.one_m_eps = (float)(1.0 - e);
  op.half_eps = (float)(0.5 * e);
  op.lad_const = (float)(log1p(-e) - 2.0 * e);
  op.bound = (float)log((1.0 - 0.5 * e) / (0.5 * e));
  fc::TileArgs a{};
  a.x = x; a.y = y; a.params = params; a.cols = cols; a.logabsdet = logabsdet; a.err = err_flag;
  a.N = n; a.D = d; a.d_t = d_t;
  a.rowlen = d_t * 3 * n_sigmoids;
  a.shared_params = shared_params;
  a.lad_mode = lad_mode;
  return fc::launch_tile(op, a, static_cast<hipStream_t>(stream));
}
