// LinearSplineOp / QuadraticSplineOp / CubicSplineOp: one element of a piecewise spline on a parameter row in LDS.
// Shared by the streaming kernels (fc_splines.hip, where the schemes are described), the column step of the
// one-kernel autoregressive inverse (fc_made_inverse.h, kMiForm) and the backward kernel (fc_splines_backward.hip).
//
// The forward direction of each spline is written once as templates over the number type T and instantiated with float
// (the Ops below) and with Dual (fc_dual.h: the backward kernel's forward-mode derivative): `*_prepare`, then
// `linear_spline_forward`, `cubic_bin` + `cubic_spline_forward`, and `quadratic_spline_eval`, which is the quadratic's whole
// element (see there why).  The inverse directions (the linear cdf search, the quadratic's square-root root, Blinn's closed
// form and the Newton polish of the cubic) are float only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>
#include "fc_tile.h"
#include "fc_math.h"
#include "fc_dual.h"
#include "../../include/flowcon_hip.h"

namespace fc {

struct SplineParams {
  int K;
  int tails;       // 0 none, 1 linear
  int inverse;
  float left, right, bottom, top;
  float min_w, min_h;   // float casts of the python floats
  float cw, ch;         // (float)(1 - min_w*K), (float)(1 - min_h*K)
  float w_div, h_div;   // divisors applied to unnormalised widths / heights (1 = off)
  float eps;            // cubic: root-in-bin slack (1e-5)
  float quad_thresh;    // cubic: |a| below this -> quadratic fallback (1e-3)
};

// the host's view of an fc_spline_config
inline SplineParams spline_params_from_config(const fc_spline_config& cfg) {
  SplineParams q;
  q.K = cfg.num_bins;
  q.tails = cfg.tails;
  q.inverse = cfg.inverse;
  q.left = cfg.left; q.right = cfg.right; q.bottom = cfg.bottom; q.top = cfg.top;
  q.min_w = (float)cfg.min_bin_width;
  q.min_h = (float)cfg.min_bin_height;
  q.cw = (float)(1.0 - cfg.min_bin_width * q.K);
  q.ch = (float)(1.0 - cfg.min_bin_height * q.K);
  q.w_div = cfg.width_divisor > 0.f ? cfg.width_divisor : 1.f;
  q.h_div = cfg.height_divisor > 0.f ? cfg.height_divisor : 1.f;
  q.eps = cfg.cubic_eps;
  q.quad_thresh = cfg.cubic_quadratic_threshold;
  return q;
}

// raw parameters per transformed dim (the FC_SPLINE_* row layouts of flowcon_hip.h); negative for an unknown kind
inline int spline_params_per_dim(int kind, int K, int tails) {
  switch (kind) {
    case FC_SPLINE_LINEAR: return K;
    case FC_SPLINE_QUADRATIC: return tails ? 2 * K - 1 : 2 * K + 1;
    case FC_SPLINE_CUBIC: return 2 * K + 2;
    default: return -1;
  }
}

// shared: domain gate + normalisation of the input to [0, 1]
template <class T>
__device__ __forceinline__ bool spline_gate(const SplineParams& q, T x, T& xn, T& y, T& lad, uint32_t& err) {
  const bool inside = (val(x) >= q.left) && (val(x) <= q.right);
  if (!inside) {
    y = x;
    lad = T(0.f);
    if (!q.tails) err |= kErrOutsideDomain;
    return false;
  }
  xn = q.inverse ? (x - q.bottom) / (q.top - q.bottom) : (x - q.left) / (q.right - q.left);
  return true;
}

template <class T>
__device__ __forceinline__ T spline_out(const SplineParams& q, T v) {
  return q.inverse ? v * (q.right - q.left) + q.left : v * (q.top - q.bottom) + q.bottom;
}

// softmax of K values in place: p[i] = floor + c1 * softmax_i   (floor = 0, c1 = 1: plain softmax)
template <class T>
__device__ __forceinline__ void softmax_inplace(T* __restrict__ p, int K, float div, float floor_v, float c1) {
  float m = -INFINITY;
  for (int i = 0; i < K; ++i) {
    const T t = p[i] / div;
    p[i] = t;
    m = fmaxf(m, val(t));
  }
  T sum = T(0.f);
  for (int i = 0; i < K; ++i) {
    const T e = exp_of(p[i] - m);
    p[i] = e;
    sum = sum + e;
  }
  const T rs = 1.f / sum;
  for (int i = 0; i < K; ++i) p[i] = floor_v + c1 * (p[i] * rs);
}

// ---- linear -----------------------------------------------------------------------------------------

// torch.linspace(0, 1, K + 1)[i] in float32 (symmetric evaluation used by ATen)
__device__ __forceinline__ float linspace01(int i, int K) {
  const float step = 1.f / (float)K;
  const int steps = K + 1;
  return i < steps / 2 ? step * (float)i : 1.f - step * (float)(steps - 1 - i);
}

template <class T>
__device__ __forceinline__ void linear_prepare(const SplineParams& q, T* __restrict__ p) {
  softmax_inplace(p, q.K, 1.f, 0.f, 1.f);  // pdf
}

// linear.py:38-75 (forward): out = cdf[idx] + alpha pdf[idx], lad = log pdf[idx] + log K
template <class T>
__device__ __forceinline__ void linear_spline_forward(const SplineParams& q, const T* __restrict__ pdf, T xn, T& out, T& lad) {
  const int K = q.K;
  const T bin_pos = xn * (float)K;
  int idx = (int)floorf(val(bin_pos));
  if (idx >= K) idx = K - 1;
  if (idx < 0) idx = 0;
  const T alpha = bin_pos - (float)idx;
  RunningSum<T> cum;
  for (int i = 0; i < idx; ++i) cum.add(pdf[i]);
  const T p = pdf[idx];
  out = clamp01(cum.get() + alpha * p);
  lad = log_of(p) - logf(1.f / (float)K);
}

struct LinearSplineOp {
  static constexpr bool kHasPrepare = true;
  SplineParams q;

  __device__ __forceinline__ void prepare(float* __restrict__ prow, int j, int d_t) const {
    linear_prepare(q, prow + j * q.K);
  }

  __device__ __forceinline__ void eval(const float* __restrict__ prow, int j, int d_t, float x, float& y,
                                       float& lad, uint32_t& err) const {
    const int K = q.K;
    const float* pdf = prow + j * K;
    float xn;
    if (!spline_gate(q, x, xn, y, lad, err)) return;
    if (!q.inverse) {
      float out;
      linear_spline_forward(q, pdf, xn, out, lad);
      y = spline_out(q, out);
    } else {
      // cdf knots: 0, c_0, ..., c_{K-2}, 1 (+1e-6 after the reference's in-place searchsorted nudge)
      // (declared in this order on purpose: with the forward branch behind a call, the other order costs the
      //  <8, 2> prefetch kernel a 97th VGPR and with it a wave of occupancy; tools/kernel_stats.py shows it)
      int idx = 0;
      float knot_hi = 0.f, knot_lo = 0.f, lo = 0.f;
      double cum = 0.0;
      for (int i = 0; i < K; ++i) {
        cum += (double)pdf[i];
        const float hi = (i == K - 1) ? (1.0f + 1e-6f) : (float)cum;
        if (xn >= lo) {
          idx = i;
          knot_lo = lo;
          knot_hi = hi;
        }
        lo = hi;
      }
      const float b0 = linspace01(idx, K), b1 = linspace01(idx + 1, K);
      const float slope = (knot_hi - knot_lo) / (b1 - b0);
      const float offset = knot_hi - slope * b1;
      float out = (xn - offset) / slope;
      out = clamp01(out);
      lad = -logf(slope);
      y = spline_out(q, out);
    }
  }
};

// ---- quadratic --------------------------------------------------------------------------------------

__host__ __device__ __forceinline__ int quadratic_heights(const SplineParams& q) { return q.tails ? q.K - 1 : q.K + 1; }

template <class T>
__device__ __forceinline__ void quadratic_prepare(const SplineParams& q, T* __restrict__ p) {
  softmax_inplace(p, q.K, q.w_div, q.min_w, q.cw);  // widths
  T* h = p + q.K;
  for (int i = 0; i < quadratic_heights(q); ++i) h[i] = softplus1(h[i] / q.h_div) + 1e-3f;  // quadratic.py:85
}

// un-normalised height at knot i (0..K): boundary knots get `edge` when only K-1 were given
template <class T>
__device__ __forceinline__ T quadratic_knot_h(const SplineParams& q, const T* __restrict__ h, int i, T edge) {
  if (!q.tails) return h[i];
  return (i == 0 || i == q.K) ? edge : h[i - 1];
}

// One element of the quadratic spline on its prepared row (w, h), gate and output scaling included (quadratic.py:55-159).
// Forward and inverse share the knot walk; the inverse's root is float only.  (The whole element is one function on
// purpose: with the gate, the walk or the output scaling split off, the device-loop kernels of
// fc_made_inverse_spline_quadratic.hip take up to 17 more VGPRs and one of them spills; tools/kernel_stats.py shows it.)
template <class T>
__device__ __forceinline__ void quadratic_spline_eval(const SplineParams& q, const T* __restrict__ w, const T* __restrict__ h,
                                                      T x, T& y, T& lad, uint32_t& err) {
  const int K = q.K;
  T xn;
  if (!spline_gate(q, x, xn, y, lad, err)) return;

  T edge = T(0.f);
  if (q.tails) {
    // boundary heights such that the normalised boundary density is 1 (quadratic.py:87-102)
    const T first_w = 0.5f * w[0], last_w = 0.5f * w[K - 1];
    T mid = T(0.f);
    for (int i = 0; i + 1 < K - 1; ++i) mid = mid + ((h[i] + h[i + 1]) / 2.f) * w[i + 1];
    const T numer = 0.5f * first_w * h[0] + 0.5f * last_w * h[K - 2] + mid;
    edge = numer / (1.f - 0.5f * first_w - 0.5f * last_w);
  }
  T area = T(0.f);
  for (int i = 0; i < K; ++i) area = area + ((quadratic_knot_h(q, h, i, edge) + quadratic_knot_h(q, h, i + 1, edge)) / 2.f) * w[i];
  const float oh = 1.f - q.min_h;

  // walk: cumulative cdf / locations, last entries pinned to 1 (+1e-6 nudge on the searched axis)
  RunningSum<T> cum_cdf, cum_loc;
  T lo_cdf = T(0.f), lo_loc = T(0.f);
  T hl_prev = q.min_h + oh * (quadratic_knot_h(q, h, 0, edge) / area);
  T loc = T(0.f), wk = w[0], lc = T(0.f), hl = hl_prev, hr = hl_prev;
  for (int i = 0; i < K; ++i) {
    const T hr_i = q.min_h + oh * (quadratic_knot_h(q, h, i + 1, edge) / area);
    cum_cdf.add(((hl_prev + hr_i) / 2.f) * w[i]);
    cum_loc.add(w[i]);
    const T hi_cdf = (i == K - 1) ? T(1.f) : cum_cdf.get();
    const T hi_loc = (i == K - 1) ? T(1.f) : cum_loc.get();
    const bool take = q.inverse ? (val(xn) >= val(lo_cdf)) : (val(xn) >= val(lo_loc));
    if (take) {
      loc = lo_loc;
      wk = w[i];
      lc = lo_cdf;
      hl = hl_prev;
      hr = hr_i;
    }
    lo_cdf = hi_cdf;
    lo_loc = hi_loc;
    hl_prev = hr_i;
  }
  const T a = 0.5f * (hr - hl) * wk;
  const T b = hl * wk;
  T out;
  if (q.inverse) {
    if constexpr (std::is_same<T, float>::value) {
      const float c_ = lc - xn;
      // The reference's (-b + sqrt(b^2 - 4 a c)) / (2 a) (quadratic.py:139) cancels where the two knot heights of the bin
      // are close (a -> 0; 0 / 0 at a = 0): its float32 result is then off by up to 6e-4 against its own float64
      // evaluation on random parameters.  2 c / (-b - sqrt(..)) is the same root without the cancellation (b = left
      // height x width > 0, c <= 0 inside the bin), as in the cubic's a -> 0 fallback below.
      const float alpha = (2.f * c_) / (-b - sqrtf(b * b - 4.f * a * c_));
      out = alpha * wk + loc;
      out = clamp01(out);
      lad = -logf(alpha * (hr - hl) + hl);
    }
  } else {
    const T alpha = (xn - loc) / wk;
    out = a * (alpha * alpha) + b * alpha + lc;
    out = clamp01(out);
    lad = log_of(alpha * (hr - hl) + hl);
  }
  y = spline_out(q, out);
}

struct QuadraticSplineOp {
  static constexpr bool kHasPrepare = true;
  SplineParams q;

  __device__ __forceinline__ int nh() const { return quadratic_heights(q); }

  __device__ __forceinline__ void prepare(float* __restrict__ prow, int j, int d_t) const {
    quadratic_prepare(q, prow + j * (q.K + nh()));
  }

  __device__ __forceinline__ void eval(const float* __restrict__ prow, int j, int d_t, float x, float& y,
                                       float& lad, uint32_t& err) const {
    const float* w = prow + j * (q.K + nh());
    quadratic_spline_eval(q, w, w + q.K, x, y, lad, err);
  }
};

// ---- cubic --------------------------------------------------------------------------------------------

__device__ __forceinline__ float cbrt_ref(float v) {  // torchutils.cbrt: sign * exp(log|v| / 3)
  return sgn(v) * expf(logf(fabsf(v)) / 3.f);
}

template <class T>
__device__ __forceinline__ void cubic_prepare(const SplineParams& q, T* __restrict__ p) {
  softmax_inplace(p, q.K, q.w_div, q.min_w, q.cw);
  softmax_inplace(p + q.K, q.K, q.h_div, q.min_h, q.ch);
}

// interior knot derivative between bins i and i+1 (cubic.py:113-131)
template <class T>
__device__ __forceinline__ T cubic_interior(const T* __restrict__ w, const T* __restrict__ h, int i) {
  const T s0 = h[i] / w[i], s1 = h[i + 1] / w[i + 1];
  const T m1 = min_of(abs_of(s0), abs_of(s1));
  const T m2 = 0.5f * (w[i + 1] * s0 + w[i] * s1) / (w[i] + w[i + 1]);
  return min_of(m1, m2) * (sgn(s0) + sgn(s1));
}

// the bin an element falls into: y = ca t^3 + cb t^2 + cc t + dco on t = x - left_w
template <class T>
struct CubicBin {
  T left_w, right_w, ca, cb, cc, dco;
};

// Walks the knots of prepared (w, h, the two boundary-derivative logits behind them) (cubic.py:84-151).  `xn` is compared
// with the cumulative heights for the inverse and with the cumulative widths otherwise.
template <class T>
__device__ __forceinline__ CubicBin<T> cubic_bin(const SplineParams& q, const T* __restrict__ w, const T* __restrict__ h,
                                                 float xn, bool inverse) {
  const int K = q.K;
  RunningSum<T> cw, chh;
  T lo_w = T(0.f), lo_h = T(0.f);
  int idx = 0;
  CubicBin<T> bin;
  bin.left_w = T(0.f), bin.right_w = T(1.f), bin.dco = T(0.f);
  for (int i = 0; i < K; ++i) {
    cw.add(w[i]);
    chh.add(h[i]);
    const T hi_w = (i == K - 1) ? T(1.f) : cw.get();
    const T hi_h = (i == K - 1) ? T(1.f) : chh.get();
    const bool take = inverse ? (xn >= val(lo_h)) : (xn >= val(lo_w));
    if (take) {
      idx = i;
      bin.left_w = lo_w;
      bin.right_w = hi_w;
      bin.dco = lo_h;
    }
    lo_w = hi_w;
    lo_h = hi_h;
  }
  // (right_w is only read by the inverse, where the searched -- and nudged -- axis is cumheights,
  //  so cumwidths[idx + 1] is the un-nudged knot, cubic.py:139-151)

  const T wk = w[idx];
  const T s = h[idx] / wk;
  const T dl = idx == 0 ? sigmoidf(w[2 * K]) * 3.f * (h[0] / w[0]) : cubic_interior(w, h, idx - 1);
  const T dr = idx == K - 1 ? sigmoidf(w[2 * K + 1]) * 3.f * (h[K - 1] / w[K - 1]) : cubic_interior(w, h, idx);
  bin.ca = (dl + dr - 2.f * s) / (wk * wk);
  bin.cb = (3.f * s - 2.f * dl - dr) / wk;
  bin.cc = dl;
  return bin;
}

// cubic.py:246-267 (forward)
template <class T>
__device__ __forceinline__ void cubic_spline_forward(const CubicBin<T>& s, T xn, T& out, T& lad) {
  const T t = xn - s.left_w;
  out = s.ca * (t * t * t) + s.cb * (t * t) + s.cc * t + s.dco;
  lad = log_of(3.f * s.ca * (t * t) + 2.f * s.cb * t + s.cc);
}

struct CubicSplineOp {
  static constexpr bool kHasPrepare = true;
  SplineParams q;

  __device__ __forceinline__ void prepare(float* __restrict__ prow, int j, int d_t) const {
    cubic_prepare(q, prow + j * (2 * q.K + 2));
  }

  __device__ __forceinline__ void eval(const float* __restrict__ prow, int j, int d_t, float x, float& y,
                                       float& lad, uint32_t& err) const {
    const int K = q.K;
    const float* w = prow + j * (2 * K + 2);
    const float* h = w + K;
    float xn;
    if (!spline_gate(q, x, xn, y, lad, err)) return;
    const CubicBin<float> s = cubic_bin(q, w, h, xn, q.inverse != 0);

    float out;
    if (!q.inverse) {
      cubic_spline_forward(s, xn, out, lad);
    } else {
      // Blinn's closed form (cubic.py:152-244), evaluated without its two cancellations.  The reference's float32
      // sequence is correct in exact arithmetic but loses the answer in two places (measured against its own float64
      // evaluation: max error 1e-3 .. 8e-3 on random parameters, tools/probe/cubic_inverse_accuracy.py):
      //  * one real root: q^3 = (-dep1 - sqrt(-disc)) / 2 cancels to a few ulps when |delta_1|^3 << dep1^2 (an almost
      //    quadratic bin just above the |a| < 1e-3 fallback) and the cube root amplifies what is left by ~1e3.  Here the
      //    cube of larger magnitude is taken by the sum that does not cancel and the other from p q = -delta_1.
      //  * a -> 0 fallback: (-b + sqrt(b^2 - 4 a c)) / (2 a) cancels (and is 0 / 0 at a = 0); 2 c / (-b - sqrt(..)) is
      //    the same root (b = left knot derivative > 0, c <= 0 inside the bin).
      // Two Newton steps on the bin's cubic then remove the rounding of the closed form itself; a step is taken only
      // if it stays inside the bin (+- eps) with a positive slope.  The a -> 0 fallback is NOT polished: there the
      // reference DEFINES the inverse through the quadratic part alone, and that definition is kept.
      // Against float64 the result is never further off than the reference's float32 result (same probe).
      const float b_ = (s.cb / s.ca) / 3.f;
      const float c_ = (s.cc / s.ca) / 3.f;
      const float d_ = (s.dco - xn) / s.ca;
      const float delta_1 = -(b_ * b_) + c_;
      const float delta_2 = -c_ * b_ + d_;
      const float delta_3 = b_ * d_ - c_ * c_;
      const float disc = 4.f * delta_1 * delta_3 - delta_2 * delta_2;
      const float dep1 = -2.f * b_ * delta_1 + delta_2;
      const float dep2 = delta_1;
      if (disc >= 0.f) {
        float theta = atan2f(sqrtf(disc), -dep1);
        theta /= 3.f;
        const float c1 = cosf(theta), s1 = sinf(theta);
        const float k3 = 0.5f * 1.7320508075688772f;  // 0.5 * math.sqrt(3)
        float r1 = c1, r2 = -0.5f * c1 - k3 * s1, r3 = -0.5f * c1 + k3 * s1;
        const float scale = 2.f * sqrtf(-dep2);
        const float shift = -b_ + s.left_w;
        r1 = r1 * scale + shift;
        r2 = r2 * scale + shift;
        r3 = r3 * scale + shift;
        const bool m1 = ((s.left_w - q.eps) < r1) && (r1 < (s.right_w + q.eps));
        const bool m2 = ((s.left_w - q.eps) < r2) && (r2 < (s.right_w + q.eps));
        const bool m3 = ((s.left_w - q.eps) < r3) && (r3 < (s.right_w + q.eps));
        // argsort(masks, descending)[0]: first root whose mask is set (stable), else the first
        out = m1 ? r1 : (m2 ? r2 : (m3 ? r3 : r1));
      } else {
        const float sq = sqrtf(-disc);
        const float big = (-dep1 + (dep1 <= 0.f ? sq : -sq)) / 2.f;
        const float p = cbrt_ref(big);
        const float qq = p != 0.f ? -dep2 / p : 0.f;
        out = (p + qq) - b_ + s.left_w;
      }
      if (fabsf(s.ca) < q.quad_thresh) {
        const float a2 = s.cb, b2 = s.cc, c2 = s.dco - xn;
        const float alpha = (2.f * c2) / (-b2 - sqrtf(b2 * b2 - 4.f * a2 * c2));
        out = alpha + s.left_w;
      } else {
#pragma unroll
        for (int it = 0; it < 2; ++it) {
          const float t = out - s.left_w;
          const float fv = ((s.ca * t + s.cb) * t + s.cc) * t + (s.dco - xn);
          const float fp = (3.f * s.ca * t + 2.f * s.cb) * t + s.cc;
          const float nxt = out - fv / fp;
          // (comparisons are false for NaN: a failed step keeps the closed-form root)
          if (fp > 0.f && nxt > s.left_w - q.eps && nxt < s.right_w + q.eps) out = nxt;
        }
      }
      const float t = out - s.left_w;
      lad = -logf(3.f * s.ca * (t * t) + 2.f * s.cb * t + s.cc);
    }
    y = spline_out(q, out);
  }
};

}  // namespace fc
