// Dual numbers (value, tangent) for forward-mode differentiation of float32 device code, and the handful of overloads
// that let ONE source text be instantiated with float and with Dual (fc_spline_ops.h).  The value part of every
// operation here is bit for bit what the float operation computes, so that a Dual evaluation takes every branch and
// picks every bin exactly as the float one does; the tangent is float arithmetic on the side.
#pragma once
#include <hip/hip_runtime.h>
#include "fc_math.h"

namespace fc {

struct Dual {
  float v, d;
  Dual() = default;
  __device__ __forceinline__ explicit Dual(float v_) : v(v_), d(0.f) {}
  __device__ __forceinline__ Dual(float v_, float d_) : v(v_), d(d_) {}
};

__device__ __forceinline__ Dual operator+(Dual a, Dual b) { return Dual{a.v + b.v, a.d + b.d}; }
__device__ __forceinline__ Dual operator-(Dual a, Dual b) { return Dual{a.v - b.v, a.d - b.d}; }
__device__ __forceinline__ Dual operator*(Dual a, Dual b) { return Dual{a.v * b.v, a.d * b.v + a.v * b.d}; }
__device__ __forceinline__ Dual operator/(Dual a, Dual b) {
  const float q = a.v / b.v;
  return Dual{q, (a.d - q * b.d) / b.v};
}
__device__ __forceinline__ Dual operator+(Dual a, float b) { return Dual{a.v + b, a.d}; }
__device__ __forceinline__ Dual operator+(float a, Dual b) { return Dual{a + b.v, b.d}; }
__device__ __forceinline__ Dual operator-(Dual a, float b) { return Dual{a.v - b, a.d}; }
__device__ __forceinline__ Dual operator-(float a, Dual b) { return Dual{a - b.v, -b.d}; }
__device__ __forceinline__ Dual operator*(Dual a, float b) { return Dual{a.v * b, a.d * b}; }
__device__ __forceinline__ Dual operator*(float a, Dual b) { return Dual{a * b.v, a * b.d}; }
__device__ __forceinline__ Dual operator/(Dual a, float b) { return Dual{a.v / b, a.d / b}; }
__device__ __forceinline__ Dual operator/(float a, Dual b) {
  const float q = a / b.v;
  return Dual{q, -(q * b.d) / b.v};
}

// the value of a number of either type (comparisons, bin search and floorf look at values only)
__device__ __forceinline__ float val(float a) { return a; }
__device__ __forceinline__ float val(Dual a) { return a.v; }

// libm functions under names of their own (an overload called expf inside fc:: would hide ::expf)
__device__ __forceinline__ float exp_of(float a) { return expf(a); }
__device__ __forceinline__ Dual exp_of(Dual a) {
  const float e = expf(a.v);
  return Dual{e, e * a.d};
}
__device__ __forceinline__ float log_of(float a) { return logf(a); }
__device__ __forceinline__ Dual log_of(Dual a) { return Dual{logf(a.v), a.d / a.v}; }
__device__ __forceinline__ float abs_of(float a) { return fabsf(a); }
__device__ __forceinline__ Dual abs_of(Dual a) { return Dual{fabsf(a.v), a.v < 0.f ? -a.d : a.d}; }
__device__ __forceinline__ float min_of(float a, float b) { return fminf(a, b); }
__device__ __forceinline__ Dual min_of(Dual a, Dual b) { return Dual{fminf(a.v, b.v), b.v < a.v ? b.d : a.d}; }

// the project's own float helpers, overloaded
__device__ __forceinline__ float sgn(float v) { return (float)((v > 0.f) - (v < 0.f)); }
__device__ __forceinline__ float sgn(Dual a) { return sgn(a.v); }

// torch.clamp(x, 0, 1) as ATen computes it: a NaN (e.g. the square root of a discriminant that rounding pushed
// below zero, splines/quadratic.py:139) stays a NaN instead of turning into 0 the way fminf / fmaxf would make it
__device__ __forceinline__ float clamp01(float x) { return x < 0.f ? 0.f : (x > 1.f ? 1.f : x); }
__device__ __forceinline__ Dual clamp01(Dual a) { return Dual{clamp01(a.v), (a.v < 0.f || a.v > 1.f) ? 0.f : a.d}; }

// F.softplus (threshold 20) and torch.sigmoid
__device__ __forceinline__ Dual softplus1(Dual a) {
  if (a.v > 20.f) return a;
  const float e = expf(a.v);
  return Dual{log1pf(e), a.d * (e / (1.f + e))};
}
__device__ __forceinline__ Dual sigmoidf(Dual a) {
  const float s = 1.f / (1.f + expf(-a.v));
  return Dual{s, a.d * s * (1.f - s)};
}

// A knot sum as the forward kernels run it: the value accumulates in double and is rounded to float where it is read;
// the tangent accumulates in float.
template <class T> struct RunningSum;
template <> struct RunningSum<float> {
  double s = 0.0;
  __device__ __forceinline__ void add(float x) { s += (double)x; }
  __device__ __forceinline__ float get() const { return (float)s; }
};
template <> struct RunningSum<Dual> {
  double s = 0.0;
  float d = 0.f;
  __device__ __forceinline__ void add(Dual x) { s += (double)x.v; d += x.d; }
  __device__ __forceinline__ Dual get() const { return Dual{(float)s, d}; }
};

}  // namespace fc
