// Discrete and uniform base densities, gfx950: four streaming kernels in the layout of fc_reduce.hip.
//
// Restates (not copies):
//   flowcon/distributions/discrete.py:41-68   ConditionalIndependentBernoulli._log_prob / ._sample
//   flowcon/distributions/uniform.py:7-29     BoxUniform.log_prob = Independent(Uniform).log_prob
//
// Layout: T lanes (a power of two <= 64) cooperate on one row, a 256-thread block covers 256 / T rows per pass and strides
// over the batch -- one wave per row once a row has 64 loads or more, sub-wave groups below that (D = 1 runs 256 rows per
// block).  kVec: D % 4 == 0 and every base pointer 16-byte aligned, rows move as float4; otherwise as scalars.  The lanes
// loop over their row, so D has no upper limit.  No atomics, no data-dependent loops: every bound is N, D or S.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "fc_device.h"
#include "fc_math.h"
#include "../../include/flowcon_hip.h"

namespace fc {

// x l - softplus(l), softplus(l) = max(l, 0) + log1p(exp(-|l|)), grouped as (x - [l > 0]) l - log1p(exp(-|l|)): the same
// real number, but x = 1 at l = +40 gives the tail -exp(-40) instead of 40 - 40 (x - [l > 0] is exact for x in {0, 1}).
// It equals the reference's -x softplus(-l) - (1 - x) softplus(l) for every real x, since softplus(-l) = softplus(l) - l.
__device__ __forceinline__ float bernoulli_term(float x, float l) {
  const float step = l > 0.f ? 1.f : 0.f;
  return (x - step) * l - log1p_lean_pos(exp_lean(-fabsf(l)));
}

template <int T>
__device__ __forceinline__ float lanes_sum(float v) {
#pragma unroll
  for (int o = T >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o, T);
  return v;
}

template <int T, bool kVec>
__global__ __launch_bounds__(256) void bernoulli_log_prob_kernel(const float* __restrict__ x, const float* __restrict__ l,
                                                                 const float* __restrict__ add, float* __restrict__ out,
                                                                 int64_t n, int d) {
  constexpr int kRows = 256 / T;
  const int lane = threadIdx.x % T;
  const int64_t stride = (int64_t)gridDim.x * kRows;
  for (int64_t row0 = (int64_t)blockIdx.x * kRows; row0 < n; row0 += stride) {
    const int64_t row = row0 + threadIdx.x / T;
    float acc = 0.f;
    if (row < n) {
      if constexpr (kVec) {
        const float4* xr = reinterpret_cast<const float4*>(x + row * d);
        const float4* lr = reinterpret_cast<const float4*>(l + row * d);
        for (int j = lane; j < (d >> 2); j += T) {
          const float4 xv = xr[j], lv = lr[j];
          acc += (bernoulli_term(xv.x, lv.x) + bernoulli_term(xv.y, lv.y)) +
                 (bernoulli_term(xv.z, lv.z) + bernoulli_term(xv.w, lv.w));
        }
      } else {
        const float* xr = x + row * d;
        const float* lr = l + row * d;
        for (int j = lane; j < d; j += T) acc += bernoulli_term(xr[j], lr[j]);
      }
    }
    acc = lanes_sum<T>(acc);
    if (row < n && lane == 0) out[row] = add ? acc + add[row] : acc;
  }
}

// grad_logits = g (x - sigmoid(l)), grad_inputs = g l; either output may be null (x is not read without grad_logits)
template <int T, bool kVec>
__global__ __launch_bounds__(256) void bernoulli_log_prob_backward_kernel(const float* __restrict__ x,
                                                                          const float* __restrict__ l,
                                                                          const float* __restrict__ g,
                                                                          float* __restrict__ gl, float* __restrict__ gx,
                                                                          int64_t n, int d) {
  constexpr int kRows = 256 / T;
  const int lane = threadIdx.x % T;
  const int64_t stride = (int64_t)gridDim.x * kRows;
  for (int64_t row0 = (int64_t)blockIdx.x * kRows; row0 < n; row0 += stride) {
    const int64_t row = row0 + threadIdx.x / T;
    if (row >= n) continue;
    const float gr = g[row];
    const int64_t base = row * d;
    if constexpr (kVec) {
      const float4* lr = reinterpret_cast<const float4*>(l + base);
      for (int j = lane; j < (d >> 2); j += T) {
        const float4 lv = lr[j];
        if (gl) {
          const float4 xv = reinterpret_cast<const float4*>(x + base)[j];
          reinterpret_cast<float4*>(gl + base)[j] =
              float4{gr * (xv.x - sigmoid_lean(lv.x)), gr * (xv.y - sigmoid_lean(lv.y)), gr * (xv.z - sigmoid_lean(lv.z)),
                     gr * (xv.w - sigmoid_lean(lv.w))};
        }
        if (gx) reinterpret_cast<float4*>(gx + base)[j] = float4{gr * lv.x, gr * lv.y, gr * lv.z, gr * lv.w};
      }
    } else {
      for (int j = lane; j < d; j += T) {
        const float lv = l[base + j];
        if (gl) gl[base + j] = gr * (x[base + j] - sigmoid_lean(lv));
        if (gx) gx[base + j] = gr * lv;
      }
    }
  }
}

// out[r, :] = noise[r, :] < sigmoid(logits[r / S, :]): the S draws of a context row read that row's logits in place
template <int T, bool kVec>
__global__ __launch_bounds__(256) void bernoulli_sample_kernel(const float* __restrict__ logits,
                                                               const float* __restrict__ noise, float* __restrict__ out,
                                                               int64_t n, int s, int d) {
  constexpr int kRows = 256 / T;
  const int lane = threadIdx.x % T;
  const bool narrow = n <= (int64_t)INT32_MAX;      // kernel-uniform: a 32-bit quotient where the row index fits
  const int64_t stride = (int64_t)gridDim.x * kRows;
  for (int64_t row0 = (int64_t)blockIdx.x * kRows; row0 < n; row0 += stride) {
    const int64_t row = row0 + threadIdx.x / T;
    if (row >= n) continue;
    const int64_t ctx = narrow ? (int64_t)((uint32_t)row / (uint32_t)s) : row / s;
    const int64_t base = row * d, lbase = ctx * d;
    if constexpr (kVec) {
      for (int j = lane; j < (d >> 2); j += T) {
        const float4 lv = reinterpret_cast<const float4*>(logits + lbase)[j];
        const float4 u = reinterpret_cast<const float4*>(noise + base)[j];
        reinterpret_cast<float4*>(out + base)[j] =
            float4{u.x < sigmoid_lean(lv.x) ? 1.f : 0.f, u.y < sigmoid_lean(lv.y) ? 1.f : 0.f,
                   u.z < sigmoid_lean(lv.z) ? 1.f : 0.f, u.w < sigmoid_lean(lv.w) ? 1.f : 0.f};
      }
    } else {
      for (int j = lane; j < d; j += T) out[base + j] = noise[base + j] < sigmoid_lean(logits[lbase + j]) ? 1.f : 0.f;
    }
  }
}

// -sum_d log(high_d - low_d) where low_d <= x_d < high_d for every d, -inf otherwise (NaN fails both comparisons).  Each
// lane group sums the logarithms once, before its rows: every finite row carries the same value.
template <int T, bool kVec>
__global__ __launch_bounds__(256) void box_log_prob_kernel(const float* __restrict__ x, const float* __restrict__ low,
                                                           const float* __restrict__ high, float* __restrict__ out,
                                                           int64_t n, int d) {
  constexpr int kRows = 256 / T;
  const int lane = threadIdx.x % T;
  float volume = 0.f;
  for (int j = lane; j < d; j += T) volume += logf(high[j] - low[j]);
  volume = lanes_sum<T>(volume);
  const int64_t stride = (int64_t)gridDim.x * kRows;
  for (int64_t row0 = (int64_t)blockIdx.x * kRows; row0 < n; row0 += stride) {
    const int64_t row = row0 + threadIdx.x / T;
    int inside = 1;
    if (row < n) {
      if constexpr (kVec) {
        const float4* xr = reinterpret_cast<const float4*>(x + row * d);
        for (int j = lane; j < (d >> 2); j += T) {
          const float4 v = xr[j];
          const float4 lo = reinterpret_cast<const float4*>(low)[j], hi = reinterpret_cast<const float4*>(high)[j];
          inside &= (lo.x <= v.x && v.x < hi.x) && (lo.y <= v.y && v.y < hi.y) && (lo.z <= v.z && v.z < hi.z) &&
                    (lo.w <= v.w && v.w < hi.w);
        }
      } else {
        const float* xr = x + row * d;
        for (int j = lane; j < d; j += T) {
          const float v = xr[j];
          inside &= low[j] <= v && v < high[j];
        }
      }
    }
#pragma unroll
    for (int o = T >> 1; o > 0; o >>= 1) inside &= __shfl_xor(inside, o, T);
    if (row < n && lane == 0) out[row] = inside ? -volume : -INFINITY;
  }
}

struct RowLaunch {
  bool vec;
  int lanes;
  dim3 grid;
};

// `aligned`: every [rows, d] / [d] base pointer of the call is on a 16-byte boundary
inline RowLaunch row_launch(int64_t n, int d, bool aligned) {
  RowLaunch r;
  r.vec = d % 4 == 0 && aligned;
  const int items = r.vec ? d / 4 : d;      // loads per row
  r.lanes = 1;
  while (r.lanes < items && r.lanes < 64) r.lanes <<= 1;
  const int rows_per_block = 256 / r.lanes;
  int64_t grid = (n + rows_per_block - 1) / rows_per_block;
  const int64_t cap = (int64_t)device_cu_count() * 16;      // grid-stride: 16 blocks of 256 threads per CU
  r.grid = dim3((unsigned)(grid > cap ? cap : grid));
  return r;
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

}  // namespace fc

#define FC_ROW_LANES(LANES, CALL)                   \
  switch (LANES) {                                  \
    case 1: { constexpr int T = 1; CALL; break; }   \
    case 2: { constexpr int T = 2; CALL; break; }   \
    case 4: { constexpr int T = 4; CALL; break; }   \
    case 8: { constexpr int T = 8; CALL; break; }   \
    case 16: { constexpr int T = 16; CALL; break; } \
    case 32: { constexpr int T = 32; CALL; break; } \
    default: { constexpr int T = 64; CALL; break; } \
  }

#define FC_ROW_LAUNCH(R, KERNEL, STREAM, ...)                                                                          \
  if ((R).vec) {                                                                                                       \
    FC_ROW_LANES((R).lanes, hipLaunchKernelGGL((fc::KERNEL<T, true>), (R).grid, dim3(256), 0, STREAM, __VA_ARGS__));  \
  } else {                                                                                                             \
    FC_ROW_LANES((R).lanes, hipLaunchKernelGGL((fc::KERNEL<T, false>), (R).grid, dim3(256), 0, STREAM, __VA_ARGS__)); \
  }

extern "C" int fc_bernoulli_log_prob(const float* inputs, const float* logits, const float* add, float* out, int64_t n,
                                     int32_t d, void* stream) {
  if (n < 0 || d <= 0) return hipErrorInvalidValue;
  if (n == 0) return hipSuccess;
  if (!inputs || !logits || !out) return hipErrorInvalidValue;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const fc::RowLaunch r = fc::row_launch(n, d, fc::aligned16(inputs) && fc::aligned16(logits));
  FC_ROW_LAUNCH(r, bernoulli_log_prob_kernel, s, inputs, logits, add, out, n, d);
  return hipGetLastError();
}

extern "C" int fc_bernoulli_log_prob_backward(const float* inputs, const float* logits, const float* grad_out,
                                              float* grad_logits, float* grad_inputs, int64_t n, int32_t d,
                                              void* stream) {
  if (n < 0 || d <= 0) return hipErrorInvalidValue;
  if (n == 0 || (!grad_logits && !grad_inputs)) return hipSuccess;
  if (!logits || !grad_out || (grad_logits && !inputs)) return hipErrorInvalidValue;
  hipStream_t s = static_cast<hipStream_t>(stream);
  // (a null pointer counts as aligned: it is never dereferenced)
  const fc::RowLaunch r = fc::row_launch(n, d, fc::aligned16(inputs) && fc::aligned16(logits) &&
                                                   fc::aligned16(grad_logits) && fc::aligned16(grad_inputs));
  FC_ROW_LAUNCH(r, bernoulli_log_prob_backward_kernel, s, inputs, logits, grad_out, grad_logits, grad_inputs, n, d);
  return hipGetLastError();
}

extern "C" int fc_bernoulli_sample(const float* logits, const float* noise, float* out, int64_t contexts,
                                   int32_t num_samples, int32_t d, void* stream) {
  if (contexts < 0 || num_samples <= 0 || d <= 0) return hipErrorInvalidValue;
  if (contexts > INT64_MAX / num_samples) return hipErrorInvalidValue;
  if (contexts == 0) return hipSuccess;
  if (!logits || !noise || !out) return hipErrorInvalidValue;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int64_t n = contexts * num_samples;
  const fc::RowLaunch r = fc::row_launch(n, d, fc::aligned16(logits) && fc::aligned16(noise) && fc::aligned16(out));
  FC_ROW_LAUNCH(r, bernoulli_sample_kernel, s, logits, noise, out, n, num_samples, d);
  return hipGetLastError();
}

extern "C" int fc_box_log_prob(const float* inputs, const float* low, const float* high, float* out, int64_t n, int32_t d,
                               void* stream) {
  if (n < 0 || d <= 0) return hipErrorInvalidValue;
  if (n == 0) return hipSuccess;
  if (!inputs || !low || !high || !out) return hipErrorInvalidValue;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const fc::RowLaunch r = fc::row_launch(n, d, fc::aligned16(inputs) && fc::aligned16(low) && fc::aligned16(high));
  FC_ROW_LAUNCH(r, box_log_prob_kernel, s, inputs, low, high, out, n, d);
  return hipGetLastError();
}
