// Backward of the row-norm bijectors (forward kernels in fc_rownorm.hip), gfx950.  One wave owns one sample row (fc_row.h);
// input gradients leave per row, the radial flow's parameter gradients are sums over the batch: every wave accumulates its
// rows' contributions in registers and adds them to the global result once, at the end, with one atomic per element and wave
// (as fc_planar_backward does).
//
// Radial (forward direction; what torch.autograd yields for no_analytic_inv/planar.py:199-211 from a = |alpha|,
// b = softplus(beta) - |alpha| on):  dz = x - z0, r = |dz|, A = a + r, h = b / A, k = -b r / A^2, y = x + h dz,
// lad = (d - 1) log(1 + h) + log(1 + h + k).  With c = gy.dz and gl the gradient of lad:
//   g_h = c + gl ((d - 1) / (1 + h) + 1 / (1 + h + k));   g_k = gl / (1 + h + k)
//   g_A = -g_h b / A^2 + 2 g_k b r / A^3;   g_r = g_A - g_k b / A^2
//   ga += g_A;   gb += g_h / A - g_k r / A^2;   g_dz = h gy + g_r dz / r;   gx = gy + g_dz;   gz0 -= g_dz
// A row exactly on z0 (r = 0): the reference's autograd yields NaN there through the norm's gradient; here the norm's
// subgradient is taken as 0 (g_r dz / r := 0), which keeps every gradient finite.
//
// Unit vector, no parameters.  Forward (s = |x|^2, y[:d] = 2 x / (s + 1), y[d] = 1 - 2 / (s + 1), lad = d (log 2 - log1p s)):
//   gx = 2 gy[:d] / (s + 1) + 2 x G,   G = 2 (gy[d] - gy[:d].x) / (s + 1)^2 - gl d / (s + 1)
// Inverse (t = 1 - y[d], x = y[:d] / t, lad = -d (log 2 - log1p |x|^2)):
//   g = gx + gl 2 d x / (1 + |x|^2);   gy[:d] = g / t;   gy[d] = (g.x) / t
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "fc_math.h"
#include "fc_lane.h"
#include "fc_row.h"
#include "../../include/flowcon_hip.h"

namespace fc {

template <int E>
__global__ __launch_bounds__(256) void radial_backward_kernel(const float* __restrict__ x, const float* __restrict__ gy,
                                                              const float* __restrict__ gl, const float* __restrict__ z0,
                                                              const float* __restrict__ a_ptr, const float* __restrict__ b_ptr,
                                                              float* __restrict__ gx, float* __restrict__ gz0,
                                                              float* __restrict__ ga, float* __restrict__ gb, int64_t n,
                                                              int d) {
  const float a = a_ptr[0], b = b_ptr[0];
  const int lane = threadIdx.x & 63;
  Row<E> zv, gzv;
  load_row<E>(zv, z0, d, lane);
#pragma unroll
  for (int e = 0; e < E; ++e) gzv.v[e] = 0.f;
  float gav = 0.f, gbv = 0.f;
  const int64_t stride = wave_unit_stride();
  for (int64_t row = wave_first_unit(); row < n; row += stride) {
    Row<E> dz, g;
    load_row<E>(dz, x + row * d, d, lane);
    load_row<E>(g, gy + row * d, d, lane);
#pragma unroll
    for (int e = 0; e < E; ++e) dz.v[e] -= zv.v[e];
    const float glr = gl ? gl[row] : 0.f;
    const float r = sqrtf(dot_rows<E>(dz, dz));
    const float c = dot_rows<E>(g, dz);
    const float ar = a + r, ar2 = ar * ar;
    const float h = b / ar, k = -b * r / ar2;
    const float g_k = glr / (1.f + h + k);
    const float g_h = c + glr * ((float)(d - 1) / (1.f + h)) + g_k;
    const float g_a = -g_h * b / ar2 + 2.f * g_k * b * r / (ar2 * ar);
    const float g_r = g_a - g_k * b / ar2;
    const float w = r > 0.f ? g_r / r : 0.f;
    gav += g_a;
    gbv += g_h / ar - g_k * r / ar2;
#pragma unroll
    for (int e = 0; e < E; ++e) {
      const float g_dz = h * g.v[e] + w * dz.v[e];
      gzv.v[e] -= g_dz;
      g.v[e] += g_dz;
    }
    store_row<E>(g, gx + row * d, d, lane);
  }
#pragma unroll
  for (int e = 0; e < E; ++e) {
    const int i = lane + 64 * e;
    if (i < d) atomicAdd(gz0 + i, gzv.v[e]);
  }
  if (lane == 0) {
    atomicAdd(ga, gav);
    atomicAdd(gb, gbv);
  }
}

template <int E>
__global__ __launch_bounds__(256) void unit_vector_backward_kernel(const float* __restrict__ in, const float* __restrict__ gout,
                                                                   const float* __restrict__ gl, float* __restrict__ gin,
                                                                   int64_t n, int d, int inverse) {
  const int lane = threadIdx.x & 63;
  const int d_in = inverse ? d + 1 : d, d_out = inverse ? d : d + 1;
  const int64_t stride = wave_unit_stride();
  for (int64_t row = wave_first_unit(); row < n; row += stride) {
    Row<E> v, g;
    load_row<E>(v, in + row * d_in, d_in, lane);
    load_row<E>(g, gout + row * d_out, d_out, lane);
    const float glr = gl ? gl[row] : 0.f;
    if (!inverse) {
      // v = x (zero from d on), g = gy with gy[d] in slot d
      const float sp1 = dot_rows<E>(v, v) + 1.f;
      const float c = dot_rows<E>(g, v);
      const float gyd = bcast<E>(g, d);
      const float big = 2.f * (gyd - c) / (sp1 * sp1) - glr * (float)d / sp1;
#pragma unroll
      for (int e = 0; e < E; ++e) g.v[e] = 2.f * g.v[e] / sp1 + 2.f * v.v[e] * big;
    } else {
      // v = y with y[d] in slot d, g = gx (zero from d on)
      const float t = 1.f - bcast<E>(v, d);
#pragma unroll
      for (int e = 0; e < E; ++e) v.v[e] = lane + 64 * e < d ? v.v[e] / t : 0.f;
      const float lw = glr * 2.f * (float)d / (1.f + dot_rows<E>(v, v));
#pragma unroll
      for (int e = 0; e < E; ++e) g.v[e] += lw * v.v[e];
      const float m = dot_rows<E>(g, v) / t;
#pragma unroll
      for (int e = 0; e < E; ++e) g.v[e] = lane + 64 * e == d ? m : g.v[e] / t;
    }
    store_row<E>(g, gin + row * d_in, d_in, lane);
  }
}

}  // namespace fc

extern "C" int fc_radial_backward(const float* x, const float* grad_y, const float* grad_logabsdet, const float* z0,
                                  const float* a, const float* b, float* grad_x, float* grad_z0, float* grad_a,
                                  float* grad_b, int64_t n, int32_t d, void* stream) {
  if (n < 0 || d <= 0 || d > fc::kMaxRowFeatures) return hipErrorInvalidValue;
  if (n == 0) return hipSuccess;
  if (!x || !grad_y || !z0 || !a || !b || !grad_x || !grad_z0 || !grad_a || !grad_b) return hipErrorInvalidValue;
  hipStream_t s = static_cast<hipStream_t>(stream);
  FC_ROW_DISPATCH(d, hipLaunchKernelGGL(fc::radial_backward_kernel<E>, dim3(fc::row_grid(n, fc::kReduceGridCap)), dim3(256), 0,
                                        s, x, grad_y, grad_logabsdet, z0, a, b, grad_x, grad_z0, grad_a, grad_b, n, d));
  return hipGetLastError();
}

extern "C" int fc_unit_vector_backward(const float* x_or_y, const float* grad_out, const float* grad_logabsdet,
                                       float* grad_in, int64_t n, int32_t d, int32_t inverse, void* stream) {
  if (n < 0 || d <= 0 || d + 1 > fc::kMaxRowFeatures) return hipErrorInvalidValue;
  if (n == 0) return hipSuccess;
  if (!x_or_y || !grad_out || !grad_in) return hipErrorInvalidValue;
  hipStream_t s = static_cast<hipStream_t>(stream);
  FC_ROW_DISPATCH(d + 1, hipLaunchKernelGGL(fc::unit_vector_backward_kernel<E>, dim3(fc::row_grid(n, fc::kReduceGridCap)),
                                            dim3(256), 0, s, x_or_y, grad_out, grad_logabsdet, grad_in, n, d, inverse));
  return hipGetLastError();
}
