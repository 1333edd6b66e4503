// Row-norm bijectors, gfx950: read a row, reduce its squared norm across the lanes that hold it, rescale the row, write it
// with one log-determinant.  HBM traffic is the row in, the row out and one logabsdet word.
//
// Restates (not copies):
//   flowcon/transforms/no_analytic_inv/planar.py:199-211   radial flow  y = x + h(r) (x - z0),  h = b / (a + r)
//   flowcon/transforms/unitvector.py:18-53                 stereographic map R^d -> S^d and back
// The radial INVERSE is an addition (the reference raises): with rho = |y - z0| the forward gives
// rho = r (1 + b / (a + r)), so r is the non-negative root of r^2 + (a + b - rho) r - a rho = 0, taken in the form that
// does not cancel.
//
// Three layouts, as the planar kernels have them (fc_rowwave.hip):
//   Row<E>   one wave per row, lane l holds elements l, l + 64, ... (any width <= 512)
//   pieces   L lanes per row, each a 4-float piece, 64 / L rows per wave; a side whose rows are a multiple of 4 floats long
//            (and 16-byte aligned) moves as 16-byte requests, the other side as scalars
//   narrow   rows of <= 16 floats, one per 16-lane DPP row, four per wave
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "fc_math.h"
#include "fc_lane.h"
#include "fc_row.h"
#include "../../include/flowcon_hip.h"

namespace fc {

constexpr float kLog2 = 0.69314718055994530942f;
constexpr float kSphereTol = 1e-4f;      // unitvector.py:40

// (factor on dz, logabsdet) of one row from its squared distance to z0.
// forward: y = x + h dz;  inverse: x = z0 + dz / (1 + h) at the recovered r, logabsdet negated.
__device__ __forceinline__ void radial_row(float sq, float a, float b, int d, bool inverse, float& factor, float& lad) {
  float r = sqrtf(sq);
  if (inverse) {
    const float rho = r, q = a + b - rho;
    const float root = sqrtf(q * q + 4.f * a * rho);
    r = q > 0.f ? 2.f * a * rho / (q + root) : (root - q) * 0.5f;
  }
  const float ar = a + r;
  const float h = b / ar;
  const float hr = -b * r / (ar * ar);
  const float ld = (float)(d - 1) * logf(1.f + h) + logf(1.f + h + hr);
  factor = inverse ? 1.f / (1.f + h) : h;
  lad = inverse ? -ld : ld;
}

template <int W>
__device__ __forceinline__ float group_sum(float v) {
#pragma unroll
  for (int o = W >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o, W);
  return v;
}

// ---- radial ---------------------------------------------------------------------------------------------------------

template <int E>
__global__ __launch_bounds__(256) void radial_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                     float* __restrict__ lad, const float* __restrict__ z0,
                                                     const float* __restrict__ a_ptr, const float* __restrict__ b_ptr,
                                                     int64_t n, int d, int inverse) {
  const float a = a_ptr[0], b = b_ptr[0];
  const int lane = threadIdx.x & 63;
  Row<E> zv;
  load_row<E>(zv, z0, d, lane);
  const int64_t stride = wave_unit_stride();
  for (int64_t row = wave_first_unit(); row < n; row += stride) {
    Row<E> r, dz;
    load_row<E>(r, x + row * d, d, lane);
    float s = 0.f;
#pragma unroll
    for (int e = 0; e < E; ++e) {
      dz.v[e] = r.v[e] - zv.v[e];
      s += dz.v[e] * dz.v[e];
    }
    s = wave_sum(s);
    float f, ld;
    radial_row(s, a, b, d, inverse != 0, f, ld);
#pragma unroll
    for (int e = 0; e < E; ++e) r.v[e] = inverse ? zv.v[e] + dz.v[e] * f : r.v[e] + f * dz.v[e];
    store_row<E>(r, y + row * d, d, lane);
    if (lane == 0 && lad) lad[row] = ld;
  }
}

// rows of 4 L' <= 4 L floats, 16-byte aligned: L lanes carry a row as float4 pieces, the next group's rows requested before
// this group's arithmetic (planar_rows4_kernel's structure)
template <int L>
__global__ __launch_bounds__(256) void radial_rows4_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                           float* __restrict__ lad, const float* __restrict__ z0,
                                                           const float* __restrict__ a_ptr, const float* __restrict__ b_ptr,
                                                           int64_t n, int d, int inverse) {
  constexpr int kRows = 64 / L;
  const float a = a_ptr[0], b = b_ptr[0];
  const int lane = threadIdx.x & 63, sub = lane % L, rw = lane / L;
  const int d4 = d >> 2;
  const bool live = sub < d4;
  const float4 zero4 = float4{0.f, 0.f, 0.f, 0.f};
  // (an if, not a ?: -- selecting between two float4 lvalues selects an ADDRESS and puts the zero vector in scratch)
  float4 zv = zero4;
  if (live) zv = reinterpret_cast<const float4*>(z0)[sub];
  const int64_t groups = (n + kRows - 1) / kRows;
  const int64_t stride = wave_unit_stride();
  int64_t grp = wave_first_unit();
  auto fetch = [&](int64_t g) {
    const int64_t row = g * kRows + rw;
    float4 v = zero4;
    if (live && row < n) v = reinterpret_cast<const float4*>(x + row * d)[sub];
    return v;
  };
  float4 rnext = zero4;
  if (grp < groups) rnext = fetch(grp);
  for (; grp < groups; grp += stride) {
    const int64_t row = grp * kRows + rw;
    const float4 r = rnext;
    if (grp + stride < groups) rnext = fetch(grp + stride);
    const float4 dz = float4{r.x - zv.x, r.y - zv.y, r.z - zv.z, r.w - zv.w};
    const float s = group_sum<L>((dz.x * dz.x + dz.y * dz.y) + (dz.z * dz.z + dz.w * dz.w));
    float f, ld;
    radial_row(s, a, b, d, inverse != 0, f, ld);
    // inverse: z0 + dz f;  forward: x + f dz
    const float4 base = float4{inverse ? zv.x : r.x, inverse ? zv.y : r.y, inverse ? zv.z : r.z, inverse ? zv.w : r.w};
    if (live && row < n)
      reinterpret_cast<float4*>(y + row * d)[sub] =
          float4{base.x + f * dz.x, base.y + f * dz.y, base.z + f * dz.z, base.w + f * dz.w};
    if (sub == 0 && row < n && lad) lad[row] = ld;
  }
}

// rows of <= 16 floats: four rows per wave, one per 16-lane DPP row
__global__ __launch_bounds__(256) void radial_narrow_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                            float* __restrict__ lad, const float* __restrict__ z0,
                                                            const float* __restrict__ a_ptr, const float* __restrict__ b_ptr,
                                                            int64_t n, int d, int inverse) {
  const float a = a_ptr[0], b = b_ptr[0];
  const int lane = threadIdx.x & 63, j = lane & 15;
  const float zv = j < d ? z0[j] : 0.f;
  const int64_t stride = wave_unit_stride() * 4;
  for (int64_t base = wave_first_unit() * 4; base < n; base += stride) {
    const int64_t row = base + (lane >> 4);
    const bool live = row < n && j < d;
    const float v = live ? x[row * d + j] : 0.f;
    const float dz = live ? v - zv : 0.f;
    const float s = row16_allsum(dz * dz);
    float f, ld;
    radial_row(s, a, b, d, inverse != 0, f, ld);
    if (live) y[row * d + j] = inverse ? zv + dz * f : v + f * dz;
    if (lad && row < n && j == 0) lad[row] = ld;
  }
}

// ---- unit vector ----------------------------------------------------------------------------------------------------
// forward:  s = |x|^2;  y[:d] = 2 x / (s + 1),  y[d] = (s - 1) / (s + 1);  lad = d (log 2 - log1p(s))
// inverse:  x = y[:d] / (1 - y[d]);  lad = -d (log 2 - log1p(|x|^2));  a row with | |y|^2 - 1 | > 1e-4 sets the domain bit

__device__ __forceinline__ float unit_lad(float s, int d, bool inverse) {
  const float ld = (float)d * (kLog2 - log1pf(s));
  return inverse ? -ld : ld;
}

template <int E>
__global__ __launch_bounds__(256) void unit_vector_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                          float* __restrict__ lad, uint32_t* __restrict__ err, int64_t n,
                                                          int d, int inverse) {
  const int lane = threadIdx.x & 63;
  const int d_in = inverse ? d + 1 : d, d_out = inverse ? d : d + 1;
  bool outside = false;
  const int64_t stride = wave_unit_stride();
  for (int64_t row = wave_first_unit(); row < n; row += stride) {
    Row<E> r;
    load_row<E>(r, x + row * d_in, d_in, lane);
    float s = dot_rows<E>(r, r);
    if (!inverse) {
      const float sp1 = s + 1.f;
#pragma unroll
      for (int e = 0; e < E; ++e) {
        const int i = lane + 64 * e;
        r.v[e] = i == d ? (s - 1.f) / sp1 : (2.f * r.v[e]) / sp1;
      }
    } else {
      outside |= fabsf(s - 1.f) > kSphereTol;
      const float t = 1.f - bcast<E>(r, d);
#pragma unroll
      for (int e = 0; e < E; ++e) {
        const int i = lane + 64 * e;
        r.v[e] = i < d ? r.v[e] / t : 0.f;
      }
      s = dot_rows<E>(r, r);
    }
    store_row<E>(r, y + row * d_out, d_out, lane);
    if (lane == 0 && lad) lad[row] = unit_lad(s, d, inverse != 0);
  }
  if (outside && err && lane == 0) atomicOr(err, FC_ERR_OUTSIDE_DOMAIN);
}

template <bool kVec>
__device__ __forceinline__ float4 load_piece(const float* __restrict__ row, int sub, int len) {
  const int i = 4 * sub;
  if (kVec) {
    float4 v = float4{0.f, 0.f, 0.f, 0.f};
    if (i < len) v = reinterpret_cast<const float4*>(row)[sub];
    return v;
  }
  return float4{i < len ? row[i] : 0.f, i + 1 < len ? row[i + 1] : 0.f, i + 2 < len ? row[i + 2] : 0.f,
                i + 3 < len ? row[i + 3] : 0.f};
}

template <bool kVec>
__device__ __forceinline__ void store_piece(float* __restrict__ row, int sub, int len, const float4& v) {
  const int i = 4 * sub;
  if (kVec) {
    if (i < len) reinterpret_cast<float4*>(row)[sub] = v;
    return;
  }
  if (i < len) row[i] = v.x;
  if (i + 1 < len) row[i + 1] = v.y;
  if (i + 2 < len) row[i + 2] = v.z;
  if (i + 3 < len) row[i + 3] = v.w;
}

// L lanes per row (4 L >= d), 64 / L rows per wave.  kVecD: the R^d side (d % 4 == 0) moves as float4 and the sphere side
// as scalars; otherwise the sphere side ((d + 1) % 4 == 0) moves as float4.  When the pieces end exactly at d (4 L == d: D = 64
// on 16 lanes, four rows per wave) no lane's piece holds the sphere's last coordinate: the group's first lane writes it, every
// lane of the group reads it.
template <int L, bool kVecD>
__global__ __launch_bounds__(256) void unit_vector_pieces_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                                 float* __restrict__ lad, uint32_t* __restrict__ err,
                                                                 int64_t n, int d, int inverse) {
  constexpr int kRows = 64 / L;
  const int lane = threadIdx.x & 63, sub = lane % L, rw = lane / L;
  const int i0 = 4 * sub;
  const bool last_apart = 4 * L <= d;
  bool outside = false;
  const int64_t groups = (n + kRows - 1) / kRows;
  const int64_t stride = wave_unit_stride();
  for (int64_t grp = wave_first_unit(); grp < groups; grp += stride) {
    const int64_t row = grp * kRows + rw;
    const bool live = row < n;
    const int64_t rr = live ? row : n - 1;
    float s;
    float4 out;
    if (!inverse) {
      const float4 p = load_piece<kVecD>(x + rr * d, sub, d);
      s = group_sum<L>((p.x * p.x + p.y * p.y) + (p.z * p.z + p.w * p.w));
      const float sp1 = s + 1.f, last = (s - 1.f) / sp1;
      out = float4{i0 == d ? last : (2.f * p.x) / sp1, i0 + 1 == d ? last : (2.f * p.y) / sp1,
                   i0 + 2 == d ? last : (2.f * p.z) / sp1, i0 + 3 == d ? last : (2.f * p.w) / sp1};
      if (live) store_piece<!kVecD>(y + row * (int64_t)(d + 1), sub, d + 1, out);
      if (last_apart && sub == 0 && live) y[row * (int64_t)(d + 1) + d] = last;
    } else {
      const float4 p = load_piece<!kVecD>(x + rr * (int64_t)(d + 1), sub, d + 1);
      const float apart = last_apart ? x[rr * (int64_t)(d + 1) + d] : 0.f;
      const float ysq = group_sum<L>((p.x * p.x + p.y * p.y) + (p.z * p.z + p.w * p.w)) + apart * apart;
      const float yd = group_sum<L>((i0 == d ? p.x : 0.f) + (i0 + 1 == d ? p.y : 0.f) + (i0 + 2 == d ? p.z : 0.f) +
                                    (i0 + 3 == d ? p.w : 0.f)) + apart;
      outside |= live && fabsf(ysq - 1.f) > kSphereTol;
      const float t = 1.f - yd;
      out = float4{i0 < d ? p.x / t : 0.f, i0 + 1 < d ? p.y / t : 0.f, i0 + 2 < d ? p.z / t : 0.f,
                   i0 + 3 < d ? p.w / t : 0.f};
      s = group_sum<L>((out.x * out.x + out.y * out.y) + (out.z * out.z + out.w * out.w));
      if (live) store_piece<kVecD>(y + row * d, sub, d, out);
    }
    if (sub == 0 && live && lad) lad[row] = unit_lad(s, d, inverse != 0);
  }
  if (outside && err) atomicOr(err, FC_ERR_OUTSIDE_DOMAIN);
}

// d + 1 <= 16: four rows per wave, one per 16-lane DPP row
__global__ __launch_bounds__(256) void unit_vector_narrow_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                                 float* __restrict__ lad, uint32_t* __restrict__ err,
                                                                 int64_t n, int d, int inverse) {
  const int lane = threadIdx.x & 63, j = lane & 15;
  const int d_in = inverse ? d + 1 : d, d_out = inverse ? d : d + 1;
  bool outside = false;
  const int64_t stride = wave_unit_stride() * 4;
  for (int64_t base = wave_first_unit() * 4; base < n; base += stride) {
    const int64_t row = base + (lane >> 4);
    const bool live = row < n;
    float v = (live && j < d_in) ? x[row * d_in + j] : 0.f;
    float s = row16_allsum(v * v);
    if (!inverse) {
      const float sp1 = s + 1.f;
      v = j == d ? (s - 1.f) / sp1 : (2.f * v) / sp1;
    } else {
      outside |= live && fabsf(s - 1.f) > kSphereTol;
      const float t = 1.f - row16_allsum(j == d ? v : 0.f);
      v = j < d ? v / t : 0.f;
      s = row16_allsum(v * v);
    }
    if (live && j < d_out) y[row * d_out + j] = v;
    if (lad && live && j == 0) lad[row] = unit_lad(s, d, inverse != 0);
  }
  if (outside && err) atomicOr(err, FC_ERR_OUTSIDE_DOMAIN);
}

}  // namespace fc

extern "C" int fc_radial(const float* x, float* y, float* logabsdet, const float* z0, const float* a, const float* b,
                         int64_t n, int32_t d, int32_t inverse, void* stream) {
  if (n < 0 || d <= 0 || d > fc::kMaxRowFeatures) return hipErrorInvalidValue;
  if (n == 0) return hipSuccess;
  if (!x || !y || !z0 || !a || !b) return hipErrorInvalidValue;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (d % 4 == 0 && d <= 256 && fc::aligned16(x) && fc::aligned16(y) && fc::aligned16(z0)) {
    const int lanes = fc::lanes_for(d / 4);
    const int rows = 64 / lanes;
    const unsigned grid = fc::row_grid((n + rows - 1) / rows, fc::kStreamGridCap);
    FC_ROW_LANES(lanes, hipLaunchKernelGGL(fc::radial_rows4_kernel<L>, dim3(grid), dim3(256), 0, s, x, y, logabsdet, z0, a,
                                          b, n, d, inverse));
    return hipGetLastError();
  }
  if (d <= 16) {
    hipLaunchKernelGGL(fc::radial_narrow_kernel, dim3(fc::row_grid((n + 3) / 4, fc::kStreamGridCap)), dim3(256), 0, s, x, y,
                       logabsdet, z0, a, b, n, d, inverse);
    return hipGetLastError();
  }
  FC_ROW_DISPATCH(d, hipLaunchKernelGGL(fc::radial_kernel<E>, dim3(fc::row_grid(n, fc::kStreamGridCap)), dim3(256), 0, s, x, y,
                                        logabsdet, z0, a, b, n, d, inverse));
  return hipGetLastError();
}

extern "C" int fc_unit_vector(const float* x, float* y, float* logabsdet, uint32_t* err, int64_t n, int32_t d,
                              int32_t inverse, void* stream) {
  if (n < 0 || d <= 0 || d + 1 > fc::kMaxRowFeatures) return hipErrorInvalidValue;
  if (n == 0) return hipSuccess;
  if (!x || !y) return hipErrorInvalidValue;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int wide = d + 1;
  if (wide <= 16) {
    hipLaunchKernelGGL(fc::unit_vector_narrow_kernel, dim3(fc::row_grid((n + 3) / 4, fc::kStreamGridCap)), dim3(256), 0, s, x,
                       y, logabsdet, err, n, d, inverse);
    return hipGetLastError();
  }
  // the side that moves as 16-byte pieces: R^d rows when d % 4 == 0, sphere rows when (d + 1) % 4 == 0
  const float* d_side = inverse ? y : x;
  const float* s_side = inverse ? x : y;
  const bool vec_d = d % 4 == 0 && fc::aligned16(d_side), vec_s = wide % 4 == 0 && fc::aligned16(s_side);
  if ((vec_d && d <= 256) || (vec_s && wide <= 256)) {
    const int lanes = fc::lanes_for(vec_d ? d / 4 : wide / 4);
    const int rows = 64 / lanes;
    const unsigned grid = fc::row_grid((n + rows - 1) / rows, fc::kStreamGridCap);
    if (vec_d) {
      FC_ROW_LANES(lanes, hipLaunchKernelGGL((fc::unit_vector_pieces_kernel<L, true>), dim3(grid), dim3(256), 0, s, x, y,
                                            logabsdet, err, n, d, inverse));
    } else {
      FC_ROW_LANES(lanes, hipLaunchKernelGGL((fc::unit_vector_pieces_kernel<L, false>), dim3(grid), dim3(256), 0, s, x, y,
                                            logabsdet, err, n, d, inverse));
    }
    return hipGetLastError();
  }
  FC_ROW_DISPATCH(wide, hipLaunchKernelGGL(fc::unit_vector_kernel<E>, dim3(fc::row_grid(n, fc::kStreamGridCap)), dim3(256), 0,
                                           s, x, y, logabsdet, err, n, d, inverse));
  return hipGetLastError();
}
