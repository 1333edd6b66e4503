// Row-per-wavefront scaffold shared by every kernel of the family: fc_rowwave.hip (forward / inverse), fc_rowwave_backward.hip,
// fc_rowwave_backward_per_sample.hip, fc_rownorm.hip, fc_rownorm_backward.hip and fc_hdh_linear.hip.  One 64-lane wave owns one
// sample row, lane l holds elements l, l + 64, ... in registers (E <= 8, D <= kMaxRowFeatures).
//
// Held here once: the width -> E and lanes-per-row dispatch (FC_ROW_DISPATCH, FC_ROW_LANES), the grid clamp with its two caps
// (row_grid) and the wave's first unit and stride that every row loop walks (wave_first_unit, wave_unit_stride: the same
// kWavesPerBlock and the same "wave index" as the grid); and the planar backward formula that the shared-parameter and the
// per-sample kernel have in common (planar_backward_row).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "fc_lane.h"

namespace fc {

constexpr int kWavesPerBlock = 4;
constexpr int kMaxRowFeatures = 512;      // 8 registers of 64 lanes: the widest row the entry points take

// Grid caps, in workgroups of kWavesPerBlock waves; past the cap a wave walks several units (wave_unit_stride).
// Kernels that only stream rows (every output is written by the wave that owns the row): eight workgroups per CU of a
// 256-CU part.
constexpr int64_t kStreamGridCap = 256 * 8;
// Kernels that end in a batch reduction by atomics (each wave adds its register sums to the global result once, at the
// end): half as many waves, so half as many atomics per element of the result.
constexpr int64_t kReduceGridCap = 256 * 4;

// workgroups for `units` wave-sized units of work (rows, groups of 64 / L rows, groups of 4 or R rows)
inline unsigned row_grid(int64_t units, int64_t cap) {
  int64_t g = (units + kWavesPerBlock - 1) / kWavesPerBlock;
  if (g > cap) g = cap;
  return (unsigned)(g < 1 ? 1 : g);
}

// the unit a wave starts at and the distance to its next one, for a grid from row_grid:
//   for (int64_t row = wave_first_unit(); row < n; row += wave_unit_stride())
__device__ __forceinline__ int64_t wave_first_unit() { return (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6); }
__device__ __forceinline__ int64_t wave_unit_stride() { return (int64_t)gridDim.x * kWavesPerBlock; }

// registers per lane of a Row<E> that holds d features
inline int elems_for(int d) { return d <= 64 ? 1 : d <= 128 ? 2 : d <= 256 ? 4 : 8; }

// float4 row kernels: lanes per row (a power of two) for `pieces` 16-byte pieces, and the alignment they need
inline int lanes_for(int pieces) {
  int lanes = 1;
  while (lanes < pieces) lanes <<= 1;
  return lanes;
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

__device__ __forceinline__ float wave_sum(float v) { return wave64_allsum(v, threadIdx.x & 63); }
// the ds_bpermute butterfly: slower per reduction, but the shared-parameter Sylvester kernel runs faster with it
// (3.4 vs 5.4 ms at D = 128, M = 32, N = 2^18 -- its reductions overlap the column reads of the mat-vecs)
__device__ __forceinline__ float wave_sum_lds(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

template <int E>
struct Row {
  float v[E];
};

template <int E>
__device__ __forceinline__ void load_row(Row<E>& r, const float* __restrict__ p, int d, int lane) {
#pragma unroll
  for (int e = 0; e < E; ++e) {
    const int i = lane + 64 * e;
    r.v[e] = i < d ? p[i] : 0.f;
  }
}

template <int E>
__device__ __forceinline__ void store_row(const Row<E>& r, float* __restrict__ p, int d, int lane) {
#pragma unroll
  for (int e = 0; e < E; ++e) {
    const int i = lane + 64 * e;
    if (i < d) p[i] = r.v[e];
  }
}

template <int E, bool kLds = false>
__device__ __forceinline__ float dot_rows(const Row<E>& a, const Row<E>& b) {
  float s = 0.f;
#pragma unroll
  for (int e = 0; e < E; ++e) s += a.v[e] * b.v[e];
  return kLds ? wave_sum_lds(s) : wave_sum(s);
}

// x_j for a wave-uniform j: element j lives in register j/64 of lane j%64
template <int E>
__device__ __forceinline__ float bcast(const Row<E>& r, int j) {
  float out = 0.f;
#pragma unroll
  for (int e = 0; e < E; ++e) {
    // j is wave-uniform: v_readlane, no LDS traffic
    const float c = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(r.v[e]), j & 63));
    if ((j >> 6) == e) out = c;
  }
  return out;
}

// Backward of one planar row (formulas: header of fc_rowwave_backward.hip) from the row r, the upstream gradients g = gy and
// glr, the parameters w, u, b and uw = u.w.  Leaves g = gx and returns the factors of the row's parameter gradients (the
// shared-parameter kernel accumulates them over its rows, the per-sample kernel stores them); gb = g_a.
struct PlanarBackward {
  float g_a, t, c;
  __device__ __forceinline__ float gw(float r, float u) const { return g_a * r + c * u; }
  __device__ __forceinline__ float gu(float gy, float w) const { return t * gy + c * w; }
};

template <int E>
__device__ __forceinline__ PlanarBackward planar_backward_row(const Row<E>& r, Row<E>& g, const Row<E>& wv, const Row<E>& uv,
                                                              float b, float glr, float uw) {
  const float a = dot_rows<E>(r, wv) + b;
  const float t = tanhf(a);
  const float dt = 1.f - t * t;
  const float psi = 1.f + dt * uw;
  const float dl = glr * (psi >= 0.f ? 1.f : -1.f) / (1e-7f + fabsf(psi));      // d lad / d psi times gl
  const float g_t = dot_rows<E>(g, uv) - dl * (2.f * t * uw);
  const float g_a = g_t * dt;
  const float c = dl * dt;
#pragma unroll
  for (int e = 0; e < E; ++e) g.v[e] = g.v[e] + g_a * wv.v[e];
  return PlanarBackward{g_a, t, c};
}

}  // namespace fc

// CALL with `constexpr int E` = registers per lane for rows of D features
#define FC_ROW_DISPATCH(D, CALL)                   \
  switch (fc::elems_for(D)) {                      \
    case 1: { constexpr int E = 1; CALL; break; }  \
    case 2: { constexpr int E = 2; CALL; break; }  \
    case 4: { constexpr int E = 4; CALL; break; }  \
    default: { constexpr int E = 8; CALL; break; } \
  }

// CALL with `constexpr int L` = LANES (from fc::lanes_for: a power of two, at most 64)
#define FC_ROW_LANES(LANES, CALL)                   \
  switch (LANES) {                                  \
    case 1: { constexpr int L = 1; CALL; break; }   \
    case 2: { constexpr int L = 2; CALL; break; }   \
    case 4: { constexpr int L = 4; CALL; break; }   \
    case 8: { constexpr int L = 8; CALL; break; }   \
    case 16: { constexpr int L = 16; CALL; break; } \
    case 32: { constexpr int L = 32; CALL; break; } \
    default: { constexpr int L = 64; CALL; break; } \
  }
