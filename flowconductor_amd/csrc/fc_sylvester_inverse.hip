// Inverse of the shared-parameter Sylvester flow's triangular middle, gfx950 (the reference has no inverse:
// no_analytic_inv/planar.py:168 raises).
//
// In the coordinates rotated by Q the map is c = v + R2 tanh(R1 v + b) with upper-triangular R1 / R2, so v follows by
// back substitution, j = d-1 .. 0:
//   s = b_j + sum_{k>j} R1[j][k] v_k,   t = c_j - sum_{k>j} R2[j][k] th_k,   th_k = tanh(R1 v + b)_k
//   v_j = the root of  g(v) = v + r2 tanh(r1 v + s) - t,   r1 = R1[j][j], r2 = R2[j][j]
// g' = 1 + r1 r2 (1 - tanh^2) lies in [1 - |r1 r2|, 1 + |r1 r2|] and |r1 r2| < 1, so the root is unique and lies in
// [t - |r2|, t + |r2|].  logabsdet = -sum_j log g'(v_j): minus the forward's own expression at the solution.
//
// ONE LANE PER ROW, 64 rows per wavefront: the scalar solve is per row, so every lane does useful work in it and no
// step needs a cross-lane sum.  A wavefront keeps v_k and th_k of its 64 rows in LDS as [d][64] floats each
// (2 * d * 256 bytes: 64 KB at d = 128, hence d <= 128); c is staged into the v image by coalesced reads and solved in
// place, v leaves by coalesced writes.  Column j of the image is rotated by j lanes (slot (row + j) & 63), so that both
// the per-column accesses of the solve (64 rows, one column) and the transposing accesses of the staging (one row, 32
// columns) fall on distinct banks.
//
// Columns are taken in blocks of 16: the block's 16 s and 16 t values are accumulated in registers while the later
// columns k are walked once (one LDS read of v_k and of th_k per 16 rows of R), then the 16 solves run with the
// in-block updates unrolled.
//
// R1 / R2 entries are the same for every lane and come transposed, so that the 16 rows of a block are contiguous.  At
// d = 128 the LDS admits one wave per SIMD on two SIMDs of a CU: nothing hides a load's latency but the wave's own
// arithmetic, so the loads must be in flight several columns ahead.  Scalar loads cannot be (they return out of order:
// every use waits for all of them, and two columns of 32 values do not fit the scalar registers beside the rest: 150
// spills); the entries are therefore read by VECTOR loads of one address for all lanes (the index carries a per-lane
// zero the compiler cannot see through), which return in order into the plentiful vector registers: a ring of four
// columns while the later columns are walked, the next column during each Newton search.  Measured at d = 128,
// n = 2^18: scalar operands 2.23 ms, vector loads two columns deep 1.70 ms, with the tile staged 16 loads deep 1.52 ms,
// four columns deep 1.36 ms.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "fc_math.h"
#include "fc_device.h"
#include "../../include/flowcon_hip.h"

namespace fc {

constexpr int kSylInvBlock = 16;      // columns per register block
constexpr int kSylInvMaxEval = 16;    // evaluations of g per scalar solve, at most
constexpr int kSylInvMaxD = 128;
constexpr int kSylInvStage = 16;     // elements per lane in flight while a tile is staged in or out
constexpr int kSylInvLdsBytes = 160 * 1024;

// Root of g(v) = v + r2 tanh(r1 v + s) - t by a bracketed Newton search; returns v and th = tanh(r1 v + s) AT that v.
// Every evaluation moves one end of the bracket to the current point by the sign of g; the next point is the Newton
// iterate when it lies in the CLOSED bracket (its ends are points already visited: a strict test would reject every
// iterate next to the current point and degrade to bisection), else the midpoint.  Stops when |g| is at the rounding
// level of its own evaluation, 2^-22 (|t| + |r2|) (v, r2 th and t are each rounded once at that magnitude), when the
// step no longer changes v, or after kSylInvMaxEval evaluations; a NaN residual stops at once (the row is NaN).
__device__ __forceinline__ void sylvester_solve(float r1, float r2, float rd, float s, float t, float& v_out,
                                                float& th_out) {
  const float ar2 = fabsf(r2);
  const float tol = 2.384185791015625e-07f * (fabsf(t) + ar2);
  float lo = t - ar2, hi = t + ar2;
  float v = t, th = 0.f;
  for (int it = 0; it < kSylInvMaxEval; ++it) {
    th = tanh_lean(r1 * v + s);
    const float g = (v + r2 * th) - t;
    if (!(fabsf(g) > tol) || it == kSylInvMaxEval - 1) break;
    lo = g < 0.f ? v : lo;
    hi = g > 0.f ? v : hi;
    const float slope = 1.f + rd * (1.f - th * th);
    float vn = v - div_lean(g, slope);
    if (!(vn >= lo && vn <= hi)) vn = 0.5f * (lo + hi);
    if (vn == v) break;
    v = vn;
  }
  v_out = v;
  th_out = th;
}

// The 16 solves of the block of columns jb .. jb + 15 (kFull: all of them exist; otherwise those below d) from the
// block's s / t values, which already hold the contributions of every later block.
template <bool kFull>
__device__ __forceinline__ void sylvester_inverse_block(float (&s)[kSylInvBlock], float (&t)[kSylInvBlock], float& ld,
                                                        float* vb, float* tb, const float* __restrict__ r1t,
                                                        const float* __restrict__ r2t, int jb, int d, int lane,
                                                        int z) {
  // a1 / a2: column j of R1 / R2 within the block, R[jb + ii][j] for ii = 0 .. jj (the diagonal entry last).  In a full
  // block the column of the NEXT solve is requested before this one's Newton search, whose arithmetic then covers the
  // loads' latency (a wave has the SIMD to itself at d = 128: nothing else would)
  float a1[kSylInvBlock], a2[kSylInvBlock], n1[kSylInvBlock], n2[kSylInvBlock];
  if constexpr (kFull) {
    const int64_t col = (int64_t)(jb + kSylInvBlock - 1) * d + jb + z;
#pragma unroll
    for (int ii = 0; ii < kSylInvBlock; ++ii) {
      a1[ii] = r1t[col + ii];
      a2[ii] = r2t[col + ii];
    }
  }
#pragma unroll
  for (int jj = kSylInvBlock - 1; jj >= 0; --jj) {
    const int j = jb + jj;
    if (!kFull && j >= d) continue;
    if constexpr (kFull) {
      const int64_t col = (int64_t)(j - 1) * d + jb + z;
#pragma unroll
      for (int ii = 0; ii < jj; ++ii) {
        n1[ii] = r1t[col + ii];
        n2[ii] = r2t[col + ii];
      }
    } else {
      const int64_t col = (int64_t)j * d + jb + z;
#pragma unroll
      for (int ii = 0; ii <= jj; ++ii) {
        a1[ii] = r1t[col + ii];
        a2[ii] = r2t[col + ii];
      }
    }
    const float r1 = a1[jj], r2 = a2[jj];
    const float rd = r1 * r2;
    float v, th;
    sylvester_solve(r1, r2, rd, s[jj], t[jj], v, th);
    ld += log_lean(1.f + (1.f - th * th) * rd);
    const int slot = j * 64 + ((lane + j) & 63);
    vb[slot] = v;
    tb[slot] = th;
#pragma unroll
    for (int ii = 0; ii < jj; ++ii) {
      s[ii] = __builtin_fmaf(a1[ii], v, s[ii]);
      t[ii] = __builtin_fmaf(-a2[ii], th, t[ii]);
    }
    if constexpr (kFull) {
#pragma unroll
      for (int ii = 0; ii < jj; ++ii) {
        a1[ii] = n1[ii];
        a2[ii] = n2[ii];
      }
    }
  }
}

// Column k of the transposed R1 / R2 restricted to the block's rows (16 contiguous, wave-uniform values each) and this
// row's v_k / th_k; `live` == false (k clamped past the end) zeroes the pair, so that the sums take nothing from it.
struct SylInvColumn {
  float a1[kSylInvBlock], a2[kSylInvBlock], vk, thk;
};
__device__ __forceinline__ void sylvester_inverse_request(SylInvColumn& c, const float* vb, const float* tb,
                                                          const float* __restrict__ r1t, const float* __restrict__ r2t,
                                                          int k, bool live, int jb, int d, int lane, int z) {
  const int slot = k * 64 + ((lane + k) & 63);
  c.vk = live ? vb[slot] : 0.f;
  c.thk = live ? tb[slot] : 0.f;
  const int64_t col = (int64_t)k * d + jb + z;
#pragma unroll
  for (int ii = 0; ii < kSylInvBlock; ++ii) {
    c.a1[ii] = r1t[col + ii];
    c.a2[ii] = r2t[col + ii];
  }
}
__device__ __forceinline__ void sylvester_inverse_accumulate(float (&s)[kSylInvBlock], float (&t)[kSylInvBlock],
                                                             const SylInvColumn& c) {
#pragma unroll
  for (int ii = 0; ii < kSylInvBlock; ++ii) {
    s[ii] = __builtin_fmaf(c.a1[ii], c.vk, s[ii]);
    t[ii] = __builtin_fmaf(-c.a2[ii], c.thk, t[ii]);
  }
}

__global__ __launch_bounds__(256) void sylvester_inverse_kernel(const float* __restrict__ c, float* __restrict__ v,
                                                                float* __restrict__ lad, const float* __restrict__ r1t,
                                                                const float* __restrict__ r2t,
                                                                const float* __restrict__ bias, int64_t n, int d) {
  extern __shared__ __attribute__((aligned(16))) float sylinv_lds[];
  const int lane = threadIdx.x & 63;
  int z = 0;
  asm volatile("" : "+v"(z));      // a zero the compiler cannot see through
  const int wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
  float* vb = sylinv_lds + (size_t)wave * 2 * d * 64;      // this wave's [d][64] image of c, then v
  float* tb = vb + d * 64;                                  // and of th
  const float inv_d = 1.f / (float)d;
  const int64_t tiles = (n + 63) / 64;
  const int last = (d - 1) / kSylInvBlock * kSylInvBlock;   // first column of the last (possibly partial) block
  for (int64_t tile = (int64_t)blockIdx.x * waves + wave; tile < tiles; tile += (int64_t)gridDim.x * waves) {
    const int64_t base = tile * 64 * d;                     // first element of the tile, row-major [64][d]
    const int64_t left = n * d - base;                      // elements that exist from there on
    // stage c: element e of the tile is (row e / d, column e % d); (e + 0.5) / d is at least 1 / 256 away from an
    // integer and below 64, so the f32 product with 1 / d truncates to the exact quotient
    // kSylInvStage loads are requested before the first is used (one at a time the wave waits out a full memory latency
    // per 64 elements); an element past the end of the tile or of the batch is read from a clamped, valid address and
    // replaced by zero: rows beyond n are never read
    const int count = left < 64 * d ? (int)left : 64 * d;   // elements of this tile that exist (>= 1)
    for (int i0 = 0; i0 < d; i0 += kSylInvStage) {
      float x[kSylInvStage];
#pragma unroll
      for (int u = 0; u < kSylInvStage; ++u) {
        const int e = (i0 + u) * 64 + lane;
        x[u] = c[base + (e < count ? e : count - 1)];
      }
#pragma unroll
      for (int u = 0; u < kSylInvStage; ++u) {
        const int e = (i0 + u) * 64 + lane;
        const int r = (int)(((float)e + 0.5f) * inv_d);
        const int j = e - r * d;
        if (i0 + u < d) vb[j * 64 + ((r + j) & 63)] = e < count ? x[u] : 0.f;
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    float ld = 0.f;
    for (int jb = last; jb >= 0; jb -= kSylInvBlock) {
      float s[kSylInvBlock], t[kSylInvBlock];
#pragma unroll
      for (int ii = 0; ii < kSylInvBlock; ++ii) {
        const int j = jb + ii < d ? jb + ii : d - 1;        // a column past d is never solved; its s / t are unused
        s[ii] = bias[j];
        t[ii] = vb[j * 64 + ((lane + j) & 63)];
      }
      // later columns k: all solved, and all rows jb .. jb + 15 exist.  Four columns per trip in a ring of four buffers:
      // a column is requested three columns (96 FMAs) before its own FMAs run; a column index past the end is clamped
      // (a valid address) and contributes zero
      const int k0 = jb + kSylInvBlock;
      if (k0 < d) {
        SylInvColumn c0, c1, c2, c3;
        auto request = [&](SylInvColumn& col, int k) __attribute__((always_inline)) {
          sylvester_inverse_request(col, vb, tb, r1t, r2t, k < d ? k : d - 1, k < d, jb, d, lane, z);
        };
        request(c0, k0);
        request(c1, k0 + 1);
        request(c2, k0 + 2);
        for (int k = k0; k < d; k += 4) {
          request(c3, k + 3);
          sylvester_inverse_accumulate(s, t, c0);
          request(c0, k + 4);
          sylvester_inverse_accumulate(s, t, c1);
          request(c1, k + 5);
          sylvester_inverse_accumulate(s, t, c2);
          request(c2, k + 6);
          sylvester_inverse_accumulate(s, t, c3);
        }
      }
      if (jb + kSylInvBlock <= d) sylvester_inverse_block<true>(s, t, ld, vb, tb, r1t, r2t, jb, d, lane, z);
      else sylvester_inverse_block<false>(s, t, ld, vb, tb, r1t, r2t, jb, d, lane, z);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    for (int i0 = 0; i0 < d; i0 += kSylInvStage) {
      float x[kSylInvStage];
#pragma unroll
      for (int u = 0; u < kSylInvStage; ++u) {
        const int e = (i0 + u < d ? i0 + u : d - 1) * 64 + lane;
        const int r = (int)(((float)e + 0.5f) * inv_d);
        const int j = e - r * d;
        x[u] = vb[j * 64 + ((r + j) & 63)];
      }
#pragma unroll
      for (int u = 0; u < kSylInvStage; ++u) {
        const int e = (i0 + u) * 64 + lane;
        if (i0 + u < d && e < count) v[base + e] = x[u];
      }
    }
    if (tile * 64 + lane < n) lad[tile * 64 + lane] = -ld;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();                        // the next tile's staging overwrites the image
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }
}

}  // namespace fc

extern "C" int fc_sylvester_inverse(const float* c, float* v, float* logabsdet, const float* r1_t, const float* r2_t,
                                    const float* bias, int64_t n, int32_t d, void* stream) {
  if (n < 0 || d <= 0 || d > fc::kSylInvMaxD) return hipErrorInvalidValue;
  if (n == 0) return hipSuccess;
  if (!c || !v || !logabsdet || !r1_t || !r2_t || !bias || c == v) return hipErrorInvalidValue;
  // waves per workgroup from the LDS image of one wave (2 * d * 256 bytes): 4 up to d = 80, 2 at d = 128
  const int per_wave = 2 * d * 64 * (int)sizeof(float);
  int waves = fc::kSylInvLdsBytes / per_wave;
  if (waves > 4) waves = 4;
  const int64_t tiles = (n + 63) / 64;
  if (waves > tiles) waves = (int)tiles;
  static fc::PerDeviceOnce attr;
  const hipError_t ea = fc::ensure_max_dynamic_lds(attr, reinterpret_cast<const void*>(&fc::sylvester_inverse_kernel),
                                                   fc::kSylInvLdsBytes);
  if (ea != hipSuccess) return ea;
  int64_t grid = (tiles + waves - 1) / waves;
  const int64_t cap = (int64_t)fc::device_cu_count() * 8;
  if (grid > cap) grid = cap;
  hipLaunchKernelGGL(fc::sylvester_inverse_kernel, dim3((unsigned)grid), dim3(64 * waves), (size_t)waves * per_wave,
                     static_cast<hipStream_t>(stream), c, v, logabsdet, r1_t, r2_t, bias, n, d);
  return hipGetLastError();
}
