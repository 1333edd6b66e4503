// Householder - diagonal - Householder linear map with batch-shared parameters, fused, and its backward.  gfx950.
//
//   y = post + H_b( scale o H_a( x - pre ) )
//
// H_a / H_b: Householder sequences q_a [Ka, d] / q_b [Kb, d] (each in index order or reversed), the arithmetic of
// fc::householder (fc_rowwave.hip): v - (v . q)(2 / |q|^2) q.  Both directions of SVDLinear (flowcon/transforms/svd.py:56-95)
// are this map: forward a = orthogonal_2, b = orthogonal_1, scale = diagonal, post = bias; inverse a = orthogonal_1
// reversed, b = orthogonal_2 reversed, scale = 1 / diagonal, pre = bias (the bias comes off before anything else).
//
// One wave owns one sample row in registers (fc_row.h).  What a composition of fc_householder / fc_pointwise_affine
// launches pays per row and this kernel pays once per workgroup: the 2 / |q_k|^2 of every reflection (a prologue, one
// wave per q row, results in LDS), so a reflection costs ONE wave reduction per row; and, when they fit kLdsBudget, the q
// rows themselves (staged zero-padded to 64 E floats, so a lane's reads need no bounds test and never conflict).
//
// LDS budget: kLdsBudget = 64 KiB per workgroup (table + staged rows forward; table + gradient rows + staged rows
// backward).  A workgroup at the budget still leaves room for a second one on the CU's 160 KiB, and 64 KiB is what a
// launch may ask for without raising the function's dynamic-LDS limit.  Past it the q rows come from global memory
// (they are a few hundred KiB at most and stay in L2), and the backward keeps its gradient rows in registers, walking
// the sequence in chunks as householder_backward_kernel does.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "fc_math.h"
#include "fc_lane.h"
#include "fc_row.h"
#include "../../include/flowcon_hip.h"

namespace fc {

constexpr int kHdhLdsBudget = 64 * 1024;
constexpr int kHdhMaxReflections = 4096;      // ka + kb: the coefficient table (16 KiB) always lives in LDS
constexpr int kHdhChunk = 8;                  // positions whose gradients the register form of the backward holds at a time

// 2 / |q_k|^2 of the rows of both sequences (table index k: q_a rows first, then q_b rows), one wave per row; with
// kStage the rows are left in LDS as well.  Ends with the workgroup barrier.
template <int E, bool kStage>
__device__ __forceinline__ void hdh_prologue(float* __restrict__ coef, float* __restrict__ qs, const float* __restrict__ qa,
                                             const float* __restrict__ qb, int d, int ka, int kb, int lane) {
  for (int k = threadIdx.x >> 6; k < ka + kb; k += kWavesPerBlock) {
    Row<E> qv;
    load_row<E>(qv, k < ka ? qa + (int64_t)k * d : qb + (int64_t)(k - ka) * d, d, lane);
    const float sq = dot_rows<E>(qv, qv);
    if (lane == 0) coef[k] = 2.f / sq;
    if constexpr (kStage) {
#pragma unroll
      for (int e = 0; e < E; ++e) qs[k * (64 * E) + lane + 64 * e] = qv.v[e];
    }
  }
  __syncthreads();
}

// row k of the table: from LDS (staged) or from global memory
template <int E, bool kStage>
__device__ __forceinline__ void hdh_q_row(Row<E>& qv, const float* __restrict__ qs, const float* __restrict__ qa,
                                          const float* __restrict__ qb, int k, int d, int ka, int lane) {
  if constexpr (kStage) {
#pragma unroll
    for (int e = 0; e < E; ++e) qv.v[e] = qs[k * (64 * E) + lane + 64 * e];
  } else {
    load_row<E>(qv, k < ka ? qa + (int64_t)k * d : qb + (int64_t)(k - ka) * d, d, lane);
  }
}

template <int E>
__device__ __forceinline__ void load_row_or(Row<E>& r, const float* __restrict__ p, int d, int lane, float fill) {
#pragma unroll
  for (int e = 0; e < E; ++e) {
    const int i = lane + 64 * e;
    r.v[e] = (p && i < d) ? p[i] : fill;
  }
}

// R rows per wave and step: the reflections of one row are a dependent chain (dot, reduce, update), two rows' chains
// interleave.
template <int E, int R, bool kStage>
__global__ __launch_bounds__(256) void hdh_linear_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                         const float* __restrict__ qa, const float* __restrict__ qb,
                                                         const float* __restrict__ scale, const float* __restrict__ pre,
                                                         const float* __restrict__ post, int64_t n, int d, int ka, int kb,
                                                         int reverse_a, int reverse_b) {
  extern __shared__ __attribute__((aligned(16))) float hdh_lds[];
  float* coef = hdh_lds;
  float* qs = hdh_lds + ((ka + kb + 3) & ~3);
  const int lane = threadIdx.x & 63;
  hdh_prologue<E, kStage>(coef, qs, qa, qb, d, ka, kb, lane);
  Row<E> sc, pr, po;
  load_row_or<E>(sc, scale, d, lane, 0.f);
  load_row_or<E>(pr, pre, d, lane, 0.f);
  load_row_or<E>(po, post, d, lane, 0.f);
  auto reflect = [&](Row<E> (&r)[R], int first, int count, bool reverse) __attribute__((always_inline)) {
    for (int t = 0; t < count; ++t) {
      const int k = first + (reverse ? count - 1 - t : t);
      Row<E> qv;
      hdh_q_row<E, kStage>(qv, qs, qa, qb, k, d, ka, lane);
      const float c = coef[k];
#pragma unroll
      for (int j = 0; j < R; ++j) {
        const float ip = dot_rows<E>(r[j], qv);
#pragma unroll
        for (int e = 0; e < E; ++e) r[j].v[e] = r[j].v[e] - ip * (c * qv.v[e]);
      }
    }
  };
  const int64_t stride = wave_unit_stride() * R;
  for (int64_t base = wave_first_unit() * R; base < n; base += stride) {
    Row<E> r[R];
#pragma unroll
    for (int j = 0; j < R; ++j) {
      const int64_t row = base + j < n ? base + j : n - 1;
      load_row<E>(r[j], x + row * d, d, lane);
#pragma unroll
      for (int e = 0; e < E; ++e) r[j].v[e] = r[j].v[e] - pr.v[e];
    }
    reflect(r, 0, ka, reverse_a != 0);
#pragma unroll
    for (int j = 0; j < R; ++j)
#pragma unroll
      for (int e = 0; e < E; ++e) r[j].v[e] = r[j].v[e] * sc.v[e];
    reflect(r, ka, kb, reverse_b != 0);
#pragma unroll
    for (int j = 0; j < R; ++j) {
#pragma unroll
      for (int e = 0; e < E; ++e) r[j].v[e] = r[j].v[e] + po.v[e];
      if (base + j < n) store_row<E>(r[j], y + (base + j) * d, d, lane);
    }
  }
}

// Backward from the saved output.  The map is a sequence of P = ka + 1 + kb invertible stages in application order:
// positions 0 .. ka-1 the reflections of H_a, position ka the scaling, positions ka+1 .. ka+kb the reflections of H_b.
// A row walks back from y - post: at a reflection (alpha = 2 / q.q, a_out = v.q, c = g.q) v <- H v restores its input,
// gq += -alpha (c v - a_out g) - alpha^2 a_out c q, g <- H g (fc_rowwave_backward.hip); at the scaling v <- v / scale,
// gscale += g v, g <- g scale.  gx = g at the end, gpost = sum gy, gpre = -sum gx.
//
// kMode 0 / 1: the gradient row of EVERY position lives in LDS (one row of 64 E floats each, all four waves add into it
// with LDS atomics as they pass), a row is walked once; mode 0 stages the q rows in LDS too.  kMode 2 (the rows do not
// fit kHdhLdsBudget): positions are taken in chunks of kHdhChunk from the output side, a wave keeps the chunk's gradient rows
// in registers over its rows and undoes the later positions first, as householder_backward_kernel<E, KQ> does; q from
// global memory.  In every mode the workgroup's sums meet in LDS and leave with ONE global atomic per element and
// workgroup.
template <int E, int kMode>
__global__ __launch_bounds__(256) void hdh_linear_backward_kernel(
    const float* __restrict__ y, const float* __restrict__ gy, const float* __restrict__ qa, const float* __restrict__ qb,
    const float* __restrict__ scale, const float* __restrict__ post, float* __restrict__ gx, float* __restrict__ gqa,
    float* __restrict__ gqb, float* __restrict__ gscale, float* __restrict__ gpre, float* __restrict__ gpost, int64_t n, int d,
    int ka, int kb, int reverse_a, int reverse_b) {
  constexpr bool kStage = kMode == 0;
  constexpr bool kRegs = kMode == 2;
  constexpr int W = 64 * E;
  extern __shared__ __attribute__((aligned(16))) float hdh_lds[];
  const int positions = ka + kb + 1;
  const int chunk = kRegs ? kHdhChunk : positions;
  float* coef = hdh_lds;
  float* acc = hdh_lds + ((ka + kb + 3) & ~3);      // [chunk + 2][W]: the chunk's positions, then gpost, then gpre
  float* qs = acc + (chunk + 2) * W;                // [ka + kb][W] (mode 0)
  const int lane = threadIdx.x & 63;
  hdh_prologue<E, kStage>(coef, qs, qa, qb, d, ka, kb, lane);
  Row<E> sc, po;
  load_row_or<E>(sc, scale, d, lane, 1.f);          // 1 in the padding lanes: the walk divides by it
  load_row_or<E>(po, post, d, lane, 0.f);
  // table index of the reflection at position p (p != ka)
  auto table = [&](int p) { return p < ka ? (reverse_a ? ka - 1 - p : p) : ka + (reverse_b ? kb - 1 - (p - ka - 1) : p - ka - 1); };
  // one position back; kAcc: add its parameter gradient into `into`
  auto step = [&](int p, Row<E>& v, Row<E>& g, auto&& into) __attribute__((always_inline)) {
    if (p == ka) {
#pragma unroll
      for (int e = 0; e < E; ++e) {
        v.v[e] = v.v[e] / sc.v[e];
        into(e, g.v[e] * v.v[e]);
        g.v[e] = g.v[e] * sc.v[e];
      }
      return;
    }
    const int k = table(p);
    Row<E> qv;
    hdh_q_row<E, kStage>(qv, qs, qa, qb, k, d, ka, lane);
    const float alpha = coef[k];
    const float a_out = dot_rows<E>(v, qv), c = dot_rows<E>(g, qv);
    const float a = -a_out;                         // (H v) . q = -(v . q)
#pragma unroll
    for (int e = 0; e < E; ++e) {
      v.v[e] -= a_out * (alpha * qv.v[e]);
      into(e, -alpha * (c * v.v[e] + a * g.v[e]) + (alpha * alpha) * (a * c) * qv.v[e]);
      g.v[e] -= c * (alpha * qv.v[e]);
    }
  };
  auto nothing = [](int, float) {};
  const int64_t stride = wave_unit_stride();
  const int64_t row0 = wave_first_unit();
  for (int hi = positions; hi > 0; hi -= chunk) {      // positions [lo, hi), the chunk nearest the output first
    const int lo = hi - chunk > 0 ? hi - chunk : 0;
    const bool first = hi == positions, last = lo == 0;
    for (int i = threadIdx.x; i < (chunk + 2) * W; i += 256) acc[i] = 0.f;
    __syncthreads();
    Row<E> racc[kRegs ? kHdhChunk : 1], gpo, gpr;
#pragma unroll
    for (int e = 0; e < E; ++e) gpo.v[e] = gpr.v[e] = 0.f;
    if constexpr (kRegs) {
#pragma unroll
      for (int k = 0; k < kHdhChunk; ++k)
#pragma unroll
        for (int e = 0; e < E; ++e) racc[k].v[e] = 0.f;
    }
    for (int64_t row = row0; row < n; row += stride) {
      Row<E> v, g;
      load_row<E>(v, y + row * d, d, lane);
      load_row<E>(g, gy + row * d, d, lane);
#pragma unroll
      for (int e = 0; e < E; ++e) {
        v.v[e] = v.v[e] - po.v[e];
        if (first) gpo.v[e] += g.v[e];
      }
      for (int p = positions - 1; p >= hi; --p) step(p, v, g, nothing);      // the positions after this chunk: undo only
      if constexpr (kRegs) {
#pragma unroll
        for (int k = kHdhChunk - 1; k >= 0; --k) {
          const int p = lo + k;
          if (p < hi) step(p, v, g, [&](int e, float t) { racc[k].v[e] += t; });
        }
      } else {
        for (int p = hi - 1; p >= lo; --p)
          step(p, v, g, [&](int e, float t) { atomicAdd(acc + (p - lo) * W + lane + 64 * e, t); });
      }
      if (last) {
        store_row<E>(g, gx + row * d, d, lane);
#pragma unroll
        for (int e = 0; e < E; ++e) gpr.v[e] -= g.v[e];
      }
    }
    // the waves' register sums meet in LDS
    if constexpr (kRegs) {
#pragma unroll
      for (int k = 0; k < kHdhChunk; ++k)
        if (lo + k < hi) {
#pragma unroll
          for (int e = 0; e < E; ++e) atomicAdd(acc + k * W + lane + 64 * e, racc[k].v[e]);
        }
    }
#pragma unroll
    for (int e = 0; e < E; ++e) {
      if (first) atomicAdd(acc + chunk * W + lane + 64 * e, gpo.v[e]);
      if (last) atomicAdd(acc + (chunk + 1) * W + lane + 64 * e, gpr.v[e]);
    }
    __syncthreads();
    // one global atomic per element and workgroup
    for (int i = threadIdx.x; i < (hi - lo) * W; i += 256) {
      const int p = lo + i / W, col = i % W;
      if (col < d) {
        float* dst = p == ka ? gscale + col : p < ka ? gqa + (int64_t)table(p) * d + col : gqb + (int64_t)(table(p) - ka) * d + col;
        atomicAdd(dst, acc[i]);
      }
    }
    for (int col = threadIdx.x; col < d; col += 256) {
      if (first && gpost) atomicAdd(gpost + col, acc[chunk * W + col]);
      if (last && gpre) atomicAdd(gpre + col, acc[(chunk + 1) * W + col]);
    }
    __syncthreads();      // the next pass zeroes the rows
  }
}

}  // namespace fc

extern "C" int fc_hdh_linear(const float* x, float* y, const float* q_a, const float* q_b, const float* scale,
                             const float* pre, const float* post, int64_t n, int32_t d, int32_t ka, int32_t kb,
                             int32_t reverse_a, int32_t reverse_b, void* stream) {
  if (n < 0 || d <= 0 || d > fc::kMaxRowFeatures || ka < 0 || kb < 0 || ka + kb > fc::kHdhMaxReflections)
    return hipErrorInvalidValue;
  if (n == 0) return hipSuccess;
  if (!x || !y || !scale || (!q_a && ka > 0) || (!q_b && kb > 0)) return hipErrorInvalidValue;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int w = 64 * fc::elems_for(d), table = (ka + kb + 3) & ~3;
  const size_t staged = sizeof(float) * ((size_t)table + (size_t)(ka + kb) * w);
  const bool stage = staged <= (size_t)fc::kHdhLdsBudget;
  const size_t lds = stage ? staged : sizeof(float) * table;
  // two rows per wave where the registers are few (E <= 2)
#define FC_HDH_FWD(RV, STAGE)                                                                                            \
  hipLaunchKernelGGL((fc::hdh_linear_kernel<E, RV, STAGE>), dim3(fc::row_grid((n + RV - 1) / RV, fc::kStreamGridCap)),    \
                     dim3(256), lds, s, x, y, q_a, q_b, scale, pre, post, n, d, ka, kb, reverse_a, reverse_b)
  FC_ROW_DISPATCH(d, {
    constexpr int RV = E <= 2 ? 2 : 1;
    if (stage) FC_HDH_FWD(RV, true);
    else FC_HDH_FWD(RV, false);
  });
#undef FC_HDH_FWD
  return hipGetLastError();
}

extern "C" int fc_hdh_linear_backward(const float* y, const float* grad_y, const float* q_a, const float* q_b,
                                      const float* scale, const float* post, float* grad_x, float* grad_q_a,
                                      float* grad_q_b, float* grad_scale, float* grad_pre, float* grad_post, int64_t n,
                                      int32_t d, int32_t ka, int32_t kb, int32_t reverse_a, int32_t reverse_b,
                                      void* stream) {
  if (n < 0 || d <= 0 || d > fc::kMaxRowFeatures || ka < 0 || kb < 0 || ka + kb > fc::kHdhMaxReflections)
    return hipErrorInvalidValue;
  if (n == 0) return hipSuccess;
  if (!y || !grad_y || !scale || !grad_x || !grad_scale || (ka > 0 && (!q_a || !grad_q_a)) || (kb > 0 && (!q_b || !grad_q_b)))
    return hipErrorInvalidValue;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int w = 64 * fc::elems_for(d), table = (ka + kb + 3) & ~3;
  const size_t rows_all = sizeof(float) * ((size_t)table + (size_t)(ka + kb + 3) * w);      // every position + gpost + gpre
  const size_t rows_staged = rows_all + sizeof(float) * (size_t)(ka + kb) * w;
  const size_t rows_chunk = sizeof(float) * ((size_t)table + (size_t)(fc::kHdhChunk + 2) * w);
  const int mode = rows_staged <= (size_t)fc::kHdhLdsBudget ? 0 : rows_all <= (size_t)fc::kHdhLdsBudget ? 1 : 2;
  const size_t lds = mode == 0 ? rows_staged : mode == 1 ? rows_all : rows_chunk;
#define FC_HDH_BWD(MODE)                                                                                                  \
  hipLaunchKernelGGL((fc::hdh_linear_backward_kernel<E, MODE>), dim3(fc::row_grid(n, fc::kReduceGridCap)), dim3(256), lds, \
                     s, y, grad_y, q_a, q_b, scale, post, grad_x, grad_q_a, grad_q_b, grad_scale, grad_pre, grad_post, n, \
                     d, ka, kb, reverse_a, reverse_b)
  FC_ROW_DISPATCH(d, {
    if (mode == 0) FC_HDH_BWD(0);
    else if (mode == 1) FC_HDH_BWD(1);
    else FC_HDH_BWD(2);
  });
#undef FC_HDH_BWD
  return hipGetLastError();
}
