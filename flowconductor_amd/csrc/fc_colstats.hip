// Batch-axis (column) reductions over [N, D] row-major float32 rows, 2 <= N, 1 <= D <= 512, gfx950: the batch moments of
// BatchNorm in training mode (flowcon/transforms/normalization.py:98-141) with its normalise pass and backward, and the
// column sums behind the scale / shift gradients of ActNorm and PointwiseAffineTransform.
//
// Every reduction has two stages (the scheme of fc_deep_sigmoid_backward.hip's batch-shared row).  Stage 1: workgroup b of
// `partials(N, D)` <= kColMaxPartials reduces rows [b rpb, min(N, (b + 1) rpb)), rpb = ceil(N / partials), to one row of
// the partial buffer.  Stage 2: one workgroup merges the partial rows.  No atomics: the order of every floating-point
// operation is a function of (N, D) alone, so two calls give the same bits.
//
// Thread layout of the [N, D] passes.  A lane owns V consecutive columns (V = 4 and 16-byte accesses where D % 4 == 0 and
// the tensors are 16-byte aligned, V = 1 otherwise), `cl` = min(64, D / V) lanes side by side cover a row segment and
// `rl` = 256 / cl such segments stack to a workgroup.  A lane's columns stay fixed while it walks down the rows, so the
// accumulators and the per-column constants live in registers; consecutive lanes read consecutive addresses (D <= 256: whole
// rows, one after the other).  Wider rows take gridDim.y column tiles of 64 lanes.
//
// Moments never come from sum x^2: a lane takes kColUnroll rows at a time (independent loads in flight), forms their mean
// and their sum of squared deviations from that mean, and merges the group into its running (count, mean, M2) with Chan's
// pairwise formula; lanes, workgroups and partial rows merge the same way.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/flowcon_hip.h"

namespace fc {

constexpr int kColMaxPartials = FC_COLSTATS_MAX_PARTIALS;   // rows of the partial buffer: fixed, so the merge order is too
constexpr int kColUnroll = 8;                                // rows a lane loads before it touches its accumulators
constexpr int kColThreads = 256;
constexpr int kColFinishThreads = 512;
static_assert(kColThreads * kColUnroll == FC_COLSTATS_ROWS_PER_ITERATION, "header constant out of step");
static_assert(kColFinishThreads >= FC_COLSTATS_MAX_FEATURES && kColFinishThreads >= kColMaxPartials, "finish: one thread each");

struct ColShape {
  int64_t n;
  int d;
  int vec;          // 4 or 1
  int cl, rl;       // lanes across a row segment, segments per workgroup (cl * rl <= 256)
  int tiles;        // column tiles (gridDim.y)
  int partials;     // stage-1 workgroups along the batch
  int64_t rpb;      // rows per stage-1 workgroup
};

inline ColShape col_shape(int64_t n, int d, bool vec4) {
  ColShape s;
  s.n = n;
  s.d = d;
  s.vec = vec4 ? 4 : 1;
  const int lanes = d / s.vec;
  s.cl = lanes < 64 ? lanes : 64;
  s.rl = kColThreads / s.cl;
  s.tiles = (lanes + s.cl - 1) / s.cl;
  const int64_t groups = (n + s.rl - 1) / s.rl;
  s.partials = (int)(groups < kColMaxPartials ? groups : kColMaxPartials);
  s.rpb = (n + s.partials - 1) / s.partials;
  return s;
}

template <int V>
__device__ __forceinline__ void load_cols(const float* p, float (&v)[V]) {
  if constexpr (V == 4) {
    const float4 q = *reinterpret_cast<const float4*>(p);
    v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
  } else {
    v[0] = *p;
  }
}

template <int V>
__device__ __forceinline__ void store_cols(float* p, const float (&v)[V]) {
  if constexpr (V == 4) {
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
    *p = v[0];
  }
}

// (na, ma, qa) <- (na, ma, qa) merged with (nb, mb, qb); nb == 0 changes nothing (Chan et al.)
template <class T>
__device__ __forceinline__ void chan_merge(T& na, T& ma, T& qa, T nb, T mb, T qb) {
  if (nb > T(0)) {
    const T nn = na + nb;
    const T f = nb / nn;
    const T delta = mb - ma;
    ma += delta * f;
    qa += qb + delta * delta * (na * f);
    na = nn;
  }
}

// ---- stage 1: moments -------------------------------------------------------------------------------------------------
// partial[(2 b) D + j] = mean, partial[(2 b + 1) D + j] = M2 of column j over workgroup b's rows (its count follows from
// the slice bounds; an empty slice leaves zeros that the finish kernel never reads).
template <int V>
__global__ __launch_bounds__(kColThreads) void col_moments_partial_kernel(const float* __restrict__ x,
                                                                          float* __restrict__ partial, ColShape s) {
  __shared__ float sm_n[kColThreads];
  __shared__ float sm_mean[V][kColThreads];
  __shared__ float sm_m2[V][kColThreads];
  const int tid = threadIdx.x;
  const int c = tid % s.cl, r = tid / s.cl;
  const int col0 = (blockIdx.y * s.cl + c) * V;
  const bool live = r < s.rl && col0 < s.d;
  const int64_t begin = (int64_t)blockIdx.x * s.rpb;
  int64_t end = begin + s.rpb;
  if (end > s.n) end = s.n;
  float n = 0.f, mean[V], m2[V];
#pragma unroll
  for (int k = 0; k < V; ++k) mean[k] = 0.f, m2[k] = 0.f;
  if (live) {
    const int64_t step = (int64_t)s.rl * kColUnroll;
    for (int64_t row = begin + r; row < end; row += step) {
      float v[kColUnroll][V];
      int cnt = 0;
#pragma unroll
      for (int u = 0; u < kColUnroll; ++u) {
        const int64_t rr = row + (int64_t)u * s.rl;
        if (rr < end) {
          load_cols<V>(x + rr * s.d + col0, v[u]);
          ++cnt;
        } else {
#pragma unroll
          for (int k = 0; k < V; ++k) v[u][k] = 0.f;
        }
      }
      const float fc = (float)cnt;
      const float inv = cnt == kColUnroll ? 1.f / kColUnroll : 1.f / fc;
      const float nn = n + fc;
      const float f = fc / nn;
#pragma unroll
      for (int k = 0; k < V; ++k) {
        float sum = 0.f;
#pragma unroll
        for (int u = 0; u < kColUnroll; ++u) sum += v[u][k];   // (rows past the slice hold zeros)
        const float cm = sum * inv;
        float q = 0.f;
#pragma unroll
        for (int u = 0; u < kColUnroll; ++u) {
          const float dv = u < cnt ? v[u][k] - cm : 0.f;
          q += dv * dv;
        }
        const float delta = cm - mean[k];
        mean[k] += delta * f;
        m2[k] += q + delta * delta * (n * f);
      }
      n = nn;
    }
  }
  // lanes that share a column: a pairwise tree over the segment index r, through LDS
  sm_n[tid] = n;
#pragma unroll
  for (int k = 0; k < V; ++k) sm_mean[k][tid] = mean[k], sm_m2[k][tid] = m2[k];
  int top = 1;
  while (top < s.rl) top <<= 1;
  for (int half = top >> 1; half >= 1; half >>= 1) {
    __syncthreads();
    const bool take = r < half && r + half < s.rl;
    const int other = take ? tid + half * s.cl : tid;
    const float nb = sm_n[other];
    float mb[V], qb[V];
#pragma unroll
    for (int k = 0; k < V; ++k) mb[k] = sm_mean[k][other], qb[k] = sm_m2[k][other];
    __syncthreads();
    if (take) {
      float nk = n;
#pragma unroll
      for (int k = 0; k < V; ++k) {
        nk = n;
        chan_merge(nk, mean[k], m2[k], nb, mb[k], qb[k]);
        sm_mean[k][tid] = mean[k], sm_m2[k][tid] = m2[k];
      }
      n = nk;
      sm_n[tid] = n;
    }
  }
  if (r == 0 && col0 < s.d) {
    float* row = partial + (size_t)blockIdx.x * 2 * s.d;
    store_cols<V>(row + col0, mean);
    store_cols<V>(row + s.d + col0, m2);
  }
}

// A fixed tree over the workgroup's kColFinishThreads values; every thread gets the total.
__device__ __forceinline__ double finish_block_sum(double v, double* sm) {
  const int tid = threadIdx.x;
  __syncthreads();
  sm[tid] = v;
  for (int half = kColFinishThreads >> 1; half >= 1; half >>= 1) {
    __syncthreads();
    if (tid < half) sm[tid] += sm[tid + half];
  }
  __syncthreads();
  return sm[0];
}

struct ColMomentsOut {
  float* mean;           // [D]
  float* var;            // [D] unbiased
  float* invstd;         // [D] 1 / sqrt(var + eps)
  float* half_log_sum;   // [1] sum_j -0.5 log(var_j + eps)
  float* running_mean;   // [D] or null: += momentum (mean - running_mean)
  float* running_var;    // [D] or null
  float eps, momentum;
};

// ---- stage 2: moments -------------------------------------------------------------------------------------------------
// One workgroup.  Thread (g, j) = (tid / D, tid % D) merges the partial rows g per .. (g + 1) per of column j in index
// order, the groups then merge pairwise; float64 throughout (a few thousand operations).
__global__ __launch_bounds__(kColFinishThreads) void col_moments_finish_kernel(const float* __restrict__ partial, ColShape s,
                                                                               ColMomentsOut o) {
  __shared__ double sm[3][kColFinishThreads];
  const int tid = threadIdx.x, d = s.d;
  const int groups = kColFinishThreads / d;              // d <= 512: at least one
  const int per = (s.partials + groups - 1) / groups;
  const int j = tid % d, g = tid / d;
  double n = 0., mean = 0., m2 = 0.;
  if (g < groups) {
    const int last = (g + 1) * per < s.partials ? (g + 1) * per : s.partials;
    for (int b = g * per; b < last; ++b) {
      int64_t cnt = s.n - (int64_t)b * s.rpb;
      if (cnt > s.rpb) cnt = s.rpb;
      if (cnt <= 0) continue;                            // an empty slice merges as count 0
      const float* row = partial + (size_t)b * 2 * d;
      chan_merge(n, mean, m2, (double)cnt, (double)row[j], (double)row[d + j]);
    }
  }
  sm[0][tid] = n, sm[1][tid] = mean, sm[2][tid] = m2;
  int top = 1;
  while (top < groups) top <<= 1;
  for (int half = top >> 1; half >= 1; half >>= 1) {
    __syncthreads();
    if (g < half && g + half < groups) {
      const int other = tid + half * d;
      chan_merge(n, mean, m2, sm[0][other], sm[1][other], sm[2][other]);
      sm[0][tid] = n, sm[1][tid] = mean, sm[2][tid] = m2;
    }
  }
  double half_log = 0.;
  if (tid < d) {
    const float meanf = (float)mean;
    const float varf = (float)(m2 / (double)(s.n - 1));
    const float ve = varf + o.eps;                       // float32, as the reference's var + eps
    o.mean[tid] = meanf;
    o.var[tid] = varf;
    o.invstd[tid] = 1.f / sqrtf(ve);
    half_log = -0.5 * (double)logf(ve);
    if (o.running_mean) o.running_mean[tid] += o.momentum * (meanf - o.running_mean[tid]);
    if (o.running_var) o.running_var[tid] += o.momentum * (varf - o.running_var[tid]);
  }
  const double total = finish_block_sum(half_log, &sm[0][0]);
  if (tid == 0) *o.half_log_sum = (float)total;
}

// ---- normalise: y = w ((x - mean) invstd) + b ---------------------------------------------------------------------------
constexpr int kColApplyUnroll = 4;

template <int V>
__global__ __launch_bounds__(kColThreads) void bn_apply_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                               const float* __restrict__ mean,
                                                               const float* __restrict__ invstd,
                                                               const float* __restrict__ weight,
                                                               const float* __restrict__ bias, ColShape s) {
  const int tid = threadIdx.x;
  const int c = tid % s.cl, r = tid / s.cl;
  const int col0 = (blockIdx.y * s.cl + c) * V;
  if (r >= s.rl || col0 >= s.d) return;
  float m[V], is[V], w[V], b[V];
  load_cols<V>(mean + col0, m);
  load_cols<V>(invstd + col0, is);
  load_cols<V>(weight + col0, w);
  load_cols<V>(bias + col0, b);
  const int64_t stride = (int64_t)gridDim.x * s.rl;
  for (int64_t row = (int64_t)blockIdx.x * s.rl + r; row < s.n; row += stride * kColApplyUnroll) {
    float v[kColApplyUnroll][V];
#pragma unroll
    for (int u = 0; u < kColApplyUnroll; ++u) {
      const int64_t rr = row + u * stride;
      if (rr < s.n) load_cols<V>(x + rr * s.d + col0, v[u]);
    }
#pragma unroll
    for (int u = 0; u < kColApplyUnroll; ++u) {
      const int64_t rr = row + u * stride;
      if (rr < s.n) {
#pragma unroll
        for (int k = 0; k < V; ++k) v[u][k] = w[k] * ((v[u][k] - m[k]) * is[k]) + b[k];
        store_cols<V>(y + rr * s.d + col0, v[u]);
      }
    }
  }
}

// ---- stage 1: column sums -----------------------------------------------------------------------------------------------
// partial[(2 b) D + j] = sum g, partial[(2 b + 1) D + j] = sum g vh over workgroup b's rows, vh = (v - mean) invstd (or v
// itself when mean is null); gl_partial[b] = sum of gl over the same rows (column tile 0 only, when gl is given).
template <int V>
__global__ __launch_bounds__(kColThreads) void col_sums_partial_kernel(const float* __restrict__ g,
                                                                       const float* __restrict__ v,
                                                                       const float* __restrict__ mean,
                                                                       const float* __restrict__ invstd,
                                                                       const float* __restrict__ gl,
                                                                       float* __restrict__ partial,
                                                                       float* __restrict__ gl_partial, ColShape s) {
  __shared__ float sm1[V][kColThreads];
  __shared__ float sm2[V][kColThreads];
  const int tid = threadIdx.x;
  const int c = tid % s.cl, r = tid / s.cl;
  const int col0 = (blockIdx.y * s.cl + c) * V;
  const bool live = r < s.rl && col0 < s.d;
  const int64_t begin = (int64_t)blockIdx.x * s.rpb;
  int64_t end = begin + s.rpb;
  if (end > s.n) end = s.n;
  float s1[V], s2[V], m[V], is[V];
#pragma unroll
  for (int k = 0; k < V; ++k) s1[k] = 0.f, s2[k] = 0.f, m[k] = 0.f, is[k] = 1.f;
  if (live) {
    if (mean) {
      load_cols<V>(mean + col0, m);
      load_cols<V>(invstd + col0, is);
    }
    const int64_t step = (int64_t)s.rl * kColUnroll;
    for (int64_t row = begin + r; row < end; row += step) {
      float gv[kColUnroll][V], vv[kColUnroll][V];
#pragma unroll
      for (int u = 0; u < kColUnroll; ++u) {
        const int64_t rr = row + (int64_t)u * s.rl;
        if (rr < end) {
          load_cols<V>(g + rr * s.d + col0, gv[u]);
          load_cols<V>(v + rr * s.d + col0, vv[u]);
        } else {
#pragma unroll
          for (int k = 0; k < V; ++k) gv[u][k] = 0.f, vv[u][k] = 0.f;
        }
      }
#pragma unroll
      for (int k = 0; k < V; ++k) {
        float a1 = 0.f, a2 = 0.f;
#pragma unroll
        for (int u = 0; u < kColUnroll; ++u) {
          const bool valid = row + (int64_t)u * s.rl < end;
          const float term = gv[u][k] * (mean ? (vv[u][k] - m[k]) * is[k] : vv[u][k]);
          a1 += gv[u][k];                                       // (rows past the slice hold zeros)
          a2 += valid ? term : 0.f;
        }
        s1[k] += a1;
        s2[k] += a2;
      }
    }
  }
#pragma unroll
  for (int k = 0; k < V; ++k) sm1[k][tid] = s1[k], sm2[k][tid] = s2[k];
  int top = 1;
  while (top < s.rl) top <<= 1;
  for (int half = top >> 1; half >= 1; half >>= 1) {
    __syncthreads();
    if (r < half && r + half < s.rl) {
      const int other = tid + half * s.cl;
#pragma unroll
      for (int k = 0; k < V; ++k) {
        s1[k] += sm1[k][other];
        s2[k] += sm2[k][other];
        sm1[k][tid] = s1[k], sm2[k][tid] = s2[k];
      }
    }
  }
  if (r == 0 && col0 < s.d) {
    float* row = partial + (size_t)blockIdx.x * 2 * s.d;
    store_cols<V>(row + col0, s1);
    store_cols<V>(row + s.d + col0, s2);
  }
  if (gl && blockIdx.y == 0) {
    float a = 0.f;
    for (int64_t row = begin + tid; row < end; row += kColThreads) a += gl[row];
    __syncthreads();
    sm1[0][tid] = a;
    for (int half = kColThreads >> 1; half >= 1; half >>= 1) {
      __syncthreads();
      if (tid < half) sm1[0][tid] += sm1[0][tid + half];
    }
    if (tid == 0) gl_partial[blockIdx.x] = sm1[0][0];
  }
}

// ---- stage 2: column sums -----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kColFinishThreads) void col_sums_finish_kernel(const float* __restrict__ partial,
                                                                            const float* __restrict__ gl_partial, ColShape s,
                                                                            float* __restrict__ s1, float* __restrict__ s2,
                                                                            float* __restrict__ gl_sum) {
  __shared__ double sm[2][kColFinishThreads];
  const int tid = threadIdx.x, d = s.d;
  const int groups = kColFinishThreads / d;
  const int per = (s.partials + groups - 1) / groups;
  const int j = tid % d, g = tid / d;
  double a1 = 0., a2 = 0.;
  if (g < groups) {
    const int last = (g + 1) * per < s.partials ? (g + 1) * per : s.partials;
    for (int b = g * per; b < last; ++b) {
      const float* row = partial + (size_t)b * 2 * d;
      a1 += (double)row[j];
      a2 += (double)row[d + j];
    }
  }
  sm[0][tid] = a1, sm[1][tid] = a2;
  int top = 1;
  while (top < groups) top <<= 1;
  for (int half = top >> 1; half >= 1; half >>= 1) {
    __syncthreads();
    if (g < half && g + half < groups) {
      const int other = tid + half * d;
      a1 += sm[0][other];
      a2 += sm[1][other];
      sm[0][tid] = a1, sm[1][tid] = a2;
    }
  }
  if (tid < d) {
    s1[tid] = (float)a1;
    s2[tid] = (float)a2;
  }
  if (gl_sum) {                                               // (uniform over the workgroup)
    const double total = finish_block_sum(tid < s.partials ? (double)gl_partial[tid] : 0., &sm[0][0]);
    if (tid == 0) *gl_sum = (float)total;
  }
}

// ---- BatchNorm backward, point-wise part ------------------------------------------------------------------------------
// gx = w invstd (gy - s1 / N - xh s2 / (N - 1)) - GL invstd xh / (N - 1),  xh = (x - mean) invstd
template <int V>
__global__ __launch_bounds__(kColThreads) void bn_backward_apply_kernel(const float* __restrict__ x,
                                                                        const float* __restrict__ gy, float* __restrict__ gx,
                                                                        const float* __restrict__ mean,
                                                                        const float* __restrict__ invstd,
                                                                        const float* __restrict__ weight,
                                                                        const float* __restrict__ s1,
                                                                        const float* __restrict__ s2,
                                                                        const float* __restrict__ gl_sum, ColShape s) {
  const int tid = threadIdx.x;
  const int c = tid % s.cl, r = tid / s.cl;
  const int col0 = (blockIdx.y * s.cl + c) * V;
  if (r >= s.rl || col0 >= s.d) return;
  float m[V], is[V], a[V], c1[V], c2[V], c3[V];
  load_cols<V>(mean + col0, m);
  load_cols<V>(invstd + col0, is);
  load_cols<V>(weight + col0, a);
  load_cols<V>(s1 + col0, c1);
  load_cols<V>(s2 + col0, c2);
  const float nf = (float)s.n, n1 = (float)(s.n - 1);
  const float glt = gl_sum ? *gl_sum : 0.f;
#pragma unroll
  for (int k = 0; k < V; ++k) {
    a[k] *= is[k];
    c1[k] /= nf;
    c2[k] /= n1;
    c3[k] = glt * is[k] / n1;
  }
  const int64_t stride = (int64_t)gridDim.x * s.rl;
  for (int64_t row = (int64_t)blockIdx.x * s.rl + r; row < s.n; row += stride * kColApplyUnroll) {
    float xv[kColApplyUnroll][V], gv[kColApplyUnroll][V];
#pragma unroll
    for (int u = 0; u < kColApplyUnroll; ++u) {
      const int64_t rr = row + u * stride;
      if (rr < s.n) {
        load_cols<V>(x + rr * s.d + col0, xv[u]);
        load_cols<V>(gy + rr * s.d + col0, gv[u]);
      }
    }
#pragma unroll
    for (int u = 0; u < kColApplyUnroll; ++u) {
      const int64_t rr = row + u * stride;
      if (rr < s.n) {
#pragma unroll
        for (int k = 0; k < V; ++k) {
          const float xh = (xv[u][k] - m[k]) * is[k];
          gv[u][k] = a[k] * (gv[u][k] - c1[k] - xh * c2[k]) - c3[k] * xh;
        }
        store_cols<V>(gx + rr * s.d + col0, gv[u]);
      }
    }
  }
}

inline bool col_aligned16(const void* a, const void* b = nullptr, const void* c = nullptr) {
  return ((((uintptr_t)a) | ((uintptr_t)b) | ((uintptr_t)c)) & 15u) == 0;
}

inline bool col_shape_ok(int64_t n, int32_t d) { return n >= 2 && d >= 1 && d <= FC_COLSTATS_MAX_FEATURES; }

inline unsigned col_apply_grid(const ColShape& s) {
  int64_t grid = (s.n + s.rl - 1) / s.rl;
  const int64_t cap = 2048 / s.tiles;
  return (unsigned)(grid < cap ? grid : cap);
}

inline hipError_t col_sums_launch(const float* g, const float* v, const float* mean, const float* invstd, const float* gl,
                                  float* s1, float* s2, float* gl_sum, float* workspace, const ColShape& s, hipStream_t st) {
  float* gl_partial = workspace + (size_t)kColMaxPartials * 2 * s.d;
  const dim3 grid((unsigned)s.partials, (unsigned)s.tiles);
  if (s.vec == 4)
    hipLaunchKernelGGL(col_sums_partial_kernel<4>, grid, dim3(kColThreads), 0, st, g, v, mean, invstd, gl, workspace,
                       gl_partial, s);
  else
    hipLaunchKernelGGL(col_sums_partial_kernel<1>, grid, dim3(kColThreads), 0, st, g, v, mean, invstd, gl, workspace,
                       gl_partial, s);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(col_sums_finish_kernel, dim3(1), dim3(kColFinishThreads), 0, st, workspace, gl_partial, s, s1, s2,
                     gl ? gl_sum : nullptr);
  return hipGetLastError();
}

}  // namespace fc

extern "C" int fc_colstats_workspace(int32_t d) {
  if (d < 1 || d > FC_COLSTATS_MAX_FEATURES) return 0;
  return fc::kColMaxPartials * (2 * d + 1);
}

extern "C" int fc_batchnorm_train(const float* x, const float* weight, const float* bias, float* y, float* mean, float* var,
                                  float* invstd, float* half_log_sum, float* running_mean, float* running_var,
                                  float* workspace, int64_t n, int32_t d, float eps, float momentum, void* stream) {
  if (!fc::col_shape_ok(n, d)) return hipErrorInvalidValue;
  if (!x || !weight || !bias || !y || !mean || !var || !invstd || !half_log_sum || !workspace) return hipErrorInvalidValue;
  if ((running_mean == nullptr) != (running_var == nullptr)) return hipErrorInvalidValue;
  const bool vec4 = d % 4 == 0 && fc::col_aligned16(x, y) && fc::col_aligned16(mean, invstd) && fc::col_aligned16(weight, bias) &&
                    fc::col_aligned16(workspace);
  const fc::ColShape s = fc::col_shape(n, d, vec4);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)s.partials, (unsigned)s.tiles);
  if (vec4)
    hipLaunchKernelGGL(fc::col_moments_partial_kernel<4>, grid, dim3(fc::kColThreads), 0, st, x, workspace, s);
  else
    hipLaunchKernelGGL(fc::col_moments_partial_kernel<1>, grid, dim3(fc::kColThreads), 0, st, x, workspace, s);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const fc::ColMomentsOut o{mean, var, invstd, half_log_sum, running_mean, running_var, eps, momentum};
  hipLaunchKernelGGL(fc::col_moments_finish_kernel, dim3(1), dim3(fc::kColFinishThreads), 0, st, workspace, s, o);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  const dim3 agrid(fc::col_apply_grid(s), (unsigned)s.tiles);
  if (vec4)
    hipLaunchKernelGGL(fc::bn_apply_kernel<4>, agrid, dim3(fc::kColThreads), 0, st, x, y, mean, invstd, weight, bias, s);
  else
    hipLaunchKernelGGL(fc::bn_apply_kernel<1>, agrid, dim3(fc::kColThreads), 0, st, x, y, mean, invstd, weight, bias, s);
  return hipGetLastError();
}

extern "C" int fc_column_sums(const float* g, const float* v, const float* mean, const float* invstd, const float* gl,
                              float* s1, float* s2, float* gl_sum, float* workspace, int64_t n, int32_t d, void* stream) {
  if (!fc::col_shape_ok(n, d)) return hipErrorInvalidValue;
  if (!g || !v || !s1 || !s2 || !workspace) return hipErrorInvalidValue;
  if ((mean == nullptr) != (invstd == nullptr) || (gl && !gl_sum)) return hipErrorInvalidValue;
  const bool vec4 = d % 4 == 0 && fc::col_aligned16(g, v) && fc::col_aligned16(mean, invstd) && fc::col_aligned16(workspace);
  return fc::col_sums_launch(g, v, mean, invstd, gl, s1, s2, gl_sum, workspace, fc::col_shape(n, d, vec4),
                             static_cast<hipStream_t>(stream));
}

extern "C" int fc_batchnorm_train_backward(const float* x, const float* grad_y, const float* grad_logabsdet,
                                           const float* mean, const float* invstd, const float* weight, float* grad_x,
                                           float* s1, float* s2, float* gl_sum, float* workspace, int64_t n, int32_t d,
                                           void* stream) {
  if (!fc::col_shape_ok(n, d)) return hipErrorInvalidValue;
  if (!x || !grad_y || !mean || !invstd || !weight || !s1 || !s2 || !workspace) return hipErrorInvalidValue;
  if (grad_logabsdet && !gl_sum) return hipErrorInvalidValue;
  const bool vec4 = d % 4 == 0 && fc::col_aligned16(x, grad_y, grad_x) && fc::col_aligned16(mean, invstd, weight) &&
                    fc::col_aligned16(s1, s2, workspace);
  const fc::ColShape s = fc::col_shape(n, d, vec4);
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipError_t e = fc::col_sums_launch(grad_y, x, mean, invstd, grad_logabsdet, s1, s2, gl_sum, workspace, s, st);
  if (e != hipSuccess || !grad_x) return e;
  const dim3 agrid(fc::col_apply_grid(s), (unsigned)s.tiles);
  const float* glt = grad_logabsdet ? gl_sum : nullptr;
  if (vec4)
    hipLaunchKernelGGL(fc::bn_backward_apply_kernel<4>, agrid, dim3(fc::kColThreads), 0, st, x, grad_y, grad_x, mean, invstd,
                       weight, s1, s2, glt, s);
  else
    hipLaunchKernelGGL(fc::bn_backward_apply_kernel<1>, agrid, dim3(fc::kColThreads), 0, st, x, grad_y, grad_x, mean, invstd,
                       weight, s1, s2, glt, s);
  return hipGetLastError();
}
