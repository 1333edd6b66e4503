// Invertible residual blocks over Lipschitz-constrained DenseNets in eval mode (reference
// flowcon/transforms/lipschitz/iresblock.py with flowcon/nn/nets/invertible_densenet.py, lipschitz_dense.py).
//
//   fc_iresnet_forward   y = x + s g(x),  logabsdet = log|det(I + s dg/dx)|      one launch
//   fc_iresnet_inverse   x with x + s g(x) = y by the fixed-point iteration x <- y - s g(x), every row to its own
//                        convergence                                             one launch
//
// g is a DenseNet: `depth` layers  h <- cat(eta1 h, eta2 act(W h + b))  (act may itself concatenate act(t), act(-t))
// followed by one linear layer back to d outputs.  The host hands over an IMAGE of the net with the spectral
// normalisation already applied (what the eval-mode parametrisation returns), all of it float32:
//   [p0, p1, 0, 0]                                  activation scalars
//   per dense layer: [eta1, eta2, 0, 0] bias[op] wt[w_in][op]     op = out_ch rounded up to 4, wt[k][o] = W[o][k]
//   final layer:     bias[dp] wt[wtot][dp]                        dp = d rounded up to 4
// (padding entries are zero, every piece starts on a 16-byte boundary).  A block copies the image into LDS once and
// then walks over row tiles.
//
// Forward: the exact Jacobian of g is a forward-mode computation of the same shape as g.  A row is carried by a group
// of G lanes (the smallest power of two >= d + 1): lane 0 of the group runs the value stream, lane j + 1 the tangent
// d/dx_j.  Every stream keeps its growing activation vector in LDS as st[k][thread] (conflict-free, never copied: the
// concatenation is an offset), runs the same fma chain over the same float32 weights (a broadcast 16-byte LDS read per
// 4 outputs; the sums are accumulated in float64 and rounded to float32 once, so a layer's output carries one
// rounding where a float32 GEMM carries one per term), and the tangent streams pick the value stream's
// pre-activation up with a shuffle inside the group for the activation's derivative (evaluated in float64 as well).
// The final layer leaves column j of J in the registers of lane j + 1; I + s J is factorised in place, in float64, by
// LU with partial pivoting on a compile-time size (the pivot column's lane finds the pivot row and hands the
// multipliers round), logabsdet = sum log|u_ii|, rounded to float32 at the end.  A zero pivot gives
// -inf like slogdet, never NaN.
//
// Inverse: one lane per row, value stream only, the same LDS layout.  A row stops when |x - x_prev| <= atol + rtol |y|
// holds for all its elements (no square: stricter than the reference's batch-wide squared test) or after
// max_iterations; lanes that are done idle until their wave's slowest row is.  The largest iteration count of the
// launch is max-reduced into a device word for tools and tests; nothing is read back on the normal path.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/flowcon_hip.h"
#include "fc_device.h"

namespace fc {

struct IresShape {
  int d, e, depth, growth, out_ch, concat, act, wtot;
};

__host__ __device__ inline int ires_pad4(int v) { return (v + 3) & ~3; }

__host__ __device__ inline int ires_image_floats(const IresShape& sh) {
  int total = 4, w_in = sh.d + sh.e;
  const int op = ires_pad4(sh.out_ch);
  for (int l = 0; l < sh.depth; ++l) {
    total += 4 + op + w_in * op;
    w_in += sh.growth;
  }
  const int dp = ires_pad4(sh.d);
  return total + dp + w_in * dp;
}

// value f(t) and derivative f'(t) of the element-wise part of the activation (for the concatenating ones the caller
// evaluates at t and at -t).  Evaluated in float64 on the float64 pre-activation: the value a stream stores is rounded
// to float32 once, after the concatenation weight.
__device__ __forceinline__ void ires_act(int act, double t, double p0, double p1, double& f, double& df) {
  switch (act) {
    case FC_IRES_ACT_RELU:
      f = t > 0.0 ? t : 0.0;
      df = t > 0.0 ? 1.0 : 0.0;
      break;
    case FC_IRES_ACT_TANH: {
      const double th = tanh(t);
      f = th;
      df = 1.0 - th * th;
      break;
    }
    case FC_IRES_ACT_ELU: {
      f = t > 0.0 ? t : p0 * expm1(t);
      df = t > 0.0 ? 1.0 : p0 * exp(t);
      break;
    }
    case FC_IRES_ACT_SIN:
    case FC_IRES_ACT_CSIN: {
      const double a = p0 * t;
      const double div = act == FC_IRES_ACT_CSIN ? 1.41421356237309504880 : 1.0;
      f = sin(a) / (p0 * div);
      df = cos(a) / div;
      break;
    }
    default: {  // the Swish family: t sigmoid(b t) / 1.1 (/ 1.004 for LipSwish, CLipSwish), LeakyLSwish mixes with t
      const double sg = 1.0 / (1.0 + exp(-p0 * t));
      double v = t * sg / 1.1;
      double dv = (sg + p0 * t * sg * (1.0 - sg)) / 1.1;
      if (act == FC_IRES_ACT_LIPSWISH || act == FC_IRES_ACT_CLIPSWISH) {
        v = v / 1.004;
        dv = dv / 1.004;
      } else if (act == FC_IRES_ACT_LEAKY_LSWISH) {
        v = p1 * t + (1.0 - p1) * v;
        dv = p1 + (1.0 - p1) * dv;
      }
      f = v;
      df = dv;
      break;
    }
  }
}

// ---- the net on one stream ---------------------------------------------------------------------------------------

// Runs the dense layers and the final layer on the state column `mine` (stride T), whose first d + e entries the caller
// has set: the input (value stream, s == 0) or a unit tangent (s >= 1).  G lanes form a row group; the tangent streams
// read the value stream's pre-activation from lane 0 of their group.  G == 1: a value stream on its own (the inverse).
// out[i], i < DP: the final layer in unrounded float64 -- g in the value stream, column s - 1 of dg/dx in stream s.
// This is the one place that fixes where float32 roundings happen: a stored state, once, after the concatenation
// weight.
template <int G, int DP>
__device__ __forceinline__ void ires_net(const float* img, float* mine, int T, const IresShape& sh, int s, double p0,
                                         double p1, double (&out)[DP]) {
  const int op = ires_pad4(sh.out_ch), dp = ires_pad4(sh.d);
  const bool value = G == 1 || s == 0;
  int w_in = sh.d + sh.e;
  const float* p = img + 4;
  for (int l = 0; l < sh.depth; ++l) {
    const float eta1 = p[0];
    const double eta2 = (double)p[1];
    const float* bias = p + 4;
    const float* wt = bias + op;
    for (int o = 0; o < op; o += 4) {
      double sum[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) sum[c] = value ? (double)bias[o + c] : 0.0;  // a tangent has no bias
      for (int k = 0; k < w_in; ++k) {
        const double v = (double)mine[k * T];
        const float4 w4 = *reinterpret_cast<const float4*>(wt + k * op + o);
        sum[0] = fma((double)w4.x, v, sum[0]);
        sum[1] = fma((double)w4.y, v, sum[1]);
        sum[2] = fma((double)w4.z, v, sum[2]);
        sum[3] = fma((double)w4.w, v, sum[3]);
      }
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const double pre = G == 1 ? sum[c] : __shfl(sum[c], 0, G);  // the value stream's pre-activation
        if (o + c < sh.out_ch) {
          double f, df;
          ires_act(sh.act, pre, p0, p1, f, df);
          mine[(w_in + o + c) * T] = (float)((value ? f : df * sum[c]) * eta2);
          if (sh.concat) {
            ires_act(sh.act, -pre, p0, p1, f, df);
            mine[(w_in + sh.out_ch + o + c) * T] = (float)((value ? f : -(df * sum[c])) * eta2);
          }
        }
      }
    }
    for (int k = 0; k < w_in; ++k) mine[k * T] *= eta1;
    p = wt + w_in * op;
    w_in += sh.growth;
  }
#pragma unroll
  for (int i = 0; i < DP; ++i) out[i] = (value && i < dp) ? (double)p[i] : 0.0;
  const float* wt = p + dp;
  for (int k = 0; k < w_in; ++k) {
    const double v = (double)mine[k * T];
#pragma unroll
    for (int c = 0; c < DP / 4; ++c) {
      if (4 * c < dp) {
        const float4 w4 = *reinterpret_cast<const float4*>(wt + k * dp + 4 * c);
        out[4 * c + 0] = fma((double)w4.x, v, out[4 * c + 0]);
        out[4 * c + 1] = fma((double)w4.y, v, out[4 * c + 1]);
        out[4 * c + 2] = fma((double)w4.z, v, out[4 * c + 2]);
        out[4 * c + 3] = fma((double)w4.w, v, out[4 * c + 3]);
      }
    }
  }
}

// ---- forward: value + D tangent streams, LU ---------------------------------------------------------------------

template <int G>
__global__ __launch_bounds__(256) void iresnet_forward_kernel(const float* __restrict__ x,
                                                              const float* __restrict__ extra,
                                                              const float* __restrict__ scale,
                                                              const float* __restrict__ image, float* __restrict__ y,
                                                              float* __restrict__ logabsdet, int64_t n, IresShape sh,
                                                              int image_floats) {
  constexpr int DMAX = G == 32 ? 16 : G - 1;
  constexpr int DP = (DMAX + 3) & ~3;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* img = lds;
  float* st = lds + image_floats;
  const int T = blockDim.x, tid = threadIdx.x;
  for (int i = tid; i < image_floats; i += T) img[i] = image[i];
  __syncthreads();
  const double p0 = (double)img[0], p1 = (double)img[1];
  const int d = sh.d, e = sh.e;
  const int s = tid % G;
  const int rows_per_block = T / G;
  const int64_t tiles = (n + rows_per_block - 1) / rows_per_block;
  float* mine = st + tid;

  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    int64_t row = tile * rows_per_block + tid / G;
    const bool live = row < n;
    if (!live) row = n - 1;  // every lane runs (the shuffles need them); only live rows are stored
    const float* xr = x + row * d;
    for (int k = 0; k < d; ++k) mine[k * T] = s == 0 ? xr[k] : (k == s - 1 ? 1.f : 0.f);
    for (int k = 0; k < e; ++k) mine[(d + k) * T] = s == 0 ? extra[row * e + k] : 0.f;

    // g in the value lane, column s - 1 of J in lane s
    double a[DP];
    ires_net<G, DP>(img, mine, T, sh, s, p0, p1, a);
    // y = x + s g with ONE rounding: the sum is formed in float64 from the unrounded g
    const double sc = scale ? (double)scale[row] : 1.0;
#pragma unroll
    for (int i = 0; i < DP; ++i) a[i] *= sc;
    if (s == 0 && live) {
#pragma unroll
      for (int i = 0; i < DP; ++i)
        if (i < d) y[row * d + i] = (float)((double)xr[i] + a[i]);
    }
    // lanes 1..d: column s - 1 of I + s J; the others carry zeros and take part in the shuffles only
    const bool column = s >= 1 && s <= d;
#pragma unroll
    for (int i = 0; i < DP; ++i) {
      if (!column || i >= d) a[i] = 0.0;
      if (column && i == s - 1) a[i] += 1.0;
    }
    double lad = 0.0;
#pragma unroll
    for (int pv = 0; pv < DMAX; ++pv) {
      if (pv < d) {
        // the lane of column pv picks the pivot row
        int r = pv;
        double best = fabs(a[pv]);
#pragma unroll
        for (int i = pv + 1; i < DMAX; ++i) {
          const double m = fabs(a[i]);
          if (i < d && m > best) {
            best = m;
            r = i;
          }
        }
        r = __shfl(r, pv + 1, G);
#pragma unroll
        for (int i = pv + 1; i < DMAX; ++i) {
          if (i == r) {
            const double t = a[pv];
            a[pv] = a[i];
            a[i] = t;
          }
        }
        const double piv = __shfl(a[pv], pv + 1, G);
        lad += log(fabs(piv));
#pragma unroll
        for (int i = pv + 1; i < DMAX; ++i) {
          const double mult = __shfl(piv != 0.0 ? a[i] / piv : 0.0, pv + 1, G);
          a[i] = fma(-mult, a[pv], a[i]);
        }
      }
    }
    if (s == 0 && live) logabsdet[row] = (float)lad;
  }
}

// ---- inverse: value stream only, per-row fixed point --------------------------------------------------------------

// the row's input channels: the iterate and the constant extras (the dense layers rescale both in place)
template <int DP>
__device__ __forceinline__ void ires_load_row(float* mine, int T, const IresShape& sh, const float (&xin)[DP],
                                              const float* __restrict__ er) {
#pragma unroll
  for (int i = 0; i < DP; ++i)
    if (i < sh.d) mine[i * T] = xin[i];
  for (int k = 0; k < sh.e; ++k) mine[(sh.d + k) * T] = er[k];
}

template <int DP>
__global__ __launch_bounds__(256) void iresnet_inverse_kernel(const float* __restrict__ y,
                                                              const float* __restrict__ extra,
                                                              const float* __restrict__ scale,
                                                              const float* __restrict__ image, float* __restrict__ x,
                                                              uint32_t* __restrict__ max_iters, int64_t n, IresShape sh,
                                                              int image_floats, int max_iterations, float atol,
                                                              float rtol) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* img = lds;
  float* st = lds + image_floats;
  const int T = blockDim.x, tid = threadIdx.x;
  for (int i = tid; i < image_floats; i += T) img[i] = image[i];
  __syncthreads();
  const double p0 = (double)img[0], p1 = (double)img[1];
  const int d = sh.d;
  const int64_t tiles = (n + T - 1) / T;
  float* mine = st + tid;
  uint32_t most = 0;

  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    int64_t row = tile * T + tid;
    const bool live = row < n;
    if (!live) row = n - 1;
    const float* er = extra + row * sh.e;  // read only when e > 0
    const double sc = scale ? (double)scale[row] : 1.0;
    float yv[DP], tol[DP], xc[DP];
    double g[DP];
#pragma unroll
    for (int i = 0; i < DP; ++i) {
      yv[i] = i < d ? y[row * d + i] : 0.f;
      tol[i] = atol + fabsf(yv[i]) * rtol;
    }
    // x0 = y - s g(y), compared with y first, as the reference's loop does
    ires_load_row<DP>(mine, T, sh, yv, er);
    ires_net<1, DP>(img, mine, T, sh, 0, p0, p1, g);
    bool done = true;
#pragma unroll
    for (int i = 0; i < DP; ++i) {
      xc[i] = (float)((double)yv[i] - sc * g[i]);  // one rounding per iterate
      if (i < d && !(fabsf(xc[i] - yv[i]) <= tol[i])) done = false;
    }
    uint32_t it = 0;
    while (!done && it < (uint32_t)max_iterations) {
      ires_load_row<DP>(mine, T, sh, xc, er);
      ires_net<1, DP>(img, mine, T, sh, 0, p0, p1, g);
      done = true;
#pragma unroll
      for (int i = 0; i < DP; ++i) {
        const float xn = (float)((double)yv[i] - sc * g[i]);
        if (i < d && !(fabsf(xn - xc[i]) <= tol[i])) done = false;
        xc[i] = xn;
      }
      ++it;
    }
    if (live) {
#pragma unroll
      for (int i = 0; i < DP; ++i)
        if (i < d) x[row * d + i] = xc[i];
      most = it > most ? it : most;
    }
  }
  if (max_iters) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const uint32_t other = (uint32_t)__shfl_xor((int)most, off, 64);
      most = other > most ? other : most;
    }
    if ((tid & 63) == 0 && most > 0) atomicMax(max_iters, most);
  }
}

// ---- launch ---------------------------------------------------------------------------------------------------------

constexpr int kIresLdsLimit = 128 * 1024;
constexpr int kIresMaxBlocks = 2048;

static bool ires_shape(int d, int e, int depth, int growth, int act, int image_floats, IresShape* sh) {
  if (d < 1 || d > FC_IRES_MAX_DIM || e < 0 || depth < 1 || depth > FC_IRES_MAX_DEPTH || growth < 1) return false;
  if (act < 0 || act > FC_IRES_ACT_LEAKY_LSWISH) return false;
  const bool concat = act == FC_IRES_ACT_CLIPSWISH || act == FC_IRES_ACT_CSIN;
  if (concat && growth % 2 != 0) return false;
  const int64_t wtot = (int64_t)d + e + (int64_t)depth * growth;
  if (wtot > FC_IRES_MAX_WIDTH) return false;
  sh->d = d;
  sh->e = e;
  sh->depth = depth;
  sh->growth = growth;
  sh->concat = concat ? 1 : 0;
  sh->out_ch = concat ? growth / 2 : growth;
  sh->act = act;
  sh->wtot = (int)wtot;
  return ires_image_floats(*sh) == image_floats;
}

// the largest block (256, 128, 64 threads) whose image + state fits 64 KiB, else 64 threads (<= 128 KiB by the limits)
static int ires_threads(const IresShape& sh, int image_floats, int min_threads, size_t* lds) {
  int threads = 256;
  for (;; threads >>= 1) {
    *lds = sizeof(float) * ((size_t)image_floats + (size_t)sh.wtot * threads);
    if (*lds <= 64 * 1024 || threads <= 64 || threads <= min_threads) break;
  }
  return threads;
}

template <int G>
static int launch_ires_forward(const float* x, const float* extra, const float* scale, const float* image, float* y,
                               float* logabsdet, int64_t n, const IresShape& sh, int image_floats, hipStream_t s) {
  size_t lds;
  const int threads = ires_threads(sh, image_floats, G, &lds);
  if (lds > (size_t)kIresLdsLimit) return hipErrorInvalidConfiguration;
  static PerDeviceOnce once;
  const hipError_t e = ensure_max_dynamic_lds(once, reinterpret_cast<const void*>(&iresnet_forward_kernel<G>),
                                              kIresLdsLimit);
  if (e != hipSuccess) return e;
  const int rows = threads / G;
  int64_t grid = (n + rows - 1) / rows;
  if (grid > kIresMaxBlocks) grid = kIresMaxBlocks;
  hipLaunchKernelGGL((iresnet_forward_kernel<G>), dim3((unsigned)grid), dim3(threads), lds, s, x, extra, scale, image,
                     y, logabsdet, n, sh, image_floats);
  return hipGetLastError();
}

template <int DP>
static int launch_ires_inverse(const float* y, const float* extra, const float* scale, const float* image, float* x,
                               uint32_t* max_iters, int64_t n, const IresShape& sh, int image_floats,
                               int max_iterations, float atol, float rtol, hipStream_t s) {
  size_t lds;
  const int threads = ires_threads(sh, image_floats, 64, &lds);
  if (lds > (size_t)kIresLdsLimit) return hipErrorInvalidConfiguration;
  static PerDeviceOnce once;
  const hipError_t e = ensure_max_dynamic_lds(once, reinterpret_cast<const void*>(&iresnet_inverse_kernel<DP>),
                                              kIresLdsLimit);
  if (e != hipSuccess) return e;
  int64_t grid = (n + threads - 1) / threads;
  if (grid > kIresMaxBlocks) grid = kIresMaxBlocks;
  hipLaunchKernelGGL((iresnet_inverse_kernel<DP>), dim3((unsigned)grid), dim3(threads), lds, s, y, extra, scale, image,
                     x, max_iters, n, sh, image_floats, max_iterations, atol, rtol);
  return hipGetLastError();
}

}  // namespace fc

extern "C" int fc_iresnet_forward(const float* x, const float* extra, const float* scale, const float* image, float* y,
                                  float* logabsdet, int64_t n, int32_t d, int32_t e, int32_t depth, int32_t growth,
                                  int32_t activation, int32_t image_floats, void* stream) {
  fc::IresShape sh;
  if (n < 0 || !fc::ires_shape(d, e, depth, growth, activation, image_floats, &sh)) return hipErrorInvalidValue;
  if (n == 0) return hipSuccess;
  if (!x || !image || !y || !logabsdet || x == y || (e > 0 && !extra)) return hipErrorInvalidValue;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (d < 2) return fc::launch_ires_forward<2>(x, extra, scale, image, y, logabsdet, n, sh, image_floats, s);
  if (d < 4) return fc::launch_ires_forward<4>(x, extra, scale, image, y, logabsdet, n, sh, image_floats, s);
  if (d < 8) return fc::launch_ires_forward<8>(x, extra, scale, image, y, logabsdet, n, sh, image_floats, s);
  if (d < 16) return fc::launch_ires_forward<16>(x, extra, scale, image, y, logabsdet, n, sh, image_floats, s);
  return fc::launch_ires_forward<32>(x, extra, scale, image, y, logabsdet, n, sh, image_floats, s);
}

extern "C" int fc_iresnet_inverse(const float* y, const float* extra, const float* scale, const float* image, float* x,
                                  uint32_t* max_iters, int64_t n, int32_t d, int32_t e, int32_t depth, int32_t growth,
                                  int32_t activation, int32_t image_floats, int32_t max_iterations, float atol,
                                  float rtol, void* stream) {
  fc::IresShape sh;
  if (n < 0 || max_iterations < 0 || !(atol >= 0.f) || !(rtol >= 0.f)) return hipErrorInvalidValue;
  if (!fc::ires_shape(d, e, depth, growth, activation, image_floats, &sh)) return hipErrorInvalidValue;
  if (n == 0) return hipSuccess;
  if (!y || !image || !x || x == y || (e > 0 && !extra)) return hipErrorInvalidValue;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (d <= 4)
    return fc::launch_ires_inverse<4>(y, extra, scale, image, x, max_iters, n, sh, image_floats, max_iterations, atol,
                                      rtol, s);
  if (d <= 8)
    return fc::launch_ires_inverse<8>(y, extra, scale, image, x, max_iters, n, sh, image_floats, max_iterations, atol,
                                      rtol, s);
  return fc::launch_ires_inverse<16>(y, extra, scale, image, x, max_iters, n, sh, image_floats, max_iterations, atol,
                                     rtol, s);
}
