// Invertible residual blocks over Lipschitz-constrained DenseNets (reference
// flowcon/transforms/lipschitz/iresblock.py with flowcon/nn/nets/invertible_densenet.py, lipschitz_dense.py).
//
//   fc_iresnet_forward   y = x + s g(x),  logabsdet = log|det(I + s dg/dx)|      one launch
//   fc_iresnet_inverse   x with x + s g(x) = y by the fixed-point iteration x <- y - s g(x), every row to its own
//                        convergence                                             one launch
//   fc_iresnet_backward  the reverse sweep of fc_iresnet_forward: gradients of the rows, the per-row operands and
//                        every entry of the image, the streams recomputed in LDS      one launch + a reduction
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
//
// Backward: the forward's lane groups and LDS layout plus an adjoint state of the same shape.  A tile recomputes the
// streams through ires_net, inverts I + s J inside the lane group (the cotangent of column j of J is gl s (A^-T)[:, j]),
// and sweeps the layers from the last; every block adds its parameter-gradient sums onto one image-shaped float64
// partial, each entry by one thread in a fixed order, and partial_sum_kernel (fc_partial_sum.h) adds the partials in
// block order (no atomics).  See DESIGN.md, "iResBlock training".
//
// The lane groups, the block set-up (GroupBlock), the float64 weight sums and the launch plan are the lane-group
// scaffold's (fc_lane_group.h), which the CNF kernels share; this file keeps the image layout, the activations, the
// concatenating dense layers, the LU, the fixed-point loop and the reverse sweep.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/flowcon_hip.h"
#include "fc_lane_group.h"
#include "fc_partial_sum.h"

namespace fc {

struct IresShape {
  int d, e, depth, growth, out_ch, concat, act, wtot;
};

__host__ __device__ inline int ires_image_floats(const IresShape& sh) {
  int total = 4, w_in = sh.d + sh.e;
  const int op = pad4(sh.out_ch);
  for (int l = 0; l < sh.depth; ++l) {
    total += 4 + op + w_in * op;
    w_in += sh.growth;
  }
  const int dp = pad4(sh.d);
  return total + dp + w_in * dp;
}

// value f(t) and derivative f'(t) of the element-wise part of the activation (for the concatenating ones the caller
// evaluates at t and at -t).  Evaluated in float64 on the float64 pre-activation: the value a stream stores is rounded
// to float32 once, after the concatenation weight.  SECOND adds what the reverse sweep of fc_iresnet_backward needs:
// f''(t) and the derivatives of f and f' with respect to the activation scalars p0 / p1.
struct IresActJet {
  double f, df, d2f, f_p0, df_p0, f_p1, df_p1;
};

template <bool SECOND>
__device__ __forceinline__ void ires_act_jet(int act, double t, double p0, double p1, IresActJet& r) {
  r.d2f = r.f_p0 = r.df_p0 = r.f_p1 = r.df_p1 = 0.0;
  switch (act) {
    case FC_IRES_ACT_RELU:
      r.f = t > 0.0 ? t : 0.0;
      r.df = t > 0.0 ? 1.0 : 0.0;
      break;
    case FC_IRES_ACT_TANH: {
      const double th = tanh(t);
      r.f = th;
      r.df = 1.0 - th * th;
      if (SECOND) r.d2f = -2.0 * th * r.df;
      break;
    }
    case FC_IRES_ACT_ELU: {
      r.f = t > 0.0 ? t : p0 * expm1(t);
      r.df = t > 0.0 ? 1.0 : p0 * exp(t);
      if (SECOND) {
        r.d2f = t > 0.0 ? 0.0 : r.df;
        r.f_p0 = t > 0.0 ? 0.0 : expm1(t);
        r.df_p0 = t > 0.0 ? 0.0 : exp(t);
      }
      break;
    }
    case FC_IRES_ACT_SIN:
    case FC_IRES_ACT_CSIN: {
      const double a = p0 * t;
      const double div = act == FC_IRES_ACT_CSIN ? 1.41421356237309504880 : 1.0;
      r.f = sin(a) / (p0 * div);
      r.df = cos(a) / div;
      if (SECOND) {
        r.d2f = -(p0 * sin(a)) / div;
        r.f_p0 = (a * cos(a) - sin(a)) / (p0 * p0 * div);
        r.df_p0 = -(t * sin(a)) / div;
      }
      break;
    }
    default: {  // the Swish family: t sigmoid(b t) / 1.1 (/ 1.004 for LipSwish, CLipSwish), LeakyLSwish mixes with t
      const double sg = 1.0 / (1.0 + exp(-p0 * t));
      double v = t * sg / 1.1;
      double dv = (sg + p0 * t * sg * (1.0 - sg)) / 1.1;
      // q = sg (1 - sg): d sg / dt = p0 q, d sg / dp0 = t q, dq / d(p0 t) = q (1 - 2 sg)
      const double q = sg * (1.0 - sg);
      const double bend = q * (2.0 + p0 * t * (1.0 - 2.0 * sg)) / 1.1;
      double d2v = p0 * bend, v_p0 = t * t * q / 1.1, dv_p0 = t * bend;
      if (act == FC_IRES_ACT_LIPSWISH || act == FC_IRES_ACT_CLIPSWISH) {
        v = v / 1.004;
        dv = dv / 1.004;
        d2v = d2v / 1.004;
        v_p0 = v_p0 / 1.004;
        dv_p0 = dv_p0 / 1.004;
      } else if (act == FC_IRES_ACT_LEAKY_LSWISH) {
        if (SECOND) {
          r.f_p1 = t - v;
          r.df_p1 = 1.0 - dv;
        }
        v = p1 * t + (1.0 - p1) * v;
        dv = p1 + (1.0 - p1) * dv;
        d2v = (1.0 - p1) * d2v;
        v_p0 = (1.0 - p1) * v_p0;
        dv_p0 = (1.0 - p1) * dv_p0;
      }
      r.f = v;
      r.df = dv;
      if (SECOND) {
        r.d2f = d2v;
        r.f_p0 = v_p0;
        r.df_p0 = dv_p0;
      }
      break;
    }
  }
}

__device__ __forceinline__ void ires_act(int act, double t, double p0, double p1, double& f, double& df) {
  IresActJet r;
  ires_act_jet<false>(act, t, p0, p1, r);
  f = r.f;
  df = r.df;
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
  const int op = pad4(sh.out_ch), dp = pad4(sh.d);
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
      weight_sum4(wt, mine, T, w_in, op, o, value, [&](int oc) { return (double)bias[oc]; }, sum);
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
  constexpr int DMAX = LaneGroup<G>::DMAX, DP = LaneGroup<G>::DP;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const GroupBlock b = group_block<G>(lds, image, image_floats, 0, 0, n);
  __syncthreads();
  const float* img = b.img;
  float* mine = b.mine;
  const double p0 = (double)img[0], p1 = (double)img[1];
  const int T = b.T, d = sh.d, e = sh.e, s = b.s;

  for (int64_t tile = blockIdx.x; tile < b.tiles; tile += gridDim.x) {
    bool live;
    const int64_t row = tile_row(b, tile, n, live);
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
  const GroupBlock b = group_block<1>(lds, image, image_floats, 0, 0, n);  // a group of one lane: a row per thread
  __syncthreads();
  const float* img = b.img;
  float* mine = b.mine;
  const double p0 = (double)img[0], p1 = (double)img[1];
  const int T = b.T, tid = b.tid, d = sh.d;
  uint32_t most = 0;

  for (int64_t tile = blockIdx.x; tile < b.tiles; tile += gridDim.x) {
    bool live;
    const int64_t row = tile_row(b, tile, n, live);
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

// ---- backward: recompute the streams, invert I + s J, sweep the layers from the last ----------------------------------

// part[at + k * ld + o] += sum over the block's streams of lhs[o][t] * st[k][t] for k < rows, and the bias entries
// part[bias_at + o] += sum over the VALUE streams of lhs[o][t] (a tangent has no bias), o < cols.  One (k, o) per
// thread and pass; the sum over t is a float64 fma chain that starts at the thread's own lane (conflict-free LDS
// reads), so its order is a function of the entry alone and a rerun gives the same bits.
template <int G>
__device__ __forceinline__ void ires_outer_sums(double* part, int at, int bias_at, int ld, int cols, int rows,
                                                const float* lhs, const float* st, int T, int tid) {
  for (int idx = tid; idx < (rows + 1) * ld; idx += T) {
    const int k = idx / ld, o = idx - k * ld;
    if (o >= cols) continue;
    const float* l = lhs + o * T;
    double sum = 0.0;
    if (k < rows) {
      const float* r = st + k * T;
      for (int i = 0; i < T; ++i) {
        const int t = (tid + i) & (T - 1);
        sum = fma((double)l[t], (double)r[t], sum);
      }
      part[at + k * ld + o] += sum;
    } else {
      for (int i = 0; i < T; i += G) sum += (double)l[((tid & ~(G - 1)) + i) & (T - 1)];
      part[bias_at + o] += sum;
    }
  }
}

// LDS: the image, the state st[wtot][T] and its adjoint adj[wtot][T] (one column per stream, as the forward keeps its
// state), cb[dp][T] for the rows of (I + s J)^-1 on their way to the lanes that need them and then for the cotangent of
// the final layer, and two float64 words per wave for the concatenation weights' sums.  A block owns one image-shaped
// float64 partial of ws and adds every tile's sums onto it: each entry by one thread, always the same one.
template <int G>
__global__ __launch_bounds__(256) void iresnet_backward_kernel(
    const float* __restrict__ x, const float* __restrict__ extra, const float* __restrict__ scale,
    const float* __restrict__ image, const float* __restrict__ gy, const float* __restrict__ gl,
    float* __restrict__ dx, float* __restrict__ dextra, float* __restrict__ dscale, double* __restrict__ ws, int64_t n,
    IresShape sh, int image_floats) {
  constexpr int DMAX = LaneGroup<G>::DMAX, DP = LaneGroup<G>::DP;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const GroupBlock b = group_block<G>(lds, image, image_floats, 0, 0, n);
  const int T = b.T, tid = b.tid, s = b.s;
  const int d = sh.d, e = sh.e, op = pad4(sh.out_ch), dp = pad4(d), wtot = sh.wtot;
  const float* img = b.img;
  float* st = b.st;
  float* adj = st + wtot * T;
  float* cb = adj + wtot * T;
  double* red = reinterpret_cast<double*>(cb + dp * T);
  double* part = ws + (size_t)blockIdx.x * image_floats;
  for (int i = tid; i < image_floats; i += T) part[i] = 0.0;
  __syncthreads();
  const double p0 = (double)img[0], p1 = (double)img[1];
  const bool value = s == 0;
  float* mine = b.mine;
  float* adjm = adj + tid;
  const int final_at = image_floats - dp - wtot * dp;
  double dp0 = 0.0, dp1 = 0.0;

  for (int64_t tile = blockIdx.x; tile < b.tiles; tile += gridDim.x) {
    bool live;  // a row beyond the batch carries zero cotangents
    const int64_t row = tile_row(b, tile, n, live);
    const float* xr = x + row * d;
    for (int k = 0; k < d; ++k) mine[k * T] = value ? xr[k] : (k == s - 1 ? 1.f : 0.f);
    for (int k = 0; k < e; ++k) mine[(d + k) * T] = value ? extra[row * e + k] : 0.f;

    // the forward again: g in the value lane, column s - 1 of J in lane s
    double c[DP];
    {
      double jc[DP], a[DP], b[DP];
      ires_net<G, DP>(img, mine, T, sh, s, p0, p1, jc);
      const double sc = scale ? (double)scale[row] : 1.0;
      const double glv = live ? (double)gl[row] : 0.0;
      const bool column = s >= 1 && s <= d;
      // Gauss-Jordan on [I + s J | I], one column of either half per lane: the row operations of the pivot column's
      // lane, handed round by shuffles, leave column s - 1 of the inverse in lane s
#pragma unroll
      for (int i = 0; i < DP; ++i) {
        a[i] = column && i < d ? sc * jc[i] : 0.0;
        b[i] = 0.0;
        if (column && i == s - 1) {
          a[i] += 1.0;
          b[i] = 1.0;
        }
      }
#pragma unroll
      for (int pv = 0; pv < DMAX; ++pv) {
        if (pv < d) {
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
              double t = a[pv];
              a[pv] = a[i];
              a[i] = t;
              t = b[pv];
              b[pv] = b[i];
              b[i] = t;
            }
          }
          const double piv = __shfl(a[pv], pv + 1, G);
          const double inv = piv != 0.0 ? 1.0 / piv : 0.0;
#pragma unroll
          for (int i = 0; i < DMAX; ++i) {
            if (i != pv) {
              const double mult = __shfl(a[i] * inv, pv + 1, G);
              a[i] = fma(-mult, a[pv], a[i]);
              b[i] = fma(-mult, b[pv], b[i]);
            }
          }
          a[pv] *= inv;
          b[pv] *= inv;
        }
      }
      // lane s needs ROW s - 1 of the inverse (the cotangent of column s - 1 of J is gl s (A^-T)[:, s - 1])
#pragma unroll
      for (int i = 0; i < DP; ++i)
        if (i < d) cb[i * T + tid] = (float)b[i];
      __syncthreads();
      double ds = 0.0;
#pragma unroll
      for (int i = 0; i < DP; ++i) {
        c[i] = 0.0;
        if (i < d && value) {
          const double g = live ? (double)gy[row * d + i] : 0.0;
          c[i] = sc * g;
          ds = fma(g, jc[i], ds);
        } else if (i < d && column) {
          const double inv_row = (double)cb[(s - 1) * T + tid - s + 1 + i];
          c[i] = glv * sc * inv_row;
          ds = fma(glv * inv_row, jc[i], ds);
        }
      }
      ds = lane_sum<G>(ds);  // <gy, g> + gl tr(A^-1 J)
      if (value && live && dscale) dscale[row] = (float)ds;
      __syncthreads();
    }

    // the final layer: its input is the state as the forward left it
    {
      const float* wt = img + final_at + dp;
#pragma unroll
      for (int i = 0; i < DP; ++i)
        if (i < dp) cb[i * T + tid] = (float)c[i];
      for (int k = 0; k < wtot; ++k) {
        double acc = 0.0;
#pragma unroll
        for (int q = 0; q < DP / 4; ++q) {
          if (4 * q < dp) {
            const float4 w4 = *reinterpret_cast<const float4*>(wt + k * dp + 4 * q);
            acc = fma((double)w4.x, c[4 * q + 0], acc);
            acc = fma((double)w4.y, c[4 * q + 1], acc);
            acc = fma((double)w4.z, c[4 * q + 2], acc);
            acc = fma((double)w4.w, c[4 * q + 3], acc);
          }
        }
        adjm[k * T] = (float)acc;
      }
      __syncthreads();
      ires_outer_sums<G>(part, final_at + dp, final_at, dp, d, wtot, cb, st, T, tid);
      __syncthreads();
    }

    // the dense layers, last first.  Entering layer l the state holds the layer's OUTPUT; dividing its first w_in
    // entries by eta1 gives the layer's input back (the forward scaled them in place).
    int at = final_at;
    for (int l = sh.depth - 1; l >= 0; --l) {
      const int w_in = d + e + l * sh.growth;
      at -= 4 + op + w_in * op;
      const float* lp = img + at;
      const double eta1 = (double)lp[0], eta2 = (double)lp[1];
      const float* bias = lp + 4;
      const float* wt = bias + op;
      double de1 = 0.0, de2 = 0.0;
      for (int k = 0; k < w_in; ++k) {
        const float h = (float)((double)mine[k * T] / eta1);
        mine[k * T] = h;
        de1 = fma((double)adjm[k * T], (double)h, de1);
      }
      for (int o = 0; o < op; o += 4) {
        double sum[4];
        weight_sum4(wt, mine, T, w_in, op, o, value, [&](int oc) { return (double)bias[oc]; }, sum);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const double pre = __shfl(sum[q], 0, G);
          if (o + q < sh.out_ch) {  // uniform over the block
            IresActJet f1, f2;
            ires_act_jet<true>(sh.act, pre, p0, p1, f1);
            const double a1 = (double)adjm[(w_in + o + q) * T];
            double a2 = 0.0;
            f2.f = f2.df = f2.d2f = f2.f_p0 = f2.df_p0 = f2.f_p1 = f2.df_p1 = 0.0;
            if (sh.concat) {
              ires_act_jet<true>(sh.act, -pre, p0, p1, f2);
              a2 = (double)adjm[(w_in + sh.out_ch + o + q) * T];
            }
            // value stream: h = eta2 [f(pre), f(-pre)];  tangent: t = eta2 [f'(pre) u, -f'(-pre) u], u = W t_in
            const double u = value ? 1.0 : sum[q];
            double apre, bend = 0.0;
            if (value) {
              apre = eta2 * (f1.df * a1 - f2.df * a2);
              de2 += f1.f * a1 + f2.f * a2;
              dp0 += eta2 * (f1.f_p0 * a1 + f2.f_p0 * a2);
              dp1 += eta2 * (f1.f_p1 * a1 + f2.f_p1 * a2);
            } else {
              apre = eta2 * (f1.df * a1 - f2.df * a2);
              bend = eta2 * u * (f1.d2f * a1 + f2.d2f * a2);
              de2 += u * (f1.df * a1 - f2.df * a2);
              dp0 += eta2 * u * (f1.df_p0 * a1 - f2.df_p0 * a2);
              dp1 += eta2 * u * (f1.df_p1 * a1 - f2.df_p1 * a2);
            }
            // the value stream's pre-activation also moves every tangent through f''
            bend = lane_sum<G>(bend);
            if (value) apre += bend;
            adjm[(w_in + o + q) * T] = (float)apre;
          }
        }
      }
      de1 = lane_sum<64>(de1);
      de2 = lane_sum<64>(de2);
      if ((tid & 63) == 0) {
        red[2 * (tid >> 6)] = de1;
        red[2 * (tid >> 6) + 1] = de2;
      }
      __syncthreads();
      ires_outer_sums<G>(part, at + 4 + op, at + 4, op, sh.out_ch, w_in, adj + w_in * T, st, T, tid);
      if (tid == 0) {
        for (int w = 0; w < T / 64; ++w) {
          part[at] += red[2 * w];
          part[at + 1] += red[2 * w + 1];
        }
      }
      // adjoint of the layer's input: eta1 times that of the copied entries plus W^T adj_pre
      for (int k = 0; k < w_in; ++k) {
        double acc = eta1 * (double)adjm[k * T];
        for (int o = 0; o < op; o += 4) {
          const float4 w4 = *reinterpret_cast<const float4*>(wt + k * op + o);
          const float w[4] = {w4.x, w4.y, w4.z, w4.w};
#pragma unroll
          for (int q = 0; q < 4; ++q)
            if (o + q < sh.out_ch) acc = fma((double)w[q], (double)adjm[(w_in + o + q) * T], acc);
        }
        adjm[k * T] = (float)acc;
      }
      __syncthreads();
    }

    if (value && live) {
      for (int k = 0; k < d; ++k) dx[row * d + k] = (float)((double)gy[row * d + k] + (double)adjm[k * T]);
      for (int k = 0; k < e; ++k) dextra[row * e + k] = adjm[(d + k) * T];
    }
  }

  dp0 = lane_sum<64>(dp0);
  dp1 = lane_sum<64>(dp1);
  if ((tid & 63) == 0) {
    red[2 * (tid >> 6)] = dp0;
    red[2 * (tid >> 6) + 1] = dp1;
  }
  __syncthreads();
  if (tid == 0) {
    for (int w = 0; w < T / 64; ++w) {
      part[0] += red[2 * w];
      part[1] += red[2 * w + 1];
    }
  }
}

// ---- entry and launch -------------------------------------------------------------------------------------------------

static bool ires_shape(int d, int e, int depth, int growth, int act, IresShape* sh) {
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
  return true;
}

// what every launching entry point starts with: a row count, a net within the limits, the image it says
static bool ires_entry(int64_t n, int d, int e, int depth, int growth, int act, int image_floats, IresShape* sh) {
  return n >= 0 && ires_shape(d, e, depth, growth, act, sh) && ires_image_floats(*sh) == image_floats;
}

// The state columns of the forward (group lanes a row) and of the inverse (group 1: a row per thread).  The widest net
// the limits admit needs 67.5 KiB at 64 threads; a plan that did not fit comes back with 0 threads, which group_launch
// answers with an error.
static GroupLaunch ires_plan(const IresShape& sh, int image_floats, int group, int64_t n) {
  return group_launch_plan(image_floats, group, GroupLds{0, sh.wtot, 0, 0}, kPrefer64K, n, kGroupMaxBlocks);
}

// The backward's LDS: state, adjoint state, dp cotangent rows and two float64 words per wave.  Worst case (d 16, width
// 128, 8692-float image): 4 (8692 + 272 * 64) + 16 = 104 416 bytes.  The workspace is a partial per block of this grid.
static GroupLaunch ires_backward_plan(const IresShape& sh, int image_floats, int64_t n, int max_blocks) {
  const int cap = max_blocks > 0 && max_blocks < kGroupBackwardMaxBlocks ? max_blocks : kGroupBackwardMaxBlocks;
  return group_launch_plan(image_floats, lane_group(sh.d), GroupLds{0, 2 * sh.wtot + pad4(sh.d), 0, 2}, kPrefer64K, n,
                           cap);
}

}  // namespace fc

extern "C" int fc_iresnet_backward_workspace(int64_t n, int32_t d, int32_t e, int32_t depth, int32_t growth,
                                             int32_t activation, int32_t max_blocks) {
  fc::IresShape sh;
  // (ires_shape alone rejects an e or a growth past the width limit, before anything is computed from them; the two
  // bounds are the entry's documented ones, stated here as well)
  if (n < 0 || e > FC_IRES_MAX_WIDTH || growth > FC_IRES_MAX_WIDTH) return -1;
  if (!fc::ires_shape(d, e, depth, growth, activation, &sh)) return -1;
  if (n == 0) return 0;
  const int image_floats = fc::ires_image_floats(sh);
  return (int)(fc::ires_backward_plan(sh, image_floats, n, max_blocks).grid * image_floats);
}

extern "C" int fc_iresnet_backward(const float* x, const float* extra, const float* scale, const float* image,
                                   const float* gy, const float* gl, float* dx, float* dextra, float* dscale,
                                   float* dimage, double* ws, int64_t n, int32_t d, int32_t e, int32_t depth,
                                   int32_t growth, int32_t activation, int32_t image_floats, int32_t max_blocks,
                                   void* stream) {
  fc::IresShape sh;
  if (!fc::ires_entry(n, d, e, depth, growth, activation, image_floats, &sh)) return hipErrorInvalidValue;
  if (!dimage) return hipErrorInvalidValue;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (n == 0) return hipMemsetAsync(dimage, 0, sizeof(float) * image_floats, s);
  if (!x || !image || !gy || !gl || !dx || !ws || (e > 0 && (!extra || !dextra)) || (scale && !dscale))
    return hipErrorInvalidValue;
  const fc::GroupLaunch plan = fc::ires_backward_plan(sh, image_floats, n, max_blocks);
  const int launched = fc::with_constant<2, 4, 8, 16, 32>(fc::lane_group(d), [&](auto g) {
    return fc::group_launch<&fc::iresnet_backward_kernel<decltype(g)::value>>(
        plan, s, x, extra, scale, image, gy, gl, dx, dextra, dscale, ws, n, sh, image_floats);
  });
  if (launched != hipSuccess) return launched;
  return fc::launch_partial_sum(ws, dimage, (int)plan.grid, image_floats, 1.0, s);
}

extern "C" int fc_iresnet_forward(const float* x, const float* extra, const float* scale, const float* image, float* y,
                                  float* logabsdet, int64_t n, int32_t d, int32_t e, int32_t depth, int32_t growth,
                                  int32_t activation, int32_t image_floats, void* stream) {
  fc::IresShape sh;
  if (!fc::ires_entry(n, d, e, depth, growth, activation, image_floats, &sh)) return hipErrorInvalidValue;
  if (n == 0) return hipSuccess;
  if (!x || !image || !y || !logabsdet || x == y || (e > 0 && !extra)) return hipErrorInvalidValue;
  const int group = fc::lane_group(d);
  const fc::GroupLaunch plan = fc::ires_plan(sh, image_floats, group, n);
  return fc::with_constant<2, 4, 8, 16, 32>(group, [&](auto g) {
    return fc::group_launch<&fc::iresnet_forward_kernel<decltype(g)::value>>(
        plan, static_cast<hipStream_t>(stream), x, extra, scale, image, y, logabsdet, n, sh, image_floats);
  });
}

extern "C" int fc_iresnet_inverse(const float* y, const float* extra, const float* scale, const float* image, float* x,
                                  uint32_t* max_iters, int64_t n, int32_t d, int32_t e, int32_t depth, int32_t growth,
                                  int32_t activation, int32_t image_floats, int32_t max_iterations, float atol,
                                  float rtol, void* stream) {
  fc::IresShape sh;
  if (max_iterations < 0 || !(atol >= 0.f) || !(rtol >= 0.f)) return hipErrorInvalidValue;
  if (!fc::ires_entry(n, d, e, depth, growth, activation, image_floats, &sh)) return hipErrorInvalidValue;
  if (n == 0) return hipSuccess;
  if (!y || !image || !x || x == y || (e > 0 && !extra)) return hipErrorInvalidValue;
  const fc::GroupLaunch plan = fc::ires_plan(sh, image_floats, 1, n);
  return fc::with_constant<4, 8, 16>(d <= 4 ? 4 : d <= 8 ? 8 : 16, [&](auto dp) {  // the padded d
    return fc::group_launch<&fc::iresnet_inverse_kernel<decltype(dp)::value>>(
        plan, static_cast<hipStream_t>(stream), y, extra, scale, image, x, max_iters, n, sh, image_floats,
        max_iterations, atol, rtol);
  });
}
