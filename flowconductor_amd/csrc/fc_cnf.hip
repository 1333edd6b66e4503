// Continuous normalizing flows (reference flowcon/CNF/cnf.py with neural_odes/odefunc.py and
// neural_odes/diffeq_layers/basic.py).
//
//   fc_cnf_field       dy = f(t, y) and -div_y f(t, y) of an ODEnet over time-conditioned linear layers    one launch
//   fc_cnf_integrate   z(t1), logp(t1) from z(t0), logp(t0) under d/dt (z, logp) = (f, -div f) with a fixed-step
//                      Runge-Kutta method, every row on its own                                            one launch
//   fc_cnf_field_train / fc_cnf_field_backward   one evaluation as an autograd node: the exact divergence or
//                      Hutchinson's estimate, and the gradients of both outputs (further down)
// (fc_cnf_dopri5, the adaptive solve with per-row step control, is in fc_cnf_dopri5.hip; what the kernels share --
// CnfShape, the activations, cnf_time_table, cnf_net, cnf_field_row -- is in fc_cnf.h.)
//
// f is an MLP whose layers all reduce to
//     pre = W x + b + w_t t,   out = pre * gate + w_b t,   gate = sigmoid(w_g t + b_g)  or  1
// (ignore / concat / concat_v2 / squash / concatsquash), an element-wise activation between the layers and none after
// the last.  The host hands over an IMAGE of the net, all of it float32, every piece on a 16-byte boundary, per layer
//     b[op] w_t[op] w_g[op] b_g[op] w_b[op] wt[in][op]        op = out rounded up to 4, wt[k][o] = W[o][k]
// with zero padding.  A block copies the image into LDS once and walks over row tiles.
//
// The exact divergence is a forward-mode computation of the same shape as f, laid out like ires_net
// (fc_iresblock.hip): a row is carried by a group of G lanes (the smallest power of two >= d + 1), lane 0 runs the
// value stream, lane j + 1 the tangent d/dy_j (no bias, no time terms); the tangent streams pick the value stream's
// gated pre-activation up with a shuffle inside the group for the activation's derivative.  Activations ping-pong in
// LDS as st[k][thread].  Lane j + 1 ends with row j of its Jacobian column, of which only df_j/dy_j is used: the
// divergence is a sum over the group, no LU.
//
// Whatever depends on t alone (b + w_t t, the gate, w_b t) is the same for every row: the block computes it once per
// evaluation into an LDS table, in float64.  In the integrator all rows of a launch share the step sequence, so the
// table is rebuilt per stage behind a barrier.
//
// Numerics: sums in float64 over the float32 weights, a stored activation rounded to float32 once (cnf_net is the
// one place that decides this); the integrator keeps (z, logp) and the stage slopes in float64 registers and rounds
// a stage's state to float32 where it enters the net.
#include "fc_cnf.h"

namespace fc {

// ---- one evaluation -------------------------------------------------------------------------------------------------

template <int G>
__global__ __launch_bounds__(256) void cnf_field_kernel(const float* __restrict__ y, const float* __restrict__ image,
                                                        float* __restrict__ dy, float* __restrict__ negdiv,
                                                        float* __restrict__ evals, int64_t n, CnfShape sh,
                                                        int image_floats, int table_doubles, float t_host,
                                                        const float* __restrict__ t_dev) {
  constexpr int DP = CnfGroup<G>::DP;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* img = lds;
  double* tab = reinterpret_cast<double*>(lds + image_floats);
  float* st = lds + image_floats + 2 * table_doubles;
  const int T = blockDim.x, tid = threadIdx.x;
  for (int i = tid; i < image_floats; i += T) img[i] = image[i];
  __syncthreads();
  cnf_time_table(img, tab, sh, t_dev ? (double)t_dev[0] : (double)t_host, tid, T);
  __syncthreads();
  const int d = sh.d, s = tid % G, rows_per_block = T / G, half = cnf_max_width(sh) * T;
  const int64_t tiles = (n + rows_per_block - 1) / rows_per_block;
  float* mine = st + tid;
  if (evals && blockIdx.x == 0 && tid == 0) atomicAdd(evals, 1.f);

  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    int64_t row = tile * rows_per_block + tid / G;
    const bool live = row < n;
    if (!live) row = n - 1;  // every lane runs (the shuffles need them); only live rows are stored
    float xin[DP];
#pragma unroll
    for (int i = 0; i < DP; ++i) xin[i] = i < d ? y[row * d + i] : 0.f;
    double k[DP], nd;
    cnf_field_row<G, DP>(img, CnfBlockTime{tab}, mine, T, half, sh, s, xin, k, nd);
    if (s == 0 && live) {
#pragma unroll
      for (int i = 0; i < DP; ++i)
        if (i < d) dy[row * d + i] = (float)k[i];
      negdiv[row] = (float)nd;
    }
  }
}

// ---- the whole solve ------------------------------------------------------------------------------------------------

// Explicit methods whose stage i reads the slope of stage i - 1 only: y_i = y + a_i h k_{i-1}, t_i = t + c_i h,
// y <- y + h sum b_i k_i.  Euler, the explicit midpoint rule, the classical fourth-order Runge-Kutta method.
// (kept as selects, not as arrays: a run-time index into a local array would put it in scratch memory)
__host__ __device__ inline int cnf_stages(int method) {
  return method == FC_CNF_EULER ? 1 : method == FC_CNF_MIDPOINT ? 2 : 4;
}

// c_i, which is a_i as well: a stage that reads one slope sits at t + a_i h
__device__ __forceinline__ double cnf_node(int method, int stage) {
  if (method == FC_CNF_RK4) return stage == 0 ? 0.0 : stage == 3 ? 1.0 : 0.5;
  return stage == 0 ? 0.0 : 0.5;
}

__device__ __forceinline__ double cnf_weight(int method, int stage) {
  if (method == FC_CNF_RK4) return (stage == 0 || stage == 3) ? 1.0 / 6.0 : 1.0 / 3.0;
  if (method == FC_CNF_MIDPOINT) return stage == 1 ? 1.0 : 0.0;
  return 1.0;
}

template <int G>
__global__ __launch_bounds__(256) void cnf_integrate_kernel(const float* __restrict__ z, const float* __restrict__ logp,
                                                            const float* __restrict__ image, float* __restrict__ z_out,
                                                            float* __restrict__ logp_out, float* __restrict__ evals,
                                                            int64_t n, CnfShape sh, int image_floats,
                                                            int table_doubles, double t0, double t1, int steps,
                                                            int method) {
  constexpr int DP = CnfGroup<G>::DP;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* img = lds;
  double* tab = reinterpret_cast<double*>(lds + image_floats);
  float* st = lds + image_floats + 2 * table_doubles;
  const int T = blockDim.x, tid = threadIdx.x;
  for (int i = tid; i < image_floats; i += T) img[i] = image[i];
  const int d = sh.d, s = tid % G, rows_per_block = T / G, half = cnf_max_width(sh) * T;
  const int64_t tiles = (n + rows_per_block - 1) / rows_per_block;
  float* mine = st + tid;
  const int stages = cnf_stages(method);
  const double h = (t1 - t0) / (double)steps;
  bool have_table = false;
  double table_t = 0.0;
  if (evals && blockIdx.x == 0 && tid == 0)  // non-negative floats order like their bit patterns
    atomicMax(reinterpret_cast<int*>(evals), __float_as_int((float)steps * (float)stages));

  // the tile loop's trip count depends on the block alone, so the barriers below are met by every thread
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    int64_t row = tile * rows_per_block + tid / G;
    const bool live = row < n;
    if (!live) row = n - 1;
    double yv[DP], acc[DP], k[DP];
#pragma unroll
    for (int i = 0; i < DP; ++i) {
      yv[i] = i < d ? (double)z[row * d + i] : 0.0;
      k[i] = 0.0;
    }
    double lp = logp ? (double)logp[row] : 0.0, lk = 0.0, lacc;
    for (int step = 0; step < steps; ++step) {
      const double ts = t0 + (double)step * h;
#pragma unroll
      for (int i = 0; i < DP; ++i) acc[i] = 0.0;
      lacc = 0.0;
      for (int stage = 0; stage < stages; ++stage) {
        const double node = cnf_node(method, stage), weight = cnf_weight(method, stage);
        const double tt = ts + node * h;
        if (!have_table || tt != table_t) {
          __syncthreads();  // the image copy, and the readers of the previous table
          cnf_time_table(img, tab, sh, tt, tid, T);
          __syncthreads();
          have_table = true;
          table_t = tt;
        }
        float xin[DP];
        const double ah = node * h;
#pragma unroll
        for (int i = 0; i < DP; ++i) xin[i] = (float)(stage == 0 ? yv[i] : yv[i] + ah * k[i]);
        cnf_field_row<G, DP>(img, CnfBlockTime{tab}, mine, T, half, sh, s, xin, k, lk);
#pragma unroll
        for (int i = 0; i < DP; ++i) acc[i] += weight * k[i];
        lacc += weight * lk;
      }
#pragma unroll
      for (int i = 0; i < DP; ++i) yv[i] += h * acc[i];
      lp += h * lacc;
    }
    if (s == 0 && live) {
#pragma unroll
      for (int i = 0; i < DP; ++i)
        if (i < d) z_out[row * d + i] = (float)yv[i];
      logp_out[row] = (float)lp;
    }
  }
}

// ---- launch ---------------------------------------------------------------------------------------------------------

// the largest block (256, 128, 64 threads) whose image + table + state fits 64 KiB, else 64 threads
static int cnf_threads(const CnfShape& sh, int image_floats, int min_threads, size_t* lds) {
  int threads = 256;
  for (;; threads >>= 1) {
    *lds = sizeof(float) * ((size_t)image_floats + 2 * (size_t)cnf_max_width(sh) * threads) +
           sizeof(double) * (size_t)cnf_table_doubles(sh);
    if (*lds <= 64 * 1024 || threads <= 64 || threads <= min_threads) break;
  }
  return threads;
}

template <int G>
static int launch_cnf(const float* y, const float* logp, const float* image, float* out, float* out1, float* evals,
                      int64_t n, const CnfShape& sh, int image_floats, bool integrate, float t_host, const float* t_dev,
                      double t0, double t1, int steps, int method, hipStream_t s) {
  size_t lds;
  const int threads = cnf_threads(sh, image_floats, G, &lds);
  if (lds > (size_t)kCnfLdsLimit) return hipErrorInvalidConfiguration;
  static PerDeviceOnce once_field, once_integrate;
  const hipError_t e =
      integrate ? ensure_max_dynamic_lds(once_integrate, reinterpret_cast<const void*>(&cnf_integrate_kernel<G>),
                                         kCnfLdsLimit)
                : ensure_max_dynamic_lds(once_field, reinterpret_cast<const void*>(&cnf_field_kernel<G>), kCnfLdsLimit);
  if (e != hipSuccess) return e;
  const int rows = threads / G;
  int64_t grid = (n + rows - 1) / rows;
  if (grid > kCnfMaxBlocks) grid = kCnfMaxBlocks;
  const int table = cnf_table_doubles(sh);
  if (integrate)
    hipLaunchKernelGGL((cnf_integrate_kernel<G>), dim3((unsigned)grid), dim3(threads), lds, s, y, logp, image, out,
                       out1, evals, n, sh, image_floats, table, t0, t1, steps, method);
  else
    hipLaunchKernelGGL((cnf_field_kernel<G>), dim3((unsigned)grid), dim3(threads), lds, s, y, image, out, out1, evals,
                       n, sh, image_floats, table, t_host, t_dev);
  return hipGetLastError();
}

static int dispatch_cnf(const float* y, const float* logp, const float* image, float* out, float* out1, float* evals,
                        int64_t n, const CnfShape& sh, int image_floats, bool integrate, float t_host,
                        const float* t_dev, double t0, double t1, int steps, int method, hipStream_t s) {
#define FC_CNF_GO(G) \
  return launch_cnf<G>(y, logp, image, out, out1, evals, n, sh, image_floats, integrate, t_host, t_dev, t0, t1, steps, \
                       method, s)
  if (sh.d < 2) FC_CNF_GO(2);
  if (sh.d < 4) FC_CNF_GO(4);
  if (sh.d < 8) FC_CNF_GO(8);
  if (sh.d < 16) FC_CNF_GO(16);
  FC_CNF_GO(32);
#undef FC_CNF_GO
}

// ---- training: one evaluation as an autograd node -----------------------------------------------------------------------
//
// fc_cnf_field_train is the forward: without a noise row it IS cnf_field_kernel (the exact divergence); with one, a row
// is a group of 2 lanes, the value stream and one tangent stream seeded with e, and div = scale e^T (J e)
// (Hutchinson's estimate).  Both run cnf_net.
//
// fc_cnf_field_backward recomputes the forward and walks the layers back.  S tangent streams, a_l the value
// stream's pre-activation, m_{l,s} a tangent's gated product, u_{l,s} = act'(a_l) m_{l,s}:
//     o_bar <- act'(a) h_bar + sum_s act''(a) m_s u_bar_s,   J_bar_s <- act'(a) u_bar_s          through the activation
//     W_bar += g (o_bar h^T + sum_s J_bar_s u_s^T),  b_bar = g o_bar,  w_t_bar = t b_bar,  w_b_bar = t o_bar
//     g_bar = o_bar (W h + c) + sum_s J_bar_s (W u_s),  b_g_bar = g_bar g (1 - g),  w_g_bar = t b_g_bar
//     h_bar = W^T (g o_bar),  u_bar_s = W^T (g J_bar_s)
// The lanes are the forward's (lane 0 the value stream, lane s the tangent s), so that the second-order term is one
// sum over the group and, with ab the adjoint a lane holds (o_bar or J_bar_s) and x its stored input (h or u_s), the
// weight gradient is one sum over ALL lanes of a block: W_bar[k][o] = g[o] sum_lanes ab[o] x[k].
//
// LDS per lane: the stored inputs of every layer (slot l, w[l] floats: what cnf_net rounds to float32, so the
// recomputed pre-activations are the forward's unrounded float64 ones), a slot of d floats for the seeds, and one
// of the widest layer for the gate products.  An adjoint overwrites the slot it belongs to once the layer above has
// consumed the input in it: slot l + 1 holds ab of layer l, slot l receives h_bar / u_bar.
//
// The sums over rows: inside a block every entry of the gradient image is owned by one thread that adds the lanes in
// a fixed (rotated, bank-conflict-free) order in float64 and accumulates its tiles in the block's float64 partial
// image in global memory; cnf_backward_sum_kernel adds the blocks' partials in block order and rounds once.  No
// atomics: bitwise reproducible.  scale_output multiplies the results, not the seeds.

// first and second derivative of the activation, in float64 (what torch's double backward gives)
__device__ __forceinline__ void cnf_act2(int act, double x, double p0, double& df, double& d2f) {
  switch (act) {
    case FC_CNF_ACT_TANH: {
      const double th = tanh(x);
      df = 1.0 - th * th;
      d2f = -2.0 * th * df;
      break;
    }
    case FC_CNF_ACT_RELU:
      df = x > 0.0 ? 1.0 : 0.0;
      d2f = 0.0;
      break;
    case FC_CNF_ACT_SOFTPLUS: {
      const double sg = 1.0 / (1.0 + exp(-x));
      df = x > 20.0 ? 1.0 : sg;
      d2f = x > 20.0 ? 0.0 : sg * (1.0 - sg);
      break;
    }
    case FC_CNF_ACT_ELU:
      df = x > 0.0 ? 1.0 : p0 * exp(x);
      d2f = x > 0.0 ? 0.0 : p0 * exp(x);
      break;
    case FC_CNF_ACT_SWISH: {
      const double sg = 1.0 / (1.0 + exp(-x));
      const double ds = sg * (1.0 - sg);
      df = sg + x * ds;
      d2f = ds * (2.0 + x * (1.0 - 2.0 * sg));
      break;
    }
    case FC_CNF_ACT_SQUARE:
      df = 2.0 * x;
      d2f = 2.0;
      break;
    default:
      df = 1.0;
      d2f = 0.0;
      break;
  }
}

template <int DP>
__global__ __launch_bounds__(256) void cnf_field_hutchinson_kernel(
    const float* __restrict__ y, const float* __restrict__ e, const float* __restrict__ image, float* __restrict__ dy,
    float* __restrict__ negdiv, float* __restrict__ evals, int64_t n, CnfShape sh, int image_floats, int table_doubles,
    float t_host, const float* __restrict__ t_dev) {
  constexpr int G = 2;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* img = lds;
  double* tab = reinterpret_cast<double*>(lds + image_floats);
  float* st = lds + image_floats + 2 * table_doubles;
  const int T = blockDim.x, tid = threadIdx.x;
  for (int i = tid; i < image_floats; i += T) img[i] = image[i];
  __syncthreads();
  cnf_time_table(img, tab, sh, t_dev ? (double)t_dev[0] : (double)t_host, tid, T);
  __syncthreads();
  const int d = sh.d, s = tid % G, rows_per_block = T / G, half = cnf_max_width(sh) * T;
  const int64_t tiles = (n + rows_per_block - 1) / rows_per_block;
  float* mine = st + tid;
  if (evals && blockIdx.x == 0 && tid == 0) atomicAdd(evals, 1.f);

  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    int64_t row = tile * rows_per_block + tid / G;
    const bool live = row < n;
    if (!live) row = n - 1;
    float xin[DP], ein[DP];
#pragma unroll
    for (int i = 0; i < DP; ++i) {
      xin[i] = i < d ? y[row * d + i] : 0.f;
      ein[i] = i < d ? e[row * d + i] : 0.f;
      if (i < d) mine[i * T] = s == 0 ? xin[i] : ein[i];
    }
    double k[DP];
    cnf_net<G, DP>(img, CnfBlockTime{tab}, mine, T, half, sh, s, k);
    double dot = 0.0;  // e^T (J e), in the tangent lane
#pragma unroll
    for (int i = 0; i < DP; ++i)
      if (s == 1 && i < d) dot += (double)ein[i] * k[i];
    dot += __shfl_xor(dot, 1, G);
    double div = dot * sh.scale;
    if (sh.residual) div -= (double)d;
    if (s == 0 && live) {
#pragma unroll
      for (int i = 0; i < DP; ++i) {
        if (i < d) {
          double v = k[i] * sh.scale;
          if (sh.residual) v -= (double)xin[i];
          dy[row * d + i] = (float)v;
        }
      }
      negdiv[row] = (float)(-div);
    }
  }
}

// sum[c] = (value ? b + w_t t : 0) + sum_k W[o + c][k] x[k], as cnf_net adds it
__device__ __forceinline__ void cnf_sum4(const float* wt, const double* q, const float* x, int T, int in, int op,
                                         int o, bool value, double (&sum)[4]) {
#pragma unroll
  for (int c = 0; c < 4; ++c) sum[c] = value ? q[o + c] : 0.0;
  for (int k = 0; k < in; ++k) {
    const double v = (double)x[k * T];
    const float4 w4 = *reinterpret_cast<const float4*>(wt + k * op + o);
    sum[0] = fma((double)w4.x, v, sum[0]);
    sum[1] = fma((double)w4.y, v, sum[1]);
    sum[2] = fma((double)w4.z, v, sum[2]);
    sum[3] = fma((double)w4.w, v, sum[3]);
  }
}

__host__ __device__ inline int cnf_out_max_width(const CnfShape& sh) {
  int m = sh.d;
  for (int l = 1; l < sh.layers; ++l) m = sh.w[l] > m ? sh.w[l] : m;
  return m;
}

// floats of LDS a lane of the backward kernel owns: the inputs of every layer, the seeds, the gate products
__host__ __device__ inline int cnf_backward_lane_floats(const CnfShape& sh) {
  int total = 0;
  for (int l = 0; l < sh.layers; ++l) total += sh.w[l];
  return total + sh.d + cnf_out_max_width(sh);
}

template <int G>
__global__ __launch_bounds__(256) void cnf_backward_kernel(
    const float* __restrict__ y, const float* __restrict__ e, const float* __restrict__ image,
    const float* __restrict__ g_dy, const float* __restrict__ g_negdiv, float* __restrict__ g_y,
    double* __restrict__ partial, int64_t n, CnfShape sh, int image_floats, int table_doubles, int lane_floats,
    float t_host, const float* __restrict__ t_dev) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* img = lds;
  double* tab = reinterpret_cast<double*>(lds + image_floats);
  float* st = lds + image_floats + 2 * table_doubles;
  const int T = blockDim.x, tid = threadIdx.x;
  for (int i = tid; i < image_floats; i += T) img[i] = image[i];
  __syncthreads();
  const double t = t_dev ? (double)t_dev[0] : (double)t_host;
  cnf_time_table(img, tab, sh, t, tid, T);
  __syncthreads();
  const int d = sh.d, s = tid % G, rows_per_block = T / G;
  const bool value = s == 0;
  const int64_t tiles = (n + rows_per_block - 1) / rows_per_block;
  float* mine = st + tid;
  const int gate_slot = lane_floats - cnf_out_max_width(sh);
  double* mypart = partial + (size_t)blockIdx.x * (size_t)image_floats;
  bool first = true;

  // the trip count depends on the block alone, so every thread meets the barriers below
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    int64_t row = tile * rows_per_block + tid / G;
    const bool live = row < n;
    if (!live) row = n - 1;  // runs along for the shuffles and the barriers, with zero seeds

    // forward: the inputs of every layer, rounded where cnf_net rounds them
    for (int i = 0; i < d; ++i)
      mine[i * T] = value ? y[row * d + i] : (e ? e[row * d + i] : (i == s - 1 ? 1.f : 0.f));
    int off = 0;
    const float* p = img;
    const double* q = tab;
    for (int l = 0; l + 1 < sh.layers; ++l) {
      const int in = sh.w[l], width = sh.w[l + 1], op = cnf_pad4(width);
      const float* wt = p + 5 * op;
      const float* cur = mine + off * T;
      float* nxt = mine + (off + in) * T;
      for (int o = 0; o < op; o += 4) {
        double sum[4];
        cnf_sum4(wt, q, cur, T, in, op, o, value, sum);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          double lin = sum[c] * q[op + o + c];
          if (value) lin += q[2 * op + o + c];
          const double pre = __shfl(lin, 0, G);
          if (o + c < width) {
            double f, df;
            cnf_act(sh.act, pre, sh.p0, f, df);
            nxt[(o + c) * T] = (float)(value ? f : df * lin);
          }
        }
      }
      off += in;
      p = wt + in * op;
      q += 3 * op;
    }

    // seeds, in the slot above the last layer's input
    {
      float* seed = mine + (off + sh.w[sh.layers - 1]) * T;
      const float gn = live ? g_negdiv[row] : 0.f;
      for (int i = 0; i < d; ++i) {
        float v = 0.f;
        if (live) v = value ? g_dy[row * d + i] : -gn * (e ? e[row * d + i] : (i == s - 1 ? 1.f : 0.f));
        seed[i * T] = v;
      }
    }

    for (int l = sh.layers - 1; l >= 0; --l) {
      const bool last = l == sh.layers - 1;
      const int in = sh.w[l], width = sh.w[l + 1], op = cnf_pad4(width);
      const float* wt = p + 5 * op;
      float* x = mine + off * T;           // this lane's input of the layer
      float* adj = mine + (off + in) * T;  // in: the adjoint of the layer's activated output; out: ab
      float* gp = mine + gate_slot * T;    // ab * (W x + c): the gate's share of this lane

      for (int o = 0; o < op; o += 4) {
        double sum[4];
        cnf_sum4(wt, q, x, T, in, op, o, value, sum);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const bool real = o + c < width;
          double lin = sum[c] * q[op + o + c];
          if (value) lin += q[2 * op + o + c];
          const double pre = __shfl(lin, 0, G);
          const double xb = real ? (double)adj[(o + c) * T] : 0.0;
          double ab = xb;
          if (!last) {
            double df, d2f;
            cnf_act2(sh.act, pre, sh.p0, df, d2f);
            double cross = value ? 0.0 : d2f * lin * xb;
#pragma unroll
            for (int step = G / 2; step > 0; step >>= 1) cross += __shfl_xor(cross, step, G);
            ab = df * xb;
            if (value) ab += cross;
          }
          if (real) {
            adj[(o + c) * T] = (float)ab;
            if (sh.gated) gp[(o + c) * T] = (float)(ab * sum[c]);
          }
        }
      }
      __syncthreads();

      // the block's sums over its lanes, into its partial image
      {
        const float* xs = st + off * T;
        const float* as = st + (off + in) * T;
        const float* gs = st + gate_slot * T;
        double* pl = mypart + (p - img);
        const int ot = op / 4, kt = (in + 3) / 4;
        for (int tl = tid; tl < ot * kt; tl += T) {
          const int o0 = 4 * (tl % ot), k0 = 4 * (tl / ot);
          int oi[4], ki[4];
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            oi[c] = (o0 + c < width ? o0 + c : width - 1) * T;
            ki[c] = (k0 + c < in ? k0 + c : in - 1) * T;
          }
          double acc[4][4];
#pragma unroll
          for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int c = 0; c < 4; ++c) acc[r][c] = 0.0;
          for (int j = 0; j < T; ++j) {
            const int lane = (j + tid) & (T - 1);
            double a[4], v[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
              a[c] = (double)as[oi[c] + lane];
              v[c] = (double)xs[ki[c] + lane];
            }
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
              for (int c = 0; c < 4; ++c) acc[r][c] = fma(v[r], a[c], acc[r][c]);
          }
#pragma unroll
          for (int r = 0; r < 4; ++r) {
#pragma unroll
            for (int c = 0; c < 4; ++c) {
              if (k0 + r < in) {
                const int at = 5 * op + (k0 + r) * op + o0 + c;
                const double val = o0 + c < width ? acc[r][c] * q[op + o0 + c] : 0.0;
                pl[at] = first ? val : pl[at] + val;
              }
            }
          }
        }
        for (int o = tid; o < op; o += T) {
          double s1 = 0.0, s2 = 0.0;
          if (o < width) {
            for (int j = 0; j < T; ++j) {
              const int lane = (j + tid) & (T - 1);
              if (lane % G == 0) s1 += (double)as[o * T + lane];
              if (sh.gated) s2 += (double)gs[o * T + lane];
            }
          }
          const double g = q[op + o];
          const double vb = s1 * g, vg = sh.gated ? s2 * g * (1.0 - g) : 0.0;
          const double out5[5] = {vb, t * vb, t * vg, vg, t * s1};
#pragma unroll
          for (int c = 0; c < 5; ++c) pl[c * op + o] = first ? out5[c] : pl[c * op + o] + out5[c];
        }
      }
      __syncthreads();

      // down through W: the adjoint of this lane's input, into the input's slot (the value lane's g_y at the bottom)
      if (l > 0 || value) {
        for (int k0 = 0; k0 < in; k0 += 4) {
          double acc[4] = {0.0, 0.0, 0.0, 0.0};
          for (int o = 0; o < op; o += 4) {
            double dg[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) dg[c] = o + c < width ? (double)adj[(o + c) * T] * q[op + o + c] : 0.0;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int k = k0 + r < in ? k0 + r : in - 1;
              const float4 w4 = *reinterpret_cast<const float4*>(wt + k * op + o);
              acc[r] = fma((double)w4.x, dg[0], acc[r]);
              acc[r] = fma((double)w4.y, dg[1], acc[r]);
              acc[r] = fma((double)w4.z, dg[2], acc[r]);
              acc[r] = fma((double)w4.w, dg[3], acc[r]);
            }
          }
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            if (k0 + r < in) {
              if (l > 0) {
                x[(k0 + r) * T] = (float)acc[r];
              } else if (live) {
                double v = acc[r] * sh.scale;
                if (sh.residual) v -= (double)g_dy[row * d + k0 + r];
                g_y[row * d + k0 + r] = (float)v;
              }
            }
          }
        }
      }
      if (l > 0) {
        const int below = sh.w[l - 1];
        p -= (5 + below) * cnf_pad4(in);
        q -= 3 * cnf_pad4(in);
        off -= below;
      }
    }
    first = false;
  }
}

// g_image[i] = scale * (the blocks' partials in block order)
__global__ __launch_bounds__(256) void cnf_backward_sum_kernel(const double* __restrict__ partial,
                                                               float* __restrict__ g_image, int blocks,
                                                               int image_floats, double scale) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= image_floats) return;
  double sum = 0.0;
  for (int b = 0; b < blocks; ++b) sum += partial[(size_t)b * (size_t)image_floats + i];
  g_image[i] = (float)(sum * scale);
}

constexpr int kCnfBackwardMaxBlocks = 256;

template <int DP>
static int launch_cnf_hutchinson(const float* y, const float* e, const float* image, float* dy, float* negdiv,
                                 float* evals, int64_t n, const CnfShape& sh, int image_floats, float t_host,
                                 const float* t_dev, hipStream_t s) {
  size_t lds;
  const int threads = cnf_threads(sh, image_floats, 2, &lds);
  if (lds > (size_t)kCnfLdsLimit) return hipErrorInvalidConfiguration;
  static PerDeviceOnce once;
  const hipError_t err =
      ensure_max_dynamic_lds(once, reinterpret_cast<const void*>(&cnf_field_hutchinson_kernel<DP>), kCnfLdsLimit);
  if (err != hipSuccess) return err;
  const int rows = threads / 2;
  int64_t grid = (n + rows - 1) / rows;
  if (grid > kCnfMaxBlocks) grid = kCnfMaxBlocks;
  hipLaunchKernelGGL((cnf_field_hutchinson_kernel<DP>), dim3((unsigned)grid), dim3(threads), lds, s, y, e, image, dy,
                     negdiv, evals, n, sh, image_floats, cnf_table_doubles(sh), t_host, t_dev);
  return hipGetLastError();
}

static int cnf_backward_group(const CnfShape& sh, bool with_e) {
  if (with_e || sh.d < 2) return 2;
  return sh.d < 4 ? 4 : sh.d < 8 ? 8 : sh.d < 16 ? 16 : 32;
}

// the largest block (256, 128, 64 threads) whose image + table + lanes fit; 0 when 64 threads do not
static int cnf_backward_threads(const CnfShape& sh, int image_floats, size_t* lds) {
  for (int threads = 256; threads >= 64; threads >>= 1) {
    *lds = sizeof(float) * ((size_t)image_floats + (size_t)cnf_backward_lane_floats(sh) * threads) +
           sizeof(double) * (size_t)cnf_table_doubles(sh);
    if (*lds <= (size_t)kCnfLdsLimit) return threads;
  }
  return 0;
}

static int64_t cnf_backward_blocks(const CnfShape& sh, int image_floats, bool with_e, int64_t n, int* threads,
                                   size_t* lds) {
  *threads = cnf_backward_threads(sh, image_floats, lds);
  if (!*threads) return 0;
  const int rows = *threads / cnf_backward_group(sh, with_e);
  const int64_t tiles = (n + rows - 1) / rows;
  return tiles < kCnfBackwardMaxBlocks ? tiles : kCnfBackwardMaxBlocks;
}

template <int G>
static int launch_cnf_backward(const float* y, const float* e, const float* image, const float* g_dy,
                               const float* g_negdiv, float* g_y, float* g_image, double* partial, int64_t n,
                               const CnfShape& sh, int image_floats, float t_host, const float* t_dev, hipStream_t s) {
  int threads;
  size_t lds;
  const int64_t grid = cnf_backward_blocks(sh, image_floats, e != nullptr, n, &threads, &lds);
  if (grid < 1) return hipErrorInvalidConfiguration;
  static PerDeviceOnce once;
  const hipError_t err =
      ensure_max_dynamic_lds(once, reinterpret_cast<const void*>(&cnf_backward_kernel<G>), kCnfLdsLimit);
  if (err != hipSuccess) return err;
  hipLaunchKernelGGL((cnf_backward_kernel<G>), dim3((unsigned)grid), dim3(threads), lds, s, y, e, image, g_dy,
                     g_negdiv, g_y, partial, n, sh, image_floats, cnf_table_doubles(sh), cnf_backward_lane_floats(sh),
                     t_host, t_dev);
  hipError_t launched = hipGetLastError();
  if (launched != hipSuccess) return launched;
  hipLaunchKernelGGL(cnf_backward_sum_kernel, dim3((unsigned)((image_floats + 255) / 256)), dim3(256), 0, s, partial,
                     g_image, (int)grid, image_floats, sh.scale);
  return hipGetLastError();
}

static bool cnf_train_shape(int d, int layers, const int32_t* hidden, int kind, int act, int residual, float scale,
                            float p0, int image_floats, CnfShape* sh) {
  return layers <= FC_CNF_TRAIN_MAX_HIDDEN_LAYERS + 1 &&
         cnf_shape(d, layers, hidden, kind, act, residual, scale, p0, image_floats, sh);
}

}  // namespace fc

extern "C" int fc_cnf_field_train(const float* y, const float* e, const float* image, float* dy, float* negdiv,
                                  float* evals, int64_t n, int32_t d, int32_t layers, const int32_t* hidden,
                                  int32_t layer_kind, int32_t activation, int32_t residual, float scale_output,
                                  float p0, int32_t image_floats, float t, const float* t_dev, void* stream) {
  fc::CnfShape sh;
  if (n < 0 || !fc::cnf_train_shape(d, layers, hidden, layer_kind, activation, residual, scale_output, p0, image_floats,
                                    &sh))
    return hipErrorInvalidValue;
  if (n == 0) return hipSuccess;
  if (!y || !image || !dy || !negdiv || y == dy) return hipErrorInvalidValue;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (!e)
    return fc::dispatch_cnf(y, nullptr, image, dy, negdiv, evals, n, sh, image_floats, false, t, t_dev, 0.0, 0.0, 0, 0,
                            s);
  if (d <= 4) return fc::launch_cnf_hutchinson<4>(y, e, image, dy, negdiv, evals, n, sh, image_floats, t, t_dev, s);
  if (d <= 8) return fc::launch_cnf_hutchinson<8>(y, e, image, dy, negdiv, evals, n, sh, image_floats, t, t_dev, s);
  return fc::launch_cnf_hutchinson<16>(y, e, image, dy, negdiv, evals, n, sh, image_floats, t, t_dev, s);
}

extern "C" int fc_cnf_field_backward_rows(int32_t d, int32_t layers, const int32_t* hidden, int32_t with_e) {
  fc::CnfShape sh;
  if (d < 1 || d > FC_CNF_MAX_DIM || layers < 1 || layers > FC_CNF_TRAIN_MAX_HIDDEN_LAYERS + 1) return -1;
  if (layers > 1 && !hidden) return -1;
  int floats = 0, below = d;
  for (int l = 1; l <= layers; ++l) {
    const int width = l < layers ? hidden[l - 1] : d;
    floats += (5 + below) * fc::cnf_pad4(width);
    below = width;
  }
  if (!fc::cnf_train_shape(d, layers, hidden, 0, 0, 0, 1.f, 1.f, floats, &sh)) return -1;
  size_t lds;
  const int threads = fc::cnf_backward_threads(sh, floats, &lds);
  return threads ? threads / fc::cnf_backward_group(sh, with_e != 0) : -1;
}

extern "C" int fc_cnf_field_backward_workspace(int64_t n, int32_t d, int32_t layers, const int32_t* hidden,
                                               int32_t with_e) {
  const int rows = fc_cnf_field_backward_rows(d, layers, hidden, with_e);
  if (rows < 1 || n < 0) return -1;
  int64_t blocks = (n + rows - 1) / rows;
  if (blocks > fc::kCnfBackwardMaxBlocks) blocks = fc::kCnfBackwardMaxBlocks;
  int floats = 0, below = d;
  for (int l = 1; l <= layers; ++l) {
    const int width = l < layers ? hidden[l - 1] : d;
    floats += (5 + below) * fc::cnf_pad4(width);
    below = width;
  }
  return (int)(2 * blocks * floats);
}

extern "C" int fc_cnf_field_backward(const float* y, const float* e, const float* image, const float* g_dy,
                                     const float* g_negdiv, float* g_y, float* g_image, void* workspace, int64_t n,
                                     int32_t d, int32_t layers, const int32_t* hidden, int32_t layer_kind,
                                     int32_t activation, int32_t residual, float scale_output, float p0,
                                     int32_t image_floats, float t, const float* t_dev, void* stream) {
  fc::CnfShape sh;
  if (n < 0 || !fc::cnf_train_shape(d, layers, hidden, layer_kind, activation, residual, scale_output, p0, image_floats,
                                    &sh))
    return hipErrorInvalidValue;
  if (!g_image) return hipErrorInvalidValue;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (n == 0) return hipMemsetAsync(g_image, 0, sizeof(float) * (size_t)image_floats, s);
  if (!y || !image || !g_dy || !g_negdiv || !g_y || !workspace || (reinterpret_cast<uintptr_t>(workspace) & 7))
    return hipErrorInvalidValue;
  double* partial = static_cast<double*>(workspace);
#define FC_CNF_BACK(G) \
  return fc::launch_cnf_backward<G>(y, e, image, g_dy, g_negdiv, g_y, g_image, partial, n, sh, image_floats, t, t_dev, s)
  switch (fc::cnf_backward_group(sh, e != nullptr)) {
    case 2: FC_CNF_BACK(2);
    case 4: FC_CNF_BACK(4);
    case 8: FC_CNF_BACK(8);
    case 16: FC_CNF_BACK(16);
    default: FC_CNF_BACK(32);
  }
#undef FC_CNF_BACK
}

extern "C" int fc_cnf_field(const float* y, const float* image, float* dy, float* negdiv, float* evals, int64_t n,
                            int32_t d, int32_t layers, const int32_t* hidden, int32_t layer_kind, int32_t activation,
                            int32_t residual, float scale_output, float p0, int32_t image_floats, float t,
                            const float* t_dev, void* stream) {
  fc::CnfShape sh;
  if (n < 0 || !fc::cnf_shape(d, layers, hidden, layer_kind, activation, residual, scale_output, p0, image_floats, &sh))
    return hipErrorInvalidValue;
  if (n == 0) return hipSuccess;
  if (!y || !image || !dy || !negdiv || y == dy) return hipErrorInvalidValue;
  return fc::dispatch_cnf(y, nullptr, image, dy, negdiv, evals, n, sh, image_floats, false, t, t_dev, 0.0, 0.0, 0, 0,
                          static_cast<hipStream_t>(stream));
}

extern "C" int fc_cnf_integrate(const float* z, const float* logp, const float* image, float* z_out, float* logp_out,
                                float* evals, int64_t n, int32_t d, int32_t layers, const int32_t* hidden,
                                int32_t layer_kind, int32_t activation, int32_t residual, float scale_output, float p0,
                                int32_t image_floats, double t0, double t1, int32_t steps, int32_t method,
                                void* stream) {
  fc::CnfShape sh;
  if (n < 0 || steps < 1 || method < FC_CNF_EULER || method > FC_CNF_RK4 || !(t0 == t0) || !(t1 == t1))
    return hipErrorInvalidValue;
  if (!fc::cnf_shape(d, layers, hidden, layer_kind, activation, residual, scale_output, p0, image_floats, &sh))
    return hipErrorInvalidValue;
  if (n == 0) return hipSuccess;
  if (!z || !image || !z_out || !logp_out || z == z_out) return hipErrorInvalidValue;
  return fc::dispatch_cnf(z, logp, image, z_out, logp_out, evals, n, sh, image_floats, true, 0.f, nullptr, t0, t1,
                          steps, method, static_cast<hipStream_t>(stream));
}
