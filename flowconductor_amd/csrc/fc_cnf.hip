// Continuous normalizing flows (reference flowcon/CNF/cnf.py with neural_odes/odefunc.py and
// neural_odes/diffeq_layers/basic.py).
//
//   fc_cnf_field       dy = f(t, y) and -div_y f(t, y) of an ODEnet over time-conditioned linear layers    one launch
//   fc_cnf_integrate   z(t1), logp(t1) from z(t0), logp(t0) under d/dt (z, logp) = (f, -div f) with a fixed-step
//                      Runge-Kutta method, every row on its own                                            one launch
//   fc_cnf_field_train / fc_cnf_field_backward   one evaluation as an autograd node: the exact divergence or
//                      Hutchinson's estimate, and the gradients of both outputs (further down)
//   fc_cnf_integrate_train / fc_cnf_integrate_backward   the whole fixed-step solve as an autograd node: the solve with
//                      a tape of its stage inputs, and the reverse sweep over that tape            one launch each
// (fc_cnf_dopri5, the adaptive solve with per-row step control, is in fc_cnf_dopri5.hip; what the CNF kernels share --
// CnfShape, the activations, cnf_time_table, cnf_hidden_layers, cnf_net and cnf_field_row -- is in fc_cnf.h.  The block
// set-up (GroupBlock), the weight sums and the launch plan are the lane-group scaffold's, fc_lane_group.h, which the
// iResBlock kernels use too; the sum over the blocks' partials is fc_partial_sum.h.)
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
// Numerics: sums in float64 over the float32 weights, a stored activation rounded to float32 once (cnf_hidden_layers
// is the one place that decides this); the integrator keeps (z, logp) and the stage slopes in float64 registers and
// rounds a stage's state to float32 where it enters the net.
#include "fc_cnf.h"
#include "fc_partial_sum.h"

namespace fc {

// ---- one evaluation -------------------------------------------------------------------------------------------------

// Div = CnfExactDiv: the exact divergence, G lanes a row.  Div = CnfHutchinsonDiv<DP>: G = 2, the value stream and one
// tangent stream seeded with the row of e, div = scale e^T (J e).
template <int G, int DP, class Div>
__global__ __launch_bounds__(256) void cnf_field_kernel(const float* __restrict__ y, const float* __restrict__ e,
                                                        const float* __restrict__ image, float* __restrict__ dy,
                                                        float* __restrict__ negdiv, float* __restrict__ evals,
                                                        int64_t n, CnfShape sh, int image_floats, int table_doubles,
                                                        float t_host, const float* __restrict__ t_dev) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const CnfBlock b = cnf_block<G>(lds, image, image_floats, table_doubles, 0, n, sh);
  __syncthreads();
  cnf_time_table(b.img, b.mid, sh, t_dev ? (double)t_dev[0] : (double)t_host, b.tid, b.T);
  __syncthreads();
  const int d = sh.d;
  if (evals && blockIdx.x == 0 && b.tid == 0) atomicAdd(evals, 1.f);

  for (int64_t tile = blockIdx.x; tile < b.tiles; tile += gridDim.x) {
    bool live;
    const int64_t row = tile_row(b, tile, n, live);
    float xin[DP];
#pragma unroll
    for (int i = 0; i < DP; ++i) xin[i] = i < d ? y[row * d + i] : 0.f;
    Div dv;
    dv.load(e, row, d);
    double k[DP], nd;
    cnf_field_row<G, DP>(b.img, CnfBlockTime{b.mid}, dv, b.mine, b.T, b.half, sh, b.s, xin, k, nd);
    if (b.s == 0 && live) {
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

// Div as in cnf_field_kernel, with one row of e for the whole solve.  Tape: the float32 state every stage hands to the
// net is kept as tape[step * stages + stage][row][:], which is all fc_cnf_integrate_backward needs of the forward.
// fc_cnf_integrate is the instance <G, LaneGroup<G>::DP, CnfExactDiv, false>.
template <int G, int DP, class Div, bool Tape>
__global__ __launch_bounds__(256) void cnf_integrate_kernel(const float* __restrict__ z, const float* __restrict__ logp,
                                                            const float* __restrict__ e,
                                                            const float* __restrict__ image, float* __restrict__ z_out,
                                                            float* __restrict__ logp_out, float* __restrict__ tape,
                                                            float* __restrict__ evals, int64_t n, CnfShape sh,
                                                            int image_floats, int table_doubles, double t0, double t1,
                                                            int steps, int method) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const CnfBlock b = cnf_block<G>(lds, image, image_floats, table_doubles, 0, n, sh);
  const int d = sh.d;
  const int stages = cnf_stages(method);
  const double h = (t1 - t0) / (double)steps;
  bool have_table = false;
  double table_t = 0.0;
  if (evals && blockIdx.x == 0 && b.tid == 0)  // non-negative floats order like their bit patterns
    atomicMax(reinterpret_cast<int*>(evals), __float_as_int((float)steps * (float)stages));

  // the tile loop's trip count depends on the block alone, so the barriers below are met by every thread
  for (int64_t tile = blockIdx.x; tile < b.tiles; tile += gridDim.x) {
    bool live;
    const int64_t row = tile_row(b, tile, n, live);
    double yv[DP], acc[DP], k[DP];
#pragma unroll
    for (int i = 0; i < DP; ++i) {
      yv[i] = i < d ? (double)z[row * d + i] : 0.0;
      k[i] = 0.0;
    }
    double lp = logp ? (double)logp[row] : 0.0, lk = 0.0, lacc;
    Div dv;
    dv.load(e, row, d);
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
          cnf_time_table(b.img, b.mid, sh, tt, b.tid, b.T);
          __syncthreads();
          have_table = true;
          table_t = tt;
        }
        float xin[DP];
        const double ah = node * h;
#pragma unroll
        for (int i = 0; i < DP; ++i) xin[i] = (float)(stage == 0 ? yv[i] : yv[i] + ah * k[i]);
        if (Tape && b.s == 0 && live) {
          float* slot = tape + (((size_t)step * (size_t)stages + (size_t)stage) * (size_t)n + (size_t)row) * (size_t)d;
#pragma unroll
          for (int i = 0; i < DP; ++i)
            if (i < d) slot[i] = xin[i];
        }
        cnf_field_row<G, DP>(b.img, CnfBlockTime{b.mid}, dv, b.mine, b.T, b.half, sh, b.s, xin, k, lk);
#pragma unroll
        for (int i = 0; i < DP; ++i) acc[i] += weight * k[i];
        lacc += weight * lk;
      }
#pragma unroll
      for (int i = 0; i < DP; ++i) yv[i] += h * acc[i];
      lp += h * lacc;
    }
    if (b.s == 0 && live) {
#pragma unroll
      for (int i = 0; i < DP; ++i)
        if (i < d) z_out[row * d + i] = (float)yv[i];
      logp_out[row] = (float)lp;
    }
  }
}

// ---- training: one evaluation as an autograd node -----------------------------------------------------------------------
//
// fc_cnf_field_train is the forward: cnf_field_kernel, without a noise row with the exact divergence, with one with
// Hutchinson's estimate.
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
// LDS per lane: the stored inputs of every layer (slot l, w[l] floats: cnf_hidden_layers itself writes them, CnfStacked
// in place of the forward's ping-pong, so the recomputed pre-activations are the forward's unrounded float64 ones), a
// slot of d floats for the seeds, and one of the widest layer for the gate products.  An adjoint overwrites the slot
// it belongs to once the layer above has consumed the input in it: slot l + 1 holds ab of layer l, slot l receives
// h_bar / u_bar.
//
// The sums over rows: inside a block every entry of the gradient image is owned by one thread that adds the lanes in
// a fixed (rotated, bank-conflict-free) order in float64 and accumulates its tiles in the block's float64 partial
// image in global memory; partial_sum_kernel (fc_partial_sum.h) adds the blocks' partials in block order and rounds
// once.  No atomics: bitwise reproducible.  scale_output multiplies the results, not the seeds.

// floats of LDS a lane of the backward kernel owns: the inputs of every layer, the seeds, the gate products
__host__ __device__ inline int cnf_backward_lane_floats(const CnfShape& sh) {
  int total = 0;
  for (int l = 0; l < sh.layers; ++l) total += sh.w[l];
  return total + sh.d + cnf_max_width(sh);
}

// The backward of ONE evaluation at time t for the row of this lane's group, the block's time table standing at t:
// both backward kernels run it, once (cnf_backward_kernel) or once per stage of a solve (cnf_solve_backward_kernel).
// The caller has put this lane's input of the first layer into its slot 0 (the state, e or a unit vector).
//     seed(i)     this lane's adjoint of output i: of dy_i in the value lane, -(adjoint of negdiv) times its own seed
//                 of the forward in a tangent lane; zero for a row past the end
//     sink(k, v)  receives the adjoint of input k, in the value lane only, scale_output and residual folded in
// first: the block's partial image is overwritten, else added to.  Every thread of the block has to call it (barriers).
template <int G, class Seed, class Sink>
__device__ __forceinline__ void cnf_backward_walk(const CnfBlock& b, const CnfShape& sh, int lane_floats, double t,
                                                  double* mypart, bool first, Seed seed, Sink sink) {
  const float* img = b.img;
  float* st = b.st;
  float* mine = b.mine;
  const int T = b.T, tid = b.tid, d = sh.d;
  const bool value = b.s == 0;
  const int gate_slot = lane_floats - cnf_max_width(sh);
  // forward: the inputs of every layer, as the forward kernel computed and rounded them
  CnfBlockTime tm{b.mid};
  CnfStacked slots{mine, 0};
  const float* p = cnf_hidden_layers<G>(img, tm, slots, T, sh, value);
  int off = slots.off;
  const double* q = tm.q;

  // seeds, in the slot above the last layer's input; the last layer leaves them there
  float* seeds = mine + (off + sh.w[sh.layers - 1]) * T;
  for (int i = 0; i < d; ++i) seeds[i * T] = seed(i);

  for (int l = sh.layers - 1; l >= 0; --l) {
    const bool last = l == sh.layers - 1;
    const int in = sh.w[l], width = sh.w[l + 1], op = pad4(width);
    const float* wt = p + 5 * op;
    const CnfBlockTime here{q};          // the layer's time terms
    float* x = mine + off * T;           // this lane's input of the layer
    float* adj = mine + (off + in) * T;  // in: the adjoint of the layer's activated output; out: ab
    float* gp = mine + gate_slot * T;    // ab * (W x + c): the gate's share of this lane

    for (int o = 0; o < op; o += 4) {
      double sum[4];
      cnf_sum4(wt, here, p, x, T, in, op, o, value, sum);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const bool real = o + c < width;
        double lin, pre;
        cnf_lin_pre<G>(here, p, op, o + c, value, sum[c], lin, pre);
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

    // down through W: the adjoint of this lane's input, into the input's slot (the value lane's to the sink at the
    // bottom)
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
            } else {
              double v = acc[r] * sh.scale;
              if (sh.residual) v -= (double)seeds[(k0 + r) * T];
              sink(k0 + r, v);
            }
          }
        }
      }
    }
    if (l > 0) {
      const int below = sh.w[l - 1];
      p -= (5 + below) * pad4(in);
      q -= 3 * pad4(in);
      off -= below;
    }
  }
}

template <int G>
__global__ __launch_bounds__(256) void cnf_backward_kernel(
    const float* __restrict__ y, const float* __restrict__ e, const float* __restrict__ image,
    const float* __restrict__ g_dy, const float* __restrict__ g_negdiv, float* __restrict__ g_y,
    double* __restrict__ partial, int64_t n, CnfShape sh, int image_floats, int table_doubles, int lane_floats,
    float t_host, const float* __restrict__ t_dev) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const CnfBlock b = cnf_block<G>(lds, image, image_floats, table_doubles, 0, n, sh);
  __syncthreads();
  const double t = t_dev ? (double)t_dev[0] : (double)t_host;
  cnf_time_table(b.img, b.mid, sh, t, b.tid, b.T);
  __syncthreads();
  const int d = sh.d, s = b.s;
  const bool value = s == 0;
  double* mypart = partial + (size_t)blockIdx.x * (size_t)image_floats;
  bool first = true;

  // the trip count depends on the block alone, so every thread meets the barriers of the walk
  for (int64_t tile = blockIdx.x; tile < b.tiles; tile += gridDim.x) {
    bool live;  // a row past the end runs along with zero seeds
    const int64_t row = tile_row(b, tile, n, live);
    for (int i = 0; i < d; ++i)
      b.mine[i * b.T] = value ? y[row * d + i] : (e ? e[row * d + i] : (i == s - 1 ? 1.f : 0.f));
    const float gn = live ? g_negdiv[row] : 0.f;
    cnf_backward_walk<G>(
        b, sh, lane_floats, t, mypart, first,
        [&](int i) {
          float v = 0.f;
          if (live) v = value ? g_dy[row * d + i] : -gn * (e ? e[row * d + i] : (i == s - 1 ? 1.f : 0.f));
          return v;
        },
        [&](int k, double v) {
          if (live) g_y[row * d + k] = (float)v;
        });
    first = false;
  }
}

// ---- training: the whole fixed-step solve as an autograd node -------------------------------------------------------
//
// fc_cnf_integrate_train is cnf_integrate_kernel with a divergence policy and the tape.  fc_cnf_integrate_backward is
// the reverse sweep over the tape, the exact gradient of the solve that ran.  With ybar the adjoint of y_{n+1} and lbar
// the adjoint of logp (constant through the solve: logp never feeds f), for n = steps - 1 .. 0 and i = S - 1 .. 0:
//     seed_dy_i = h b_i ybar + (i + 1 < S ? a_{i+1} h Ybar_{i+1} : 0),   seed_negdiv_i = h b_i lbar
//     Ybar_i = cnf_backward_walk at (t_i, tape[n S + i]) with those seeds; the image's gradient accumulates
//     after stage 0:  ybar <- ybar + sum_i Ybar_i
// A seed is rounded to float32 where it enters the walk (as a stage state is where it enters the net).  ybar, the
// running sum and Ybar_{i+1} are float64: three [n, d] planes of the workspace behind the partial images, a row's
// entries touched by the value lane of its group alone.  Layout, LDS, grid cap and the sum over blocks are
// cnf_backward_kernel's; the table is rebuilt per stage behind barriers as in the integrator.
template <int G>
__global__ __launch_bounds__(256) void cnf_solve_backward_kernel(
    const float* __restrict__ tape, const float* __restrict__ e, const float* __restrict__ image,
    const float* __restrict__ g_z_out, const float* __restrict__ g_logp_out, float* __restrict__ g_z,
    double* __restrict__ partial, double* __restrict__ planes, int64_t n, CnfShape sh, int image_floats,
    int table_doubles, int lane_floats, double t0, double t1, int steps, int method) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const CnfBlock b = cnf_block<G>(lds, image, image_floats, table_doubles, 0, n, sh);
  const int d = sh.d, s = b.s;
  const bool value = s == 0;
  const int stages = cnf_stages(method);
  const double h = (t1 - t0) / (double)steps;
  const size_t plane = (size_t)n * (size_t)d;
  double* mypart = partial + (size_t)blockIdx.x * (size_t)image_floats;
  bool first = true, have_table = false;
  double table_t = 0.0;

  // the trip counts depend on the block alone, so every thread meets the barriers below and those of the walk
  for (int64_t tile = blockIdx.x; tile < b.tiles; tile += gridDim.x) {
    bool live;  // a row past the end runs along with zero seeds and touches no plane
    const int64_t row = tile_row(b, tile, n, live);
    const size_t at = (size_t)row * (size_t)d;
    double* ybar = planes + at;
    double* total = ybar + plane;
    double* above = total + plane;  // Ybar of the stage after this one
    const bool mine_to_keep = value && live;
    if (mine_to_keep) {
      for (int i = 0; i < d; ++i) {
        ybar[i] = (double)g_z_out[at + i];
        total[i] = 0.0;
      }
    }
    const double lbar = live ? (double)g_logp_out[row] : 0.0;
    for (int step = steps - 1; step >= 0; --step) {
      const double ts = t0 + (double)step * h;
      for (int stage = stages - 1; stage >= 0; --stage) {
        const double tt = ts + cnf_node(method, stage) * h;
        if (!have_table || tt != table_t) {
          __syncthreads();  // the image copy, and the readers of the previous table
          cnf_time_table(b.img, b.mid, sh, tt, b.tid, b.T);
          __syncthreads();
          have_table = true;
          table_t = tt;
        }
        const size_t slot = ((size_t)step * (size_t)stages + (size_t)stage) * (size_t)n + (size_t)row;
        const float* xin = tape + slot * (size_t)d;
        for (int i = 0; i < d; ++i) b.mine[i * b.T] = value ? xin[i] : (e ? e[at + i] : (i == s - 1 ? 1.f : 0.f));
        const double hb = h * cnf_weight(method, stage);
        const bool chained = stage + 1 < stages;
        const double ha = chained ? cnf_node(method, stage + 1) * h : 0.0;
        const float gn = (float)(hb * lbar);
        cnf_backward_walk<G>(
            b, sh, lane_floats, tt, mypart, first,
            [&](int i) {
              if (!live) return 0.f;
              if (!value) return -gn * (e ? e[at + i] : (i == s - 1 ? 1.f : 0.f));
              double v = hb * ybar[i];
              if (chained) v += ha * above[i];
              return (float)v;
            },
            [&](int k, double v) {
              if (live) {
                above[k] = v;
                total[k] += v;
              }
            });
        first = false;
      }
      if (mine_to_keep) {
        for (int i = 0; i < d; ++i) {
          ybar[i] += total[i];
          total[i] = 0.0;
        }
      }
    }
    if (mine_to_keep)
      for (int i = 0; i < d; ++i) g_z[at + i] = (float)ybar[i];
  }
}

// ---- launch ---------------------------------------------------------------------------------------------------------

constexpr int kCnfTrainMaxLayers = FC_CNF_TRAIN_MAX_HIDDEN_LAYERS + 1;

// the exact divergence by the group of d, Hutchinson's estimate (e) in 2 lanes by the padded d
static int launch_cnf_field(const float* y, const float* e, const float* image, float* dy, float* negdiv, float* evals,
                            int64_t n, const CnfShape& sh, int image_floats, float t_host, const float* t_dev,
                            hipStream_t s) {
  const int group = cnf_group(sh, e != nullptr), table = cnf_table_doubles(sh);
  const GroupLaunch plan = group_launch_plan(image_floats, group, cnf_forward_lds(sh), kPrefer64K, n, kGroupMaxBlocks);
  if (e)
    return with_constant<4, 8, 16>(sh.d <= 4 ? 4 : sh.d <= 8 ? 8 : 16, [&](auto dp) {
      constexpr int DP = decltype(dp)::value;
      return group_launch<&cnf_field_kernel<2, DP, CnfHutchinsonDiv<DP>>>(plan, s, y, e, image, dy, negdiv, evals, n, sh,
                                                                        image_floats, table, t_host, t_dev);
    });
  return with_constant<2, 4, 8, 16, 32>(group, [&](auto g) {
    constexpr int G = decltype(g)::value;
    return group_launch<&cnf_field_kernel<G, LaneGroup<G>::DP, CnfExactDiv>>(plan, s, y, e, image, dy, negdiv, evals, n,
                                                                          sh, image_floats, table, t_host, t_dev);
  });
}

template <int G, int DP, class Div, class... Args>
static int launch_cnf_integrate_as(bool tape, const GroupLaunch& plan, hipStream_t s, Args... args) {
  return tape ? group_launch<&cnf_integrate_kernel<G, DP, Div, true>>(plan, s, args...)
              : group_launch<&cnf_integrate_kernel<G, DP, Div, false>>(plan, s, args...);
}

// the fixed-step solve: instances as launch_cnf_field picks them, with the tape or without
static int launch_cnf_integrate(const float* z, const float* logp, const float* e, const float* image, float* z_out,
                                float* logp_out, float* tape, float* evals, int64_t n, const CnfShape& sh,
                                int image_floats, double t0, double t1, int steps, int method, hipStream_t s) {
  const int group = cnf_group(sh, e != nullptr), table = cnf_table_doubles(sh);
  const GroupLaunch plan = group_launch_plan(image_floats, group, cnf_forward_lds(sh), kPrefer64K, n, kGroupMaxBlocks);
  if (e)
    return with_constant<4, 8, 16>(sh.d <= 4 ? 4 : sh.d <= 8 ? 8 : 16, [&](auto dp) {
      constexpr int DP = decltype(dp)::value;
      return launch_cnf_integrate_as<2, DP, CnfHutchinsonDiv<DP>>(tape != nullptr, plan, s, z, logp, e, image, z_out,
                                                                  logp_out, tape, evals, n, sh, image_floats, table,
                                                                  t0, t1, steps, method);
    });
  return with_constant<2, 4, 8, 16, 32>(group, [&](auto g) {
    constexpr int G = decltype(g)::value;
    return launch_cnf_integrate_as<G, LaneGroup<G>::DP, CnfExactDiv>(tape != nullptr, plan, s, z, logp, e, image, z_out,
                                                                    logp_out, tape, evals, n, sh, image_floats, table,
                                                                    t0, t1, steps, method);
  });
}

// what every fixed-step entry checks of its step sequence
inline bool cnf_fixed_steps(double t0, double t1, int steps, int method) {
  return steps >= 1 && method >= FC_CNF_EULER && method <= FC_CNF_RK4 && t0 == t0 && t1 == t1;
}

// the backward kernel's table and a lane's slots: the largest block that fits, a block per tile up to the cap
static GroupLaunch cnf_backward_plan(const CnfShape& sh, int image_floats, bool with_e, int64_t n) {
  const GroupLds need{sizeof(double) * (size_t)cnf_table_doubles(sh), cnf_backward_lane_floats(sh), 0, 0};
  return group_launch_plan(image_floats, cnf_group(sh, with_e), need, kLargestBlock, n, kGroupBackwardMaxBlocks);
}

// The plan of the backward launch for n rows of a net known by its widths alone; false outside the kernel's limits.
static bool cnf_backward_query(int64_t n, int d, int layers, const int32_t* hidden, bool with_e, CnfShape* sh,
                               GroupLaunch* plan) {
  if (n < 0 || layers > kCnfTrainMaxLayers || !cnf_shape(d, layers, hidden, 0, 0, 0, 1.f, 1.f, sh)) return false;
  *plan = cnf_backward_plan(*sh, cnf_image_floats(*sh), with_e, n);
  return plan->threads != 0;
}

}  // namespace fc

extern "C" int fc_cnf_field_train(const float* y, const float* e, const float* image, float* dy, float* negdiv,
                                  float* evals, int64_t n, int32_t d, int32_t layers, const int32_t* hidden,
                                  int32_t layer_kind, int32_t activation, int32_t residual, float scale_output,
                                  float p0, int32_t image_floats, float t, const float* t_dev, void* stream) {
  fc::CnfShape sh;
  if (!fc::cnf_entry(n, d, layers, hidden, layer_kind, activation, residual, scale_output, p0, image_floats,
                     fc::kCnfTrainMaxLayers, &sh))
    return hipErrorInvalidValue;
  if (n == 0) return hipSuccess;
  if (!fc::cnf_operands(y, image, dy, negdiv)) return hipErrorInvalidValue;
  return fc::launch_cnf_field(y, e, image, dy, negdiv, evals, n, sh, image_floats, t, t_dev,
                              static_cast<hipStream_t>(stream));
}

extern "C" int fc_cnf_field_backward_rows(int32_t d, int32_t layers, const int32_t* hidden, int32_t with_e) {
  fc::CnfShape sh;
  fc::GroupLaunch plan;
  if (!fc::cnf_backward_query(0, d, layers, hidden, with_e != 0, &sh, &plan)) return -1;
  return plan.threads / fc::cnf_group(sh, with_e != 0);
}

extern "C" int fc_cnf_field_backward_workspace(int64_t n, int32_t d, int32_t layers, const int32_t* hidden,
                                               int32_t with_e) {
  fc::CnfShape sh;
  fc::GroupLaunch plan;
  if (!fc::cnf_backward_query(n, d, layers, hidden, with_e != 0, &sh, &plan)) return -1;
  return (int)(2 * plan.grid * fc::cnf_image_floats(sh));
}

extern "C" int fc_cnf_field_backward(const float* y, const float* e, const float* image, const float* g_dy,
                                     const float* g_negdiv, float* g_y, float* g_image, void* workspace, int64_t n,
                                     int32_t d, int32_t layers, const int32_t* hidden, int32_t layer_kind,
                                     int32_t activation, int32_t residual, float scale_output, float p0,
                                     int32_t image_floats, float t, const float* t_dev, void* stream) {
  fc::CnfShape sh;
  if (!fc::cnf_entry(n, d, layers, hidden, layer_kind, activation, residual, scale_output, p0, image_floats,
                     fc::kCnfTrainMaxLayers, &sh))
    return hipErrorInvalidValue;
  if (!g_image) return hipErrorInvalidValue;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (n == 0) return hipMemsetAsync(g_image, 0, sizeof(float) * (size_t)image_floats, s);
  if (!y || !image || !g_dy || !g_negdiv || !g_y || !workspace || (reinterpret_cast<uintptr_t>(workspace) & 7))
    return hipErrorInvalidValue;
  double* partial = static_cast<double*>(workspace);
  const fc::GroupLaunch plan = fc::cnf_backward_plan(sh, image_floats, e != nullptr, n);
  const int launched = fc::with_constant<2, 4, 8, 16, 32>(fc::cnf_group(sh, e != nullptr), [&](auto g) {
    return fc::group_launch<&fc::cnf_backward_kernel<decltype(g)::value>>(
        plan, s, y, e, image, g_dy, g_negdiv, g_y, partial, n, sh, image_floats, fc::cnf_table_doubles(sh),
        fc::cnf_backward_lane_floats(sh), t, t_dev);
  });
  if (launched != hipSuccess) return launched;
  return fc::launch_partial_sum(partial, g_image, (int)plan.grid, image_floats, sh.scale, s);  // scale_output
}

extern "C" int fc_cnf_field(const float* y, const float* image, float* dy, float* negdiv, float* evals, int64_t n,
                            int32_t d, int32_t layers, const int32_t* hidden, int32_t layer_kind, int32_t activation,
                            int32_t residual, float scale_output, float p0, int32_t image_floats, float t,
                            const float* t_dev, void* stream) {
  fc::CnfShape sh;
  if (!fc::cnf_entry(n, d, layers, hidden, layer_kind, activation, residual, scale_output, p0, image_floats,
                     FC_CNF_MAX_HIDDEN_LAYERS + 1, &sh))
    return hipErrorInvalidValue;
  if (n == 0) return hipSuccess;
  if (!fc::cnf_operands(y, image, dy, negdiv)) return hipErrorInvalidValue;
  return fc::launch_cnf_field(y, nullptr, image, dy, negdiv, evals, n, sh, image_floats, t, t_dev,
                              static_cast<hipStream_t>(stream));
}

extern "C" int fc_cnf_integrate(const float* z, const float* logp, const float* image, float* z_out, float* logp_out,
                                float* evals, int64_t n, int32_t d, int32_t layers, const int32_t* hidden,
                                int32_t layer_kind, int32_t activation, int32_t residual, float scale_output, float p0,
                                int32_t image_floats, double t0, double t1, int32_t steps, int32_t method,
                                void* stream) {
  fc::CnfShape sh;
  if (!fc::cnf_fixed_steps(t0, t1, steps, method)) return hipErrorInvalidValue;
  if (!fc::cnf_entry(n, d, layers, hidden, layer_kind, activation, residual, scale_output, p0, image_floats,
                     FC_CNF_MAX_HIDDEN_LAYERS + 1, &sh))
    return hipErrorInvalidValue;
  if (n == 0) return hipSuccess;
  if (!fc::cnf_operands(z, image, z_out, logp_out)) return hipErrorInvalidValue;
  return fc::launch_cnf_integrate(z, logp, nullptr, image, z_out, logp_out, nullptr, evals, n, sh, image_floats, t0, t1,
                                  steps, method, static_cast<hipStream_t>(stream));
}

extern "C" int fc_cnf_integrate_train(const float* z, const float* logp, const float* e, const float* image,
                                      float* z_out, float* logp_out, float* tape, float* evals, int64_t n, int32_t d,
                                      int32_t layers, const int32_t* hidden, int32_t layer_kind, int32_t activation,
                                      int32_t residual, float scale_output, float p0, int32_t image_floats, double t0,
                                      double t1, int32_t steps, int32_t method, void* stream) {
  fc::CnfShape sh;
  if (!fc::cnf_fixed_steps(t0, t1, steps, method)) return hipErrorInvalidValue;
  if (!fc::cnf_entry(n, d, layers, hidden, layer_kind, activation, residual, scale_output, p0, image_floats,
                     fc::kCnfTrainMaxLayers, &sh))
    return hipErrorInvalidValue;
  if (n == 0) return hipSuccess;
  if (!fc::cnf_operands(z, image, z_out, logp_out)) return hipErrorInvalidValue;
  return fc::launch_cnf_integrate(z, logp, e, image, z_out, logp_out, tape, evals, n, sh, image_floats, t0, t1, steps,
                                  method, static_cast<hipStream_t>(stream));
}

// the partial images and the three float64 [n, d] planes; -1 as well where the count does not fit an int
extern "C" int fc_cnf_integrate_backward_workspace(int64_t n, int32_t d, int32_t layers, const int32_t* hidden,
                                                   int32_t with_e) {
  fc::CnfShape sh;
  fc::GroupLaunch plan;
  if (!fc::cnf_backward_query(n, d, layers, hidden, with_e != 0, &sh, &plan)) return -1;
  if (n > (INT32_MAX / 8) / d) return -1;
  const int64_t floats = 2 * (plan.grid * (int64_t)fc::cnf_image_floats(sh) + 3 * n * (int64_t)d);
  return floats <= INT32_MAX ? (int)floats : -1;
}

extern "C" int fc_cnf_integrate_backward(const float* tape, const float* e, const float* image, const float* g_z_out,
                                         const float* g_logp_out, float* g_z, float* g_image, void* workspace,
                                         int64_t n, int32_t d, int32_t layers, const int32_t* hidden,
                                         int32_t layer_kind, int32_t activation, int32_t residual, float scale_output,
                                         float p0, int32_t image_floats, double t0, double t1, int32_t steps,
                                         int32_t method, void* stream) {
  fc::CnfShape sh;
  if (!fc::cnf_fixed_steps(t0, t1, steps, method)) return hipErrorInvalidValue;
  if (!fc::cnf_entry(n, d, layers, hidden, layer_kind, activation, residual, scale_output, p0, image_floats,
                     fc::kCnfTrainMaxLayers, &sh))
    return hipErrorInvalidValue;
  if (!g_image) return hipErrorInvalidValue;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (n == 0) return hipMemsetAsync(g_image, 0, sizeof(float) * (size_t)image_floats, s);
  if (!tape || !image || !g_z_out || !g_logp_out || !g_z || !workspace || (reinterpret_cast<uintptr_t>(workspace) & 7))
    return hipErrorInvalidValue;
  const fc::GroupLaunch plan = fc::cnf_backward_plan(sh, image_floats, e != nullptr, n);
  double* partial = static_cast<double*>(workspace);
  double* planes = partial + (size_t)plan.grid * (size_t)image_floats;
  const int launched = fc::with_constant<2, 4, 8, 16, 32>(fc::cnf_group(sh, e != nullptr), [&](auto g) {
    return fc::group_launch<&fc::cnf_solve_backward_kernel<decltype(g)::value>>(
        plan, s, tape, e, image, g_z_out, g_logp_out, g_z, partial, planes, n, sh, image_floats,
        fc::cnf_table_doubles(sh), fc::cnf_backward_lane_floats(sh), t0, t1, steps, method);
  });
  if (launched != hipSuccess) return launched;
  return fc::launch_partial_sum(partial, g_image, (int)plan.grid, image_floats, sh.scale, s);  // scale_output
}
