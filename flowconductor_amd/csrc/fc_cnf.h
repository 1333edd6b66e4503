// What the continuous-normalizing-flow kernels share (fc_cnf.hip, fc_cnf_dopri5.hip) on top of the lane-group scaffold
// of fc_lane_group.h (the block set-up, the weight sums, the launch plan): the description of a net, the activations,
// the source of the terms that depend on t alone, and cnf_hidden_layers / cnf_net / cnf_field_row -- the one copy of the
// layer arithmetic, which the backward kernel's recompute runs too.  The image layout and the lane layout are described
// at the top of fc_cnf.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/flowcon_hip.h"
#include "fc_lane_group.h"

namespace fc {

struct CnfShape {
  int d, layers, act, gated, residual;
  int w[FC_CNF_MAX_HIDDEN_LAYERS + 2];  // w[0] = d, hidden widths, w[layers] = d
  double scale, p0;
};

__host__ __device__ inline int cnf_image_floats(const CnfShape& sh) {
  int total = 0;
  for (int l = 0; l < sh.layers; ++l) total += (5 + sh.w[l]) * pad4(sh.w[l + 1]);
  return total;
}

__host__ __device__ inline int cnf_table_doubles(const CnfShape& sh) {
  int total = 0;
  for (int l = 0; l < sh.layers; ++l) total += 3 * pad4(sh.w[l + 1]);
  return total;
}

// the widest column a layer reads or writes
__host__ __device__ inline int cnf_max_width(const CnfShape& sh) {
  int m = sh.d;
  for (int l = 1; l < sh.layers; ++l) m = sh.w[l] > m ? sh.w[l] : m;
  return m;
}

// Value, derivative and (Second) second derivative of the activation, in float64 on the float64 pre-activation (what
// torch's double backward gives).  What a caller does not read is not computed.
template <bool Second>
__device__ __forceinline__ void cnf_act_eval(int act, double x, double p0, double& f, double& df, double& d2f) {
  d2f = 0.0;
  switch (act) {
    case FC_CNF_ACT_TANH: {
      const double th = tanh(x);
      f = th;
      df = 1.0 - th * th;
      if (Second) d2f = -2.0 * th * df;
      break;
    }
    case FC_CNF_ACT_RELU:
      f = x > 0.0 ? x : 0.0;
      df = x > 0.0 ? 1.0 : 0.0;
      break;
    case FC_CNF_ACT_SOFTPLUS: {  // beta 1, threshold 20 as torch evaluates it
      const double sg = 1.0 / (1.0 + exp(-x));
      f = x > 20.0 ? x : log1p(exp(x));
      df = x > 20.0 ? 1.0 : sg;
      if (Second) d2f = x > 20.0 ? 0.0 : sg * (1.0 - sg);
      break;
    }
    case FC_CNF_ACT_ELU:
      f = x > 0.0 ? x : p0 * expm1(x);
      df = x > 0.0 ? 1.0 : p0 * exp(x);
      if (Second) d2f = x > 0.0 ? 0.0 : p0 * exp(x);
      break;
    case FC_CNF_ACT_SWISH: {
      const double sg = 1.0 / (1.0 + exp(-x));
      const double ds = sg * (1.0 - sg);
      f = x * sg;
      // the one derivative whose product the backward walk has always associated the other way; both kept bit for bit
      df = Second ? sg + x * ds : sg + x * sg * (1.0 - sg);
      if (Second) d2f = ds * (2.0 + x * (1.0 - 2.0 * sg));
      break;
    }
    case FC_CNF_ACT_SQUARE:
      f = x * x;
      df = 2.0 * x;
      if (Second) d2f = 2.0;
      break;
    default:
      f = x;
      df = 1.0;
      break;
  }
}

__device__ __forceinline__ void cnf_act(int act, double x, double p0, double& f, double& df) {
  double d2f;
  cnf_act_eval<false>(act, x, p0, f, df, d2f);
}

// first and second derivative, for the backward walk
__device__ __forceinline__ void cnf_act2(int act, double x, double p0, double& df, double& d2f) {
  double f;
  cnf_act_eval<true>(act, x, p0, f, df, d2f);
}

// What depends on t alone, per layer [b + w_t t | gate | w_b t], each op doubles.  The whole block takes part; the
// caller puts barriers round it.
__device__ __forceinline__ void cnf_time_table(const float* img, double* tab, const CnfShape& sh, double t, int tid,
                                               int T) {
  const float* p = img;
  double* q = tab;
  for (int l = 0; l < sh.layers; ++l) {
    const int op = pad4(sh.w[l + 1]);
    for (int o = tid; o < op; o += T) {
      q[o] = (double)p[o] + (double)p[op + o] * t;
      q[op + o] = sh.gated ? 1.0 / (1.0 + exp(-((double)p[2 * op + o] * t + (double)p[3 * op + o]))) : 1.0;
      q[2 * op + o] = (double)p[4 * op + o] * t;
    }
    p += (5 + sh.w[l]) * op;
    q += 3 * op;
  }
}

// The scaffold's block with the forward kernels' two ping-pong columns: `mid` holds the block's time table or a gate
// strip per row.  Like group_block it ends without a barrier.
struct CnfBlock : GroupBlock {
  int half;  // the second ping-pong buffer, that many floats after the first
};

template <int G>
__device__ __forceinline__ CnfBlock cnf_block(float* lds, const float* __restrict__ image, int image_floats,
                                              int block_doubles, int row_doubles, int64_t n, const CnfShape& sh) {
  CnfBlock b;
  static_cast<GroupBlock&>(b) = group_lanes<G>();
  b.half = cnf_max_width(sh) * b.T;
  group_carve(b, lds, image, image_floats, block_doubles, row_doubles, n);
  return b;
}

// ---- where cnf_net takes the time terms of a layer from ---------------------------------------------------------------
//
// p is the layer's piece of the image (b w_t w_g b_g w_b, op floats each), o an output of the layer.  Both sources
// give the same float64 numbers for the same t: the expressions are cnf_time_table's.

// All rows of the block share t: the table cnf_time_table built, behind the caller's barriers.
struct CnfBlockTime {
  const double* q;
  __device__ __forceinline__ void begin_layer(const float*, int) {}
  __device__ __forceinline__ double bias(const float*, int, int o) const { return q[o]; }
  __device__ __forceinline__ double gate(const float*, int op, int o) const { return q[op + o]; }
  __device__ __forceinline__ double shift(const float*, int op, int o) const { return q[2 * op + o]; }
  __device__ __forceinline__ void end_layer(int op) { q += 3 * op; }
};

// Every row has its own t.  The two fma terms are computed where they are used; for the gated kinds the G lanes of the
// row's group compute the layer's gates together (op / G sigmoids per lane) into the row's LDS strip of max op doubles,
// which the value and tangent lanes of the same group read back.  A group lies inside one wave and runs in lockstep,
// so no block barrier is needed, only the ordering of the LDS accesses (the fences).  Ungated kinds touch no strip.
template <int G>
struct CnfRowTime {
  double t;
  double* strip;
  int lane, gated;
  static __device__ __forceinline__ void order() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }
  __device__ __forceinline__ void begin_layer(const float* p, int op) {
    if (!gated) return;
    for (int o = lane; o < op; o += G)
      strip[o] = 1.0 / (1.0 + exp(-((double)p[2 * op + o] * t + (double)p[3 * op + o])));
    order();
  }
  __device__ __forceinline__ double bias(const float* p, int op, int o) const {
    return (double)p[o] + (double)p[op + o] * t;
  }
  __device__ __forceinline__ double gate(const float*, int, int o) const { return gated ? strip[o] : 1.0; }
  __device__ __forceinline__ double shift(const float* p, int op, int o) const { return (double)p[4 * op + o] * t; }
  __device__ __forceinline__ void end_layer(int) {
    if (gated) order();  // the next layer's gates overwrite the strip
  }
};

// ---- where a hidden layer's columns live ------------------------------------------------------------------------------
//
// in(): the column (stride T) layer l reads, out(w): the one it writes, w its input width.

// two buffers, swapped per layer: all the forward kernels need
struct CnfPingPong {
  float* cur;
  float* nxt;
  __device__ __forceinline__ const float* in(int) const { return cur; }
  __device__ __forceinline__ float* out(int, int) const { return nxt; }
  __device__ __forceinline__ void advance(int) {
    float* swap = cur;
    cur = nxt;
    nxt = swap;
  }
};

// every layer's input kept, slot on slot: what the backward walk reads again
struct CnfStacked {
  float* mine;
  int off;  // floats of the slots below the current layer's input
  __device__ __forceinline__ const float* in(int T) const { return mine + off * T; }
  __device__ __forceinline__ float* out(int w, int T) const { return mine + (off + w) * T; }
  __device__ __forceinline__ void advance(int w) { off += w; }
};

// ---- the net on one stream -------------------------------------------------------------------------------------------

// weight_sum4 with the layer's time-dependent bias b + w_t t
template <class Time>
__device__ __forceinline__ void cnf_sum4(const float* wt, const Time& tm, const float* p, const float* x, int T, int in,
                                         int op, int o, bool value, double (&sum)[4]) {
  weight_sum4(wt, x, T, in, op, o, value, [&](int oc) { return tm.bias(p, op, oc); }, sum);
}

// From cnf_sum4's sum of output o: lin, this stream's gated product, and pre, the value stream's, which is the
// pre-activation every stream of the group differentiates at.
template <int G, class Time>
__device__ __forceinline__ void cnf_lin_pre(const Time& tm, const float* p, int op, int o, bool value, double sum,
                                            double& lin, double& pre) {
  lin = sum * tm.gate(p, op, o);
  if (value) lin += tm.shift(p, op, o);
  pre = __shfl(lin, 0, G);
}

// The hidden layers on this lane's stream, whose first column the caller has set; returns the last layer's piece of the
// image, with `tm` and `at` standing at that layer.  This is the one place that fixes where float32 roundings happen:
// a stored activation, once.  The forward kernels and the backward kernel's recompute all run it.
template <int G, class Time, class Store>
__device__ __forceinline__ const float* cnf_hidden_layers(const float* img, Time& tm, Store& at, int T,
                                                          const CnfShape& sh, bool value) {
  const float* p = img;
  for (int l = 0; l + 1 < sh.layers; ++l) {
    const int in = sh.w[l], width = sh.w[l + 1], op = pad4(width);
    const float* wt = p + 5 * op;
    const float* cur = at.in(T);
    float* nxt = at.out(in, T);
    tm.begin_layer(p, op);
    for (int o = 0; o < op; o += 4) {
      double sum[4];
      cnf_sum4(wt, tm, p, cur, T, in, op, o, value, sum);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        double lin, pre;
        cnf_lin_pre<G>(tm, p, op, o + c, value, sum[c], lin, pre);
        if (o + c < width) {
          double f, df;
          cnf_act(sh.act, pre, sh.p0, f, df);
          nxt[(o + c) * T] = (float)(value ? f : df * lin);
        }
      }
    }
    at.advance(in);
    p = wt + in * op;
    tm.end_layer(op);
  }
  return p;
}

// Runs the layers on the state column `mine` (stride T, the second buffer `half` floats further on), whose first d
// entries the caller has set: the input (value stream, s == 0) or a tangent's seed (s >= 1).  out[i], i < DP: the last
// layer in unrounded float64 -- f in the value stream, J times the seed in a tangent stream.
template <int G, int DP, class Time>
__device__ __forceinline__ void cnf_net(const float* img, Time tm, float* mine, int T, int half, const CnfShape& sh,
                                        int s, double (&out)[DP]) {
  const bool value = s == 0;
  CnfPingPong at{mine, mine + half};
  const float* p = cnf_hidden_layers<G>(img, tm, at, T, sh, value);
  const float* cur = at.in(T);
  const int in = sh.w[sh.layers - 1], dp = pad4(sh.d);
  const float* wt = p + 5 * dp;
  tm.begin_layer(p, dp);
#pragma unroll
  for (int i = 0; i < DP; ++i) out[i] = (value && i < dp) ? tm.bias(p, dp, i) : 0.0;
  for (int k = 0; k < in; ++k) {
    const double v = (double)cur[k * T];
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
#pragma unroll
  for (int i = 0; i < DP; ++i) {
    if (i < dp) {
      out[i] *= tm.gate(p, dp, i);
      if (value) out[i] += tm.shift(p, dp, i);
    }
  }
  tm.end_layer(dp);
}

// ---- what the tangent lanes carry, and how their results become the divergence ------------------------------------------

// The exact divergence: lane j + 1 carries d/dy_j and ends with column j of the Jacobian, of which the diagonal entry
// is summed over the group.  Empty, so that handing it on costs no register.
struct CnfExactDiv {
  __device__ __forceinline__ void load(const float*, int64_t, int) {}
  __device__ __forceinline__ float seed(int i, int s) const { return i == s - 1 ? 1.f : 0.f; }
  template <int G, int DP>
  __device__ __forceinline__ double reduce(const double (&k)[DP], int s, int d) const {
    double diag = 0.0;
#pragma unroll
    for (int i = 0; i < DP; ++i)
      if (i == s - 1 && i < d) diag = k[i];
    return lane_sum<G>(diag);
  }
};

// Hutchinson's estimate e^T (J e): a group of 2 lanes, the one tangent lane seeded with the row's noise e.
template <int DP>
struct CnfHutchinsonDiv {
  float e[DP];
  __device__ __forceinline__ void load(const float* __restrict__ noise, int64_t row, int d) {
#pragma unroll
    for (int i = 0; i < DP; ++i) e[i] = i < d ? noise[row * d + i] : 0.f;
  }
  __device__ __forceinline__ float seed(int i, int) const { return e[i]; }
  template <int G, int>
  __device__ __forceinline__ double reduce(const double (&k)[DP], int s, int d) const {
    static_assert(G == 2, "one tangent lane");
    double dot = 0.0;
#pragma unroll
    for (int i = 0; i < DP; ++i)
      if (s == 1 && i < d) dot += (double)e[i] * k[i];
    return dot + __shfl_xor(dot, 1, G);
  }
};

// One evaluation of the ODE function for the row of this group at the float32 state xin: k[i] = dy_i (meaningful in
// the value lane), negdiv = -div (the same in every lane of the group), scale_output and residual folded in.
template <int G, int DP, class Time, class Div>
__device__ __forceinline__ void cnf_field_row(const float* img, Time tm, Div dv, float* mine, int T, int half,
                                              const CnfShape& sh, int s, const float (&xin)[DP], double (&k)[DP],
                                              double& negdiv) {
#pragma unroll
  for (int i = 0; i < DP; ++i)
    if (i < sh.d) mine[i * T] = s == 0 ? xin[i] : dv.seed(i, s);
  cnf_net<G, DP>(img, tm, mine, T, half, sh, s, k);
  double div = dv.template reduce<G, DP>(k, s, sh.d) * sh.scale;
#pragma unroll
  for (int i = 0; i < DP; ++i) {
    if (i < sh.d) {  // nobody reads the padding
      k[i] *= sh.scale;
      if (sh.residual) k[i] -= (double)xin[i];
    }
  }
  if (sh.residual) div -= (double)sh.d;
  negdiv = -div;
}

// ---- entry: the net a call describes -----------------------------------------------------------------------------------

inline bool cnf_shape(int d, int layers, const int32_t* hidden, int kind, int act, int residual, float scale, float p0,
                      CnfShape* sh) {
  if (d < 1 || d > FC_CNF_MAX_DIM || layers < 1 || layers > FC_CNF_MAX_HIDDEN_LAYERS + 1) return false;
  if (kind < 0 || kind > FC_CNF_LAYER_CONCATSQUASH || act < 0 || act > FC_CNF_ACT_IDENTITY) return false;
  if (layers > 1 && !hidden) return false;
  sh->d = d;
  sh->layers = layers;
  sh->act = act;
  sh->gated = (kind == FC_CNF_LAYER_SQUASH || kind == FC_CNF_LAYER_CONCATSQUASH) ? 1 : 0;
  sh->residual = residual ? 1 : 0;
  sh->scale = (double)scale;
  sh->p0 = (double)p0;
  for (int l = 0; l < FC_CNF_MAX_HIDDEN_LAYERS + 2; ++l) sh->w[l] = 0;
  sh->w[0] = d;
  for (int l = 1; l < layers; ++l) {
    if (hidden[l - 1] < 1 || hidden[l - 1] > FC_CNF_MAX_WIDTH) return false;
    sh->w[l] = hidden[l - 1];
  }
  sh->w[layers] = d;
  return true;
}

// What every launching entry point starts with: a row count, a net of at most max_layers layers, the image it says.
inline bool cnf_entry(int64_t n, int d, int layers, const int32_t* hidden, int kind, int act, int residual, float scale,
                      float p0, int image_floats, int max_layers, CnfShape* sh) {
  return n >= 0 && layers <= max_layers && cnf_shape(d, layers, hidden, kind, act, residual, scale, p0, sh) &&
         cnf_image_floats(*sh) == image_floats;
}

// rows in, the image, rows out and the per-row output: all there, and not in place
inline bool cnf_operands(const void* in, const void* image, const void* out, const void* out1) {
  return in && image && out && out1 && in != out;
}

// ---- launch ---------------------------------------------------------------------------------------------------------

// The lane group of a net's rows; under Hutchinson's estimator 2 lanes carry a row.
inline int cnf_group(const CnfShape& sh, bool hutchinson = false) { return hutchinson ? 2 : lane_group(sh.d); }

// the forward kernels' time table and two ping-pong columns
inline GroupLds cnf_forward_lds(const CnfShape& sh) {
  return {sizeof(double) * (size_t)cnf_table_doubles(sh), 2 * cnf_max_width(sh), 0, 0};
}

}  // namespace fc
