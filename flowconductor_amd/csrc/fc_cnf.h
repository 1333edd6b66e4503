// What the continuous-normalizing-flow kernels share (fc_cnf.hip, fc_cnf_dopri5.hip): the description of a net, the
// activations, the source of the terms that depend on t alone, and cnf_net / cnf_field_row -- the one copy of the layer
// arithmetic.  The image layout and the lane layout are described at the top of fc_cnf.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/flowcon_hip.h"
#include "fc_device.h"

namespace fc {

struct CnfShape {
  int d, layers, act, gated, residual;
  int w[FC_CNF_MAX_HIDDEN_LAYERS + 2];  // w[0] = d, hidden widths, w[layers] = d
  double scale, p0;
};

__host__ __device__ inline int cnf_pad4(int v) { return (v + 3) & ~3; }

__host__ __device__ inline int cnf_image_floats(const CnfShape& sh) {
  int total = 0;
  for (int l = 0; l < sh.layers; ++l) total += (5 + sh.w[l]) * cnf_pad4(sh.w[l + 1]);
  return total;
}

__host__ __device__ inline int cnf_table_doubles(const CnfShape& sh) {
  int total = 0;
  for (int l = 0; l < sh.layers; ++l) total += 3 * cnf_pad4(sh.w[l + 1]);
  return total;
}

__host__ __device__ inline int cnf_max_width(const CnfShape& sh) {
  int m = sh.d;
  for (int l = 1; l < sh.layers; ++l) m = sh.w[l] > m ? sh.w[l] : m;
  return m;
}

// value and derivative of the activation, in float64 on the float64 pre-activation
__device__ __forceinline__ void cnf_act(int act, double x, double p0, double& f, double& df) {
  switch (act) {
    case FC_CNF_ACT_TANH: {
      const double th = tanh(x);
      f = th;
      df = 1.0 - th * th;
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
      break;
    }
    case FC_CNF_ACT_ELU:
      f = x > 0.0 ? x : p0 * expm1(x);
      df = x > 0.0 ? 1.0 : p0 * exp(x);
      break;
    case FC_CNF_ACT_SWISH: {
      const double sg = 1.0 / (1.0 + exp(-x));
      f = x * sg;
      df = sg + x * sg * (1.0 - sg);
      break;
    }
    case FC_CNF_ACT_SQUARE:
      f = x * x;
      df = 2.0 * x;
      break;
    default:
      f = x;
      df = 1.0;
      break;
  }
}

// What depends on t alone, per layer [b + w_t t | gate | w_b t], each op doubles.  The whole block takes part; the
// caller puts barriers round it.
__device__ __forceinline__ void cnf_time_table(const float* img, double* tab, const CnfShape& sh, double t, int tid,
                                               int T) {
  const float* p = img;
  double* q = tab;
  for (int l = 0; l < sh.layers; ++l) {
    const int op = cnf_pad4(sh.w[l + 1]);
    for (int o = tid; o < op; o += T) {
      q[o] = (double)p[o] + (double)p[op + o] * t;
      q[op + o] = sh.gated ? 1.0 / (1.0 + exp(-((double)p[2 * op + o] * t + (double)p[3 * op + o]))) : 1.0;
      q[2 * op + o] = (double)p[4 * op + o] * t;
    }
    p += (5 + sh.w[l]) * op;
    q += 3 * op;
  }
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

// ---- the net on one stream -------------------------------------------------------------------------------------------

// Runs the layers on the state column `mine` (stride T, the second buffer `half` floats further on), whose first d
// entries the caller has set: the input (value stream, s == 0) or a unit tangent (s >= 1).  out[i], i < DP: the last
// layer in unrounded float64 -- f in the value stream, column s - 1 of df/dy in stream s.  This is the one place that
// fixes where float32 roundings happen: a stored activation, once.
template <int G, int DP, class Time>
__device__ __forceinline__ void cnf_net(const float* img, Time tm, float* mine, int T, int half, const CnfShape& sh,
                                        int s, double (&out)[DP]) {
  const bool value = s == 0;
  const float* p = img;
  float* cur = mine;
  float* nxt = mine + half;
  for (int l = 0; l + 1 < sh.layers; ++l) {
    const int in = sh.w[l], width = sh.w[l + 1], op = cnf_pad4(width);
    const float* wt = p + 5 * op;
    tm.begin_layer(p, op);
    for (int o = 0; o < op; o += 4) {
      double sum[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) sum[c] = value ? tm.bias(p, op, o + c) : 0.0;  // a tangent: no bias, no time terms
      for (int k = 0; k < in; ++k) {
        const double v = (double)cur[k * T];
        const float4 w4 = *reinterpret_cast<const float4*>(wt + k * op + o);
        sum[0] = fma((double)w4.x, v, sum[0]);
        sum[1] = fma((double)w4.y, v, sum[1]);
        sum[2] = fma((double)w4.z, v, sum[2]);
        sum[3] = fma((double)w4.w, v, sum[3]);
      }
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        double lin = sum[c] * tm.gate(p, op, o + c);
        if (value) lin += tm.shift(p, op, o + c);
        const double pre = __shfl(lin, 0, G);  // the value stream's
        if (o + c < width) {
          double f, df;
          cnf_act(sh.act, pre, sh.p0, f, df);
          nxt[(o + c) * T] = (float)(value ? f : df * lin);
        }
      }
    }
    float* swap = cur;
    cur = nxt;
    nxt = swap;
    p = wt + in * op;
    tm.end_layer(op);
  }
  const int in = sh.w[sh.layers - 1], dp = cnf_pad4(sh.d);
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

// One evaluation of the ODE function for the row of this group at the float32 state xin: k[i] = dy_i (meaningful in
// the value lane), negdiv = -div (the same in every lane of the group), scale_output and residual folded in.
template <int G, int DP, class Time>
__device__ __forceinline__ void cnf_field_row(const float* img, Time tm, float* mine, int T, int half,
                                              const CnfShape& sh, int s, const float (&xin)[DP], double (&k)[DP],
                                              double& negdiv) {
#pragma unroll
  for (int i = 0; i < DP; ++i)
    if (i < sh.d) mine[i * T] = s == 0 ? xin[i] : (i == s - 1 ? 1.f : 0.f);
  cnf_net<G, DP>(img, tm, mine, T, half, sh, s, k);
  double diag = 0.0;
#pragma unroll
  for (int i = 0; i < DP; ++i)
    if (i == s - 1 && i < sh.d) diag = k[i];
#pragma unroll
  for (int off = G / 2; off > 0; off >>= 1) diag += __shfl_xor(diag, off, G);
  double div = diag * sh.scale;
#pragma unroll
  for (int i = 0; i < DP; ++i) {
    k[i] *= sh.scale;
    if (sh.residual) k[i] -= (double)xin[i];
  }
  if (sh.residual) div -= (double)sh.d;
  negdiv = -div;
}

template <int G>
struct CnfGroup {
  static constexpr int DMAX = G == 32 ? 16 : G - 1;
  static constexpr int DP = (DMAX + 3) & ~3;
};

// ---- launch ---------------------------------------------------------------------------------------------------------

constexpr int kCnfLdsLimit = 128 * 1024;
constexpr int kCnfMaxBlocks = 2048;

inline bool cnf_shape(int d, int layers, const int32_t* hidden, int kind, int act, int residual, float scale, float p0,
                      int image_floats, CnfShape* sh) {
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
  return cnf_image_floats(*sh) == image_floats;
}

}  // namespace fc
