// Backward of the deep sigmoidal flow (fc_deep_sigmoid.hip), forward direction, gfx950.
//
// For y, logabsdet = deep_sigmoid(x, raw) (flowcon/transforms/adaptive_sigmoids.py:177-210) and upstream gradients
// gy [N, D], gl [N]:
//     grad_x[n, j]        = gy dy/dx + gl dlad/dx
//     grad_raw[n, j, 3S]  = gy dy/draw + gl dlad/draw          (what torch.autograd yields for the reference's ops)
// With  a_k = (1 - m) softplus(p raw_a_k) + m,  b_k = (1 - m) p raw_b_k,  w = softmax(p raw_w),  pre_k = a_k x + b_k,
// sg_k = sigmoid(pre_k),  s = sum_k w_k sg_k,  c = (1 - eps) s + eps / 2,  q = 1 - c,  D = sum_k w_k a_k sg'_k:
//     y   = log c - log q                                        dy/ds   = (1 - eps) (1 / c + 1 / q)
//     lad = log D + log(1 - eps) - 2 eps - log c - log q          dlad/ds = (1 - eps) (1 / q - 1 / c),  dlad/dD = 1 / D
// D underflows where every sigmoid saturates, so 1 / D never appears: with lj_k = log(w_k a_k sg'_k) and
// pi_k = exp(lj_k - logsumexp(lj)) = w_k a_k sg'_k / D,
//     g_s     = gy dy/ds + gl dlad/ds
//     g_pre_k = g_s w_k sg'_k + gl pi_k (1 - 2 sg_k)
//     g_a_k   = g_pre_k x + gl pi_k / a_k,      g_b_k = g_pre_k,      grad_x = sum_k g_pre_k a_k
//     g_w_k   = g_s sg_k + gl pi_k / w_k   ->   g_rawW_k = p (g_s w_k sg_k + gl pi_k - w_k (g_s s + gl))      (softmax)
// and the chain to the raw values is p (1 - m) sigmoid(p raw_a_k) and p (1 - m).
//
// One lane per (sample, dim), three passes over the S sigmoids recomputing the derived parameters from the raw row (no
// per-thread arrays: S is a run-time value).  Per-sample rows travel through LDS (coalesced in, coalesced out); a
// batch-shared row is reduced inside the workgroup, see ds_backward_shared_kernel.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "fc_device.h"
#include "fc_math.h"
#include "fc_partial_sum.h"
#include "../../include/flowcon_hip.h"

namespace fc {

constexpr int kDsSharedMaxGrid = 512;              // rows of the partial buffer: fixed, so the sum's order is too
constexpr size_t kDsSharedMaxLds = 64 * 1024;

struct DsBwdArgs {
  const float* x;        // [N, D]
  const float* raw;      // [N, D, 3S] or [D, 3S] (shared)
  const float* gy;       // [N, D]
  const float* gl;       // [N] or null
  float* gx;             // [N, D]
  float* graw;           // [N, D, 3S]; shared: [D, 3S]
  int64_t total;         // N * D
  int64_t N;
  int D, S;
  float mollify, one_m_moll, prescale, one_m_eps, half_eps;
};

// One element: r -> its 3S raw values; emit(k, g_rawA_k, g_rawB_k, g_rawW_k) receives the gradients sigmoid by sigmoid
// (it may write them over r[k], r[S + k], r[2S + k]: those are not read again).  Returns grad_x.
template <class Emit>
__device__ __forceinline__ float ds_backward_element(const DsBwdArgs& a, const float* r, float x, float gy, float gl,
                                                     Emit emit) {
  const int S = a.S;
  const float ps = a.prescale, omm = a.one_m_moll;
  // pass 0: softmax normalisation of the weight logits
  float mw = -INFINITY;
  for (int k = 0; k < S; ++k) mw = fmaxf(mw, r[2 * S + k]);
  float zsum = 0.f;
  for (int k = 0; k < S; ++k) zsum += exp_lean((r[2 * S + k] - mw) * ps);
  const float rz = div_lean(1.f, zsum);
  // pass 1: s, 1 - s and logsumexp(lj)
  float s = 0.f, t = 0.f, m = -1e30f, se = 0.f;
  for (int k = 0; k < S; ++k) {
    const float ra = r[k] * ps;
    const float al = (ra > 20.f ? ra : fmaxf(ra, 0.f) + log1p_lean_pos(exp_lean(-fabsf(ra)))) * omm + a.mollify;
    const float w = exp_lean((r[2 * S + k] - mw) * ps) * rz;
    const float pre = al * x + (r[S + k] * ps) * omm;
    const float e = exp_lean(-fabsf(pre));
    const float rr = div_lean(1.f, 1.f + e);
    const float er = e * rr;
    s += w * (pre >= 0.f ? rr : er);
    t += w * (pre >= 0.f ? er : rr);
    const float lj = log_lean(fmaxf(w * al, 1e-37f)) - fabsf(pre) - 2.f * log1p_lean_pos(e);
    const float d = lj - m;
    const float ex = exp_lean(-fabsf(d));
    se = d > 0.f ? se * ex + 1.f : se + ex;
    m = fmaxf(m, lj);
  }
  const float lse = m + log_lean(se);
  const float c = a.one_m_eps * s + a.half_eps, q = a.one_m_eps * t + a.half_eps;
  const float rc = div_lean(1.f, c), rq = div_lean(1.f, q);
  const float gs = a.one_m_eps * (gy * (rc + rq) + gl * (rq - rc));
  const float sbar = gs * s + gl;                       // sum_k w_k g_w_k
  // pass 2: per-sigmoid adjoints
  float gxs = 0.f;
  for (int k = 0; k < S; ++k) {
    const float ra = r[k] * ps;
    const float ea = exp_lean(-fabsf(ra));
    const float rra = div_lean(1.f, 1.f + ea);
    // F.softplus(threshold=20) and its slope
    const float al = (ra > 20.f ? ra : fmaxf(ra, 0.f) + log1p_lean_pos(ea)) * omm + a.mollify;
    const float dsp = ra > 20.f ? 1.f : (ra >= 0.f ? rra : ea * rra);
    const float w = exp_lean((r[2 * S + k] - mw) * ps) * rz;
    const float pre = al * x + (r[S + k] * ps) * omm;
    const float e = exp_lean(-fabsf(pre));
    const float rr = div_lean(1.f, 1.f + e);
    const float er = e * rr;
    const float sg = pre >= 0.f ? rr : er;
    const float d1 = er * rr;                             // sigmoid'(pre)
    const float lj = log_lean(fmaxf(w * al, 1e-37f)) - fabsf(pre) - 2.f * log1p_lean_pos(e);
    const float pi = exp_lean(fminf(lj - lse, 0.f));
    const float glpi = gl * pi;
    const float g_pre = gs * (w * d1) + glpi * (1.f - 2.f * sg);
    const float g_al = g_pre * x + (al > 0.f ? div_lean(glpi, al) : 0.f);
    gxs += g_pre * al;
    emit(k, g_al * (ps * omm * dsp), g_pre * (ps * omm), ps * (gs * (w * sg) + glpi - w * sbar));
  }
  return gxs;
}

// Per-sample rows.  A wave owns groups of 64 consecutive elements: their raw rows (64 x 3S floats, contiguous in memory)
// come into LDS with coalesced loads, every lane then works on ITS element's row in place (row stride odd: conflict-free
// whatever k the lanes are at), and the gradient rows leave coalesced.
__global__ __launch_bounds__(64) void ds_backward_kernel(DsBwdArgs a, int ts) {
  extern __shared__ float ds_smem[];
  const int S = a.S, P = 3 * S;
  const int lane = threadIdx.x;
  float* tile = ds_smem;
  const int64_t groups = (a.total + 63) / 64;
  for (int64_t grp = blockIdx.x; grp < groups; grp += gridDim.x) {
    const int64_t e0 = grp * 64;
    const int cnt = a.total - e0 < 64 ? (int)(a.total - e0) : 64;
    for (int e = 0; e < cnt; ++e) {
      const float* src = a.raw + (e0 + e) * P;
      for (int k = lane; k < P; k += 64) tile[e * ts + k] = src[k];
    }
    __builtin_amdgcn_wave_barrier();
    if (lane < cnt) {
      const int64_t el = e0 + lane;
      float* row = tile + lane * ts;
      a.gx[el] = ds_backward_element(a, row, a.x[el], a.gy[el], a.gl ? a.gl[el / a.D] : 0.f,
                                     [&](int k, float ga, float gb, float gw) {
                                       row[k] = ga;
                                       row[S + k] = gb;
                                       row[2 * S + k] = gw;
                                     });
    }
    __builtin_amdgcn_wave_barrier();
    for (int e = 0; e < cnt; ++e) {
      float* dst = a.graw + (e0 + e) * P;
      for (int k = lane; k < P; k += 64) dst[k] = tile[e * ts + k];
    }
    __builtin_amdgcn_wave_barrier();
  }
}

// rows too long for the LDS tiles: one thread per element straight on global memory
__global__ __launch_bounds__(256) void ds_backward_direct_kernel(DsBwdArgs a) {
  const int S = a.S, P = 3 * S;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < a.total; e += (int64_t)gridDim.x * blockDim.x) {
    const float* r = a.raw + e * P;
    float* g = a.graw + e * P;
    a.gx[e] = ds_backward_element(a, r, a.x[e], a.gy[e], a.gl ? a.gl[e / a.D] : 0.f,
                                  [&](int k, float ga, float gb, float gw) {
                                    g[k] = ga;
                                    g[S + k] = gb;
                                    g[2 * S + k] = gw;
                                  });
  }
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// One batch-shared row [D, 3S]: its gradient is the sum over the batch.  The row sits in LDS; a wave takes 64 consecutive
// samples and walks the D dims, so that its 64 lanes hold the same (dim, sigmoid) of 64 samples: a butterfly sum, then one
// lane adds the three totals onto the wave's own accumulator row in LDS.  The four accumulator rows are added in wave order
// into row blockIdx.x of `partial`; partial_sum_kernel (fc_partial_sum.h) adds the rows in order.  No atomics: the order
// of every floating-point sum is fixed by (N, D) alone.
__global__ __launch_bounds__(256) void ds_backward_shared_kernel(DsBwdArgs a, float* __restrict__ partial) {
  extern __shared__ float ds_smem[];
  const int S = a.S, P = 3 * S, D = a.D, rowlen = D * P;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float* raw = ds_smem;
  float* acc = ds_smem + (size_t)rowlen * (1 + wave);
  for (int i = threadIdx.x; i < rowlen; i += 256) raw[i] = a.raw[i];
  for (int i = threadIdx.x; i < 4 * rowlen; i += 256) ds_smem[rowlen + i] = 0.f;
  __syncthreads();
  const int64_t groups = (a.N + 63) / 64;
  for (int64_t grp = (int64_t)blockIdx.x * 4 + wave; grp < groups; grp += (int64_t)gridDim.x * 4) {
    const int64_t n = grp * 64 + lane;
    const bool live = n < a.N;
    // a lane past the batch runs with zero upstream gradients: it adds exact zeros
    const float gl = live && a.gl ? a.gl[n] : 0.f;
    for (int j = 0; j < D; ++j) {
      const float x = live ? a.x[n * D + j] : 0.f;
      const float gy = live ? a.gy[n * D + j] : 0.f;
      float* accj = acc + j * P;
      const float gx = ds_backward_element(a, raw + j * P, x, gy, gl, [&](int k, float ga, float gb, float gw) {
        ga = wave_sum(ga);
        gb = wave_sum(gb);
        gw = wave_sum(gw);
        if (lane == 0) {
          accj[k] += ga;
          accj[S + k] += gb;
          accj[2 * S + k] += gw;
        }
      });
      if (live) a.gx[n * D + j] = gx;
    }
  }
  __syncthreads();
  const float* a0 = ds_smem + rowlen;
  for (int i = threadIdx.x; i < rowlen; i += 256)
    partial[(size_t)blockIdx.x * rowlen + i] = ((a0[i] + a0[rowlen + i]) + a0[2 * rowlen + i]) + a0[3 * rowlen + i];
}

inline int ds_shared_rows(int64_t n, int d, int n_sigmoids) {
  const int64_t rowlen = (int64_t)d * 3 * n_sigmoids;
  if (n <= 0 || d <= 0 || n_sigmoids <= 0 || (size_t)(5 * rowlen) * sizeof(float) > kDsSharedMaxLds) return 0;
  const int64_t blocks = ((n + 63) / 64 + 3) / 4;
  return (int)(blocks < kDsSharedMaxGrid ? blocks : kDsSharedMaxGrid);
}

}  // namespace fc

extern "C" int fc_deep_sigmoid_backward_rows(int64_t n, int32_t d, int32_t n_sigmoids) {
  return fc::ds_shared_rows(n, d, n_sigmoids);
}

extern "C" int fc_deep_sigmoid_backward(const float* x, const float* raw, const float* grad_y,
                                        const float* grad_logabsdet, float* grad_x, float* grad_raw, int64_t n,
                                        int32_t d, int32_t n_sigmoids, float mollify, float eps, float prescale,
                                        int32_t shared_params, void* stream) {
  if (n < 0 || d <= 0 || n_sigmoids <= 0) return hipErrorInvalidValue;
  if (!(eps > 0.f && eps < 1.f) || !(mollify >= 0.f && mollify <= 1.f) || !(prescale > 0.f)) return hipErrorInvalidValue;
  if (n == 0) return hipSuccess;
  if (!x || !raw || !grad_y || !grad_x || !grad_raw) return hipErrorInvalidValue;
  fc::DsBwdArgs a{x, raw, grad_y, grad_logabsdet, grad_x, grad_raw, n * (int64_t)d, n, d, n_sigmoids,
                  mollify, 1.f - mollify, prescale, (float)(1.0 - (double)eps), (float)(0.5 * (double)eps)};
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int P = 3 * n_sigmoids;
  if (shared_params) {
    const int rows = fc::ds_shared_rows(n, d, n_sigmoids);
    if (rows <= 0) return hipErrorInvalidConfiguration;      // (the caller expands the row to per-sample rows instead)
    const int rowlen = d * P;
    float* partial = grad_raw + rowlen;
    hipLaunchKernelGGL(fc::ds_backward_shared_kernel, dim3((unsigned)rows), dim3(256), (size_t)5 * rowlen * sizeof(float), s,
                       a, partial);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return fc::launch_partial_sum<float>(partial, grad_raw, rows, rowlen, 1.f, s);
  }
  int ts = P | 1;                      // odd stride (conflict-free per-lane rows)
  const size_t wave_bytes = (size_t)64 * ts * sizeof(float);
  const int per_cu = (int)((size_t)(160 * 1024) / wave_bytes);     // single-wave workgroups: as many as the LDS of a CU holds
  if (per_cu >= 1) {
    static fc::PerDeviceOnce attr;
    const hipError_t ea = fc::ensure_max_dynamic_lds(attr, reinterpret_cast<const void*>(&fc::ds_backward_kernel), 160 * 1024);
    if (ea != hipSuccess) return ea;
    int64_t grid = (a.total + 63) / 64;
    const int64_t cap = (int64_t)fc::device_cu_count() * per_cu;
    if (grid > cap) grid = cap;
    hipLaunchKernelGGL(fc::ds_backward_kernel, dim3((unsigned)grid), dim3(64), wave_bytes, s, a, ts);
    return hipGetLastError();
  }
  int64_t grid = (a.total + 255) / 256;
  const int64_t cap = (int64_t)fc::device_cu_count() * 16;
  if (grid > cap) grid = cap;
  hipLaunchKernelGGL(fc::ds_backward_direct_kernel, dim3((unsigned)grid), dim3(256), 0, s, a);
  return hipGetLastError();
}
