// Unconstrained monotonic neural networks (Wehenkel & Louppe, NeurIPS 2019) as ONE kernel on the f16 matrix cores, gfx950.
//
//   z = h_0 + int_0^x f(t, h) dt,   f = ELU(MLP(t, h)) + 1,   logabsdet = sum_d log f(x, h)
//   (flowcon/transforms/UMNN/MonotonicNormalizer.py:41-82 with the third-party quadrature restated: Clenshaw-Curtis,
//    z = h_0 + (x / 2) sum_i w_i f((x / 2)(s_i + 1), h), nodes and weights from the package's cc_weights)
//
// One scalar x[n, d] costs nb_steps + 2 evaluations of the integrand MLP (defaults 21 -> 50 -> 50 -> 50 -> 1: 22
// evaluations, ~110k multiply-adds against ~90 bytes of traffic).  A "row" of that MLP is one (element, point) pair and
// none of them leaves the chip: a wave owns 16 elements, lane (s = lane & 15, g = lane >> 4) belongs to element s, and
// the wave walks the points kPts at a time -- an MFMA block is "16 elements at one point", so the weighted sum over the
// points is a per-lane accumulation and needs no cross-lane step.
//
// Dataflow of the MLP (fc_resnet_hidden.hip): products transposed (A = weight rows, B = activations^T), three
// v_mfma_f32_16x16x32_f16 terms on two-piece f16 splits with a per-row power-of-two scale (fc_split.h), weight rows in the
// order that makes one layer's accumulator layout the next layer's B operand:
//     tile t, row 4g + r  <->  unit 32 (t >> 1) + 8 g + 4 (t & 1) + r.
// First layer: W1 [t | h] + b1 splits into the part that does not depend on the point, pre = W1[:, 1:] h + b1 -- one
// k-step product per element (the B operand carries 0 in t's slot) -- and one f32 fma per unit and point,
// relu(pre + W1[:, 0] t).  Hidden 64 x 64 layers: 24 MFMAs per block.  Last layer (width -> 1): 16 fmas per lane and
// the sum over the four lanes of a row; ELU + 1.  The Jacobian point t = x goes through the same stack as one more point.
//
// Inverse: the same stack inside a per-element root search.  F(0) = h_0 exactly, so the sign of z - h_0 picks [0, 20] or
// [-20, 0] without an integral; Newton steps with f as the slope, kept inside the bracket (a step that leaves it
// becomes a bisection, or a probe of the bracket's far end while that end has not been evaluated: a target beyond
// F(+-20) returns +-20 after that one probe, where the reference's 25 bisections end within 40 / 2^25 of it).  An element
// stops when its step is below float32 resolution of max(|x|, 1) (or of z through the slope: 4 ulp(z) / f); the wave's
// 16 elements iterate together until all
// have stopped (a stopped element re-evaluates its x: the same values), at most kMaxIter times.  The last evaluation
// is at the returned x and yields -log f(x).
//
// Every lane's result depends on its own element only (the scale of a split is per row), so a row of the batch gives
// the same bits wherever it stands.  The row sums of log f are taken by a second, tiny kernel over the per-element f
// (which the host API returns anyway as `jac`): a fixed order, no atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>
#include "fc_split.h"
#include "fc_lane.h"
#include "fc_math.h"
#include "fc_device.h"
#include "../../include/flowcon_hip.h"

namespace fc {

constexpr int kUmnnThreads = 256;
constexpr int kUmnnPoints = FC_UMNN_POINTS;      // entries of the node / weight tables
constexpr int kUmnnMaxIter = 48;
constexpr float kUmnnBracket = 20.f;

struct UmnnArgs {
  const float* x;      // [total]
  const float* h;      // [total, cond]
  const f16x8* frag;   // weight fragments
  const float* aux;    // biases, t column, last row, unscales, last bias, tables
  float* y;            // [total]
  float* jac;          // [total]
  int64_t total;       // n * d
  int cond, nb, inverse;
};

// image layout (include/flowcon_hip.h)
template <int NL>
struct UmnnImage {
  static constexpr int kFrags = 8 + 16 * (NL - 1);       // 1 KiB each: first layer (one k-step), hidden layers (two)
  static constexpr int kBias = 0;                        // [NL][64] accumulator order
  static constexpr int kW1t = NL * 64;                   // [64]
  static constexpr int kWlast = kW1t + 64;               // [64]
  static constexpr int kMisc = kWlast + 64;              // unscale[3], last bias
  static constexpr int kTt = kMisc + 4;                  // [kUmnnPoints] (s_i + 1) / 2, then 1
  static constexpr int kWw = kTt + kUmnnPoints;          // [kUmnnPoints] w_i, then 0
  static constexpr int kFloats = kWw + kUmnnPoints;
  static constexpr size_t kBytes = (size_t)kFrags * 1024 + (size_t)kFloats * 4;
};

// NL: hidden layers of the integrand (1..3).  kPts: points a wave pushes through the stack together (every weight
// fragment read from LDS serves all of them, and the serial layer chain of one has the other to overlap with).
template <int NL, int kPts>
__global__ __launch_bounds__(kUmnnThreads, 3) void umnn_kernel(UmnnArgs a) {
  using I = UmnnImage<NL>;
  extern __shared__ __attribute__((aligned(16))) unsigned char usmem[];
  f16x8* wfrag = reinterpret_cast<f16x8*>(usmem);
  float* aux = reinterpret_cast<float*>(usmem + (size_t)I::kFrags * 1024);

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int s16 = lane & 15, g = lane >> 4;
  for (int i = tid; i < I::kFrags * 64; i += kUmnnThreads) wfrag[i] = a.frag[i];
  for (int i = tid; i < I::kFloats; i += kUmnnThreads) aux[i] = a.aux[i];
  __syncthreads();

  const float* tt = aux + I::kTt;
  const float* ww = aux + I::kWw;
  const float blast = aux[I::kMisc + 3];
  const int C = a.cond, nb = a.nb;

  // B operand of one 64-wide layer from this lane's 16 activations v[t][r]: scale by the row maximum, split
  auto make_operand = [&](const f32x4 (&v)[4], f16x8 (&bh)[2], f16x8 (&bl)[2]) {
    float m = 0.f;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) m = fmaxf(m, fabsf(v[t][r]));
    m = rows4_allmax(m, lane);
    float sc, un;
    pow2_scale(m, sc, un);
    u32x4 hh[2], ll[2];     // tile t, registers 2p, 2p + 1 -> k-step t >> 1, elements 4 (t & 1) + 2p, + 1
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int p = 0; p < 2; ++p) {
        uint32_t ph, pl;
        split2_pair(v[t][2 * p], v[t][2 * p + 1], sc, ph, pl);
        hh[t >> 1][2 * (t & 1) + p] = ph;
        ll[t >> 1][2 * (t & 1) + p] = pl;
      }
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      bh[ks] = __builtin_bit_cast(f16x8, hh[ks]);
      bl[ks] = __builtin_bit_cast(f16x8, ll[ks]);
    }
    return un;
  };
  // acc[b] = (scaled W) (scaled act_b)^T: three split terms, the small ones first
  auto layer = [&](int base, int nks, auto& bh, auto& bl, auto& acc, auto npts) {
    constexpr int P = decltype(npts)::value;
#pragma unroll
    for (int b = 0; b < P; ++b)
#pragma unroll
      for (int t = 0; t < 4; ++t) acc[b][t] = f32x4{0.f, 0.f, 0.f, 0.f};
    const f16x8* wf = wfrag + base * 64 + lane;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
      if (ks < nks) {
        f16x8 wl[4], wh[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) wl[t] = wf[((ks * 4 + t) * 2 + 1) * 64];
#pragma unroll
        for (int t = 0; t < 4; ++t) wh[t] = wf[((ks * 4 + t) * 2 + 0) * 64];
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
          for (int b = 0; b < P; ++b) acc[b][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wl[t], bh[b][ks], acc[b][t], 0, 0, 0);
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
          for (int b = 0; b < P; ++b) acc[b][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh[t], bl[b][ks], acc[b][t], 0, 0, 0);
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
          for (int b = 0; b < P; ++b) acc[b][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh[t], bh[b][ks], acc[b][t], 0, 0, 0);
      }
  };
  // Linear output of layer l: undo both scalings and add the bias in one fma
  auto finish = [&](int l, float un_act, const f32x4 (&acc)[4], f32x4 (&out)[4]) {
    const float c = un_act * aux[I::kMisc + l];
    const f32x4* bsrc = reinterpret_cast<const f32x4*>(aux + I::kBias + l * 64 + g * 16);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const f32x4 b = bsrc[t];
#pragma unroll
      for (int r = 0; r < 4; ++r) out[t][r] = __builtin_fmaf(acc[t][r], c, b[r]);
    }
  };

  const int64_t blocks = (a.total + 15) / 16;
  for (int64_t blk = (int64_t)blockIdx.x * (kUmnnThreads / 64) + wave; blk < blocks;
       blk += (int64_t)gridDim.x * (kUmnnThreads / 64)) {
    const int64_t e = blk * 16 + s16;
    const bool real = e < a.total;
    const int64_t ec = real ? e : a.total - 1;        // a lane past the end repeats the last element and stores nothing
    const float xin = a.x[ec];
    const float* hrow = a.h + ec * C;
    const float z0 = hrow[0];

    // ---- once per element: pre = W1[:, 1:] h + b1 (k slot 0 is t's: zero here) --------------------------------------
    f32x4 pre[4];
    {
      float hv[8], m = 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int k = 8 * g + j - 1;
        const float v = hrow[(k >= 0 && k < C) ? k : 0];
        hv[j] = (k >= 0 && k < C) ? v : 0.f;
        m = fmaxf(m, fabsf(hv[j]));
      }
      m = rows4_allmax(m, lane);
      float sc, un;
      pow2_scale(m, sc, un);
      f16x8 ch[1][2] = {}, cl[1][2] = {};
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        _Float16 ph, pl;
        split2(hv[j] * sc, ph, pl);
        ch[0][0][j] = ph;
        cl[0][0][j] = pl;
      }
      f32x4 acc0[1][4];
      layer(0, 1, ch, cl, acc0, std::integral_constant<int, 1>{});
      finish(0, un, acc0[0], pre);
    }

    // f at kPts points t[b] of this lane's element
    auto stack = [&](const float (&t)[kPts], float (&f)[kPts]) {
      f32x4 act[kPts][4];
      {
        const f32x4* w1 = reinterpret_cast<const f32x4*>(aux + I::kW1t + g * 16);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const f32x4 w = w1[q];
#pragma unroll
          for (int b = 0; b < kPts; ++b)
#pragma unroll
            for (int r = 0; r < 4; ++r) act[b][q][r] = fmaxf(__builtin_fmaf(w[r], t[b], pre[q][r]), 0.f);
        }
      }
#pragma unroll
      for (int l = 1; l < NL; ++l) {
        f16x8 bh[kPts][2], bl[kPts][2];
        f32x4 acc[kPts][4];
        float un[kPts];
#pragma unroll
        for (int b = 0; b < kPts; ++b) un[b] = make_operand(act[b], bh[b], bl[b]);
        layer(8 + 16 * (l - 1), 2, bh, bl, acc, std::integral_constant<int, kPts>{});
#pragma unroll
        for (int b = 0; b < kPts; ++b) {
          finish(l, un[b], acc[b], act[b]);
#pragma unroll
          for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int r = 0; r < 4; ++r) act[b][q][r] = fmaxf(act[b][q][r], 0.f);
        }
      }
      const f32x4* wl = reinterpret_cast<const f32x4*>(aux + I::kWlast + g * 16);
      float part[kPts];
#pragma unroll
      for (int b = 0; b < kPts; ++b) part[b] = 0.f;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const f32x4 w = wl[q];
#pragma unroll
        for (int b = 0; b < kPts; ++b)
#pragma unroll
          for (int r = 0; r < 4; ++r) part[b] = __builtin_fmaf(act[b][q][r], w[r], part[b]);
      }
#pragma unroll
      for (int b = 0; b < kPts; ++b) {
        const float v = rows4_allsum(part[b], lane) + blast;
        f[b] = v > 0.f ? v + 1.f : exp_lean(v);          // ELU(v) + 1
      }
    };
    // S = sum_i w_i f(xe (s_i + 1) / 2) and fx = f(xe): the nb + 1 nodes and the Jacobian point, kPts at a time (the
    // tables continue with t = xe, weight 0)
    auto eval = [&](float xe, float& S, float& fx) {
      S = 0.f;
      fx = 0.f;
      const int groups = (nb + 2 + kPts - 1) / kPts;
      for (int i = 0; i < groups; ++i) {
        // the weight fragments are loop-invariant LDS loads: without this fence the compiler hoists them and spills
        asm volatile("" ::: "memory");
        float t[kPts], f[kPts];
#pragma unroll
        for (int b = 0; b < kPts; ++b) t[b] = xe * tt[i * kPts + b];
        stack(t, f);
#pragma unroll
        for (int b = 0; b < kPts; ++b) {
          S = __builtin_fmaf(ww[i * kPts + b], f[b], S);
          if (i * kPts + b == nb + 1) fx = f[b];
        }
      }
    };

    float S, fx, out;
    if (!a.inverse) {
      eval(xin, S, fx);
      out = __builtin_fmaf(0.5f * xin, S, z0);
    } else {
      const float target = xin;
      const bool up = target >= z0;
      const float far = up ? kUmnnBracket : -kUmnnBracket;
      float lo = up ? 0.f : -kUmnnBracket, hi = up ? kUmnnBracket : 0.f;
      float xc = fminf(fmaxf(target - z0, lo), hi);          // the slope-1 guess
      bool far_known = false, done = false;
      for (int it = 0; it < kUmnnMaxIter; ++it) {
        eval(xc, S, fx);
        if (!done) {
          const float r = __builtin_fmaf(0.5f * xc, S, z0) - target;
          if (xc == far) {
            far_known = true;
            if (up ? r <= 0.f : r >= 0.f) done = true;        // the target lies beyond F(+-20): the end of the bracket
          }
          if (!done) {
            if (r > 0.f) hi = xc; else lo = xc;
            // F is evaluated in float32: a Newton step below the resolution of x, or below the resolution of z carried
            // through the slope, is evaluation noise.  This test comes before the bracket test -- a search that closes in
            // from one side still has the bracket's far end 20 away, and a noise step across the near end would otherwise
            // be answered with a bisection into that gap.
            const float ax = fmaxf(fabsf(xc), 1.f);
            const float tol = 1.1920929e-7f * fmaxf(ax, fminf(4.f * fmaxf(fabsf(target), fabsf(z0)) / fx, 1024.f * ax));
            float xn = xc - r / fx;
            bool stop = fabsf(xn - xc) <= tol;
            if (!stop) {
              if (!(xn > lo && xn < hi))                       // (a NaN step lands here too)
                xn = (!far_known && (up ? xn >= hi : xn <= lo)) ? far : 0.5f * (lo + hi);
              stop = fabsf(xn - xc) <= tol || hi - lo <= tol;
            }
            if (stop || it == kUmnnMaxIter - 1) done = true;   // xc stays: it is the point that was evaluated
            else xc = xn;
          }
        }
        if (!__any(!done)) break;
      }
      out = xc;
    }
    if (real) {
      a.y[e] = out;
      a.jac[e] = fx;
    }
  }
}

// logabsdet[n] (+)= +-sum_d log jac[n, d]: 16 lanes (one DPP row) per sample, a fixed order
__global__ __launch_bounds__(256) void umnn_logabsdet_kernel(const float* jac, float* lad, int64_t n, int d, int negate,
                                                             int accumulate) {
  const int lane16 = threadIdx.x & 15;
  const int64_t row = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 4;
  const int64_t rc = row < n ? row : n - 1;
  float s = 0.f;
  for (int j = lane16; j < d; j += 16) s += log_lean(jac[rc * d + j]);
  s = row16_allsum(s);
  if (row < n && lane16 == 0) {
    const float v = negate ? -s : s;
    lad[row] = accumulate ? lad[row] + v : v;
  }
}

template <int NL, int kPts>
hipError_t launch_umnn(const UmnnArgs& a, hipStream_t s) {
  using I = UmnnImage<NL>;
  static PerDeviceOnce attr;
  const hipError_t ea = ensure_max_dynamic_lds(attr, reinterpret_cast<const void*>(&umnn_kernel<NL, kPts>), 64 * 1024);
  if (ea != hipSuccess) return ea;
  const int64_t blocks = (a.total + 15) / 16;
  const int64_t need = (blocks + kUmnnThreads / 64 - 1) / (kUmnnThreads / 64);
  int64_t grid = (int64_t)device_cu_count() * 3;      // 42 KiB of LDS and <= 168 registers: three workgroups per CU
  if (grid > need) grid = need;
  hipLaunchKernelGGL((umnn_kernel<NL, kPts>), dim3((unsigned)grid), dim3(kUmnnThreads), I::kBytes, s, a);
  return hipGetLastError();
}

}  // namespace fc

extern "C" int fc_umnn(const float* x, const float* h, const void* w_frag, const float* aux, float* y, float* jac,
                       float* logabsdet, int64_t n, int32_t d, int32_t cond_size, int32_t hidden_layers,
                       int32_t nb_steps, int32_t inverse, int32_t lad_mode, void* stream) {
  if (n < 0 || d <= 0 || cond_size < 1 || cond_size > FC_UMNN_MAX_COND || hidden_layers < 1 ||
      hidden_layers > FC_UMNN_MAX_HIDDEN_LAYERS || nb_steps < 1 || nb_steps > FC_UMNN_MAX_STEPS)
    return hipErrorInvalidValue;
  if (lad_mode < 0 || lad_mode > 3) return hipErrorInvalidValue;
  if (n == 0) return hipSuccess;
  if (!x || !h || !w_frag || !aux || !y || !jac || x == y) return hipErrorInvalidValue;
  if (((uintptr_t)w_frag & 15u) != 0) return hipErrorInvalidValue;
  hipStream_t s = static_cast<hipStream_t>(stream);
  fc::UmnnArgs a{x, h, static_cast<const fc::f16x8*>(w_frag), aux, y, jac, n * (int64_t)d, cond_size, nb_steps,
                 inverse ? 1 : 0};
  hipError_t err;
  switch (hidden_layers) {
    case 1: err = fc::launch_umnn<1, 2>(a, s); break;
    case 2: err = fc::launch_umnn<2, 2>(a, s); break;
    default: err = fc::launch_umnn<3, 2>(a, s); break;
  }
  if (err != hipSuccess || !logabsdet) return err;
  const int64_t grid = (n * 16 + 255) / 256;
  hipLaunchKernelGGL(fc::umnn_logabsdet_kernel, dim3((unsigned)grid), dim3(256), 0, s, jac, logabsdet, n, (int)d,
                     ((lad_mode & 2) ? 1 : 0) ^ (inverse ? 1 : 0), lad_mode & 1);
  return hipGetLastError();
}
