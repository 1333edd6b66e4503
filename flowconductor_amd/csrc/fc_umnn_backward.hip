// Backward of fc_umnn (csrc/fc_umnn.hip) with the integrand MLP recomputed in the kernel, gfx950.
//
//   z = h_0 + (x / 2) sum_i w_i f(t_i, h),  t_i = (x / 2)(s_i + 1),   jac = J = f(x, h),   f = ELU(v) + 1, v = MLP(t, h)
//
// Leibniz' rule, as MonotonicNormalizer._compose states it: the limits of the quadrature are constants, d z / d x = J.
// Given the upstream gradients gz and gj (the caller has folded logabsdet's into gj: gj = gjac +- glad / J), one backward
// pass of the MLP per (element, point) row, seeded with c ELU'(v):
//     point i:       c_i = s (x / 2) w_i            s = gz (forward direction)
//     point t = x:   c   = gj
//     gx = gz J + q,   q = W1[:, 0]^T delta_1 at the point t = x   (= gj df/dt(x, h))
//     gh_k = [k == 0] s + sum_points W1[:, 1 + k]^T delta_1
// Inverse direction (x is the root of F(x) = z, gx comes from upstream): the implicit-function step on the same pass --
// the point t = x runs FIRST and yields q and J, then g = gx + q, gz = g / J and the quadrature points are seeded with
// s = -g / J.  No second root search.
//
// Layout: fc_umnn's.  A wave owns 16 elements, lane (s = lane & 15, g = lane >> 4) belongs to element s and holds the 16
// units 32 (t >> 1) + 8 g + 4 (t & 1) + r of every 64-wide activation; the wave walks the nb_steps + 2 points one at a
// time (the point t = x first; the tables' padding is never walked, so no padded point can be seeded).  Per point:
//   forward    pre + W1[:, 0] t, the hidden layers as three split-f16 v_mfma_f32_16x16x32_f16 terms (fc_split.h), all
//              activations kept in registers (16 per layer and lane)
//   backward   delta_{l-1} = (W_l^T delta_l) [act_{l-1} > 0] with the SAME product routine on a second fragment set (the
//              packing applied to the transposed weights; a transposed layer shares its layer's power-of-two scale)
//   weights    gW_l += delta_l (x) act_{l-1} contracts over rows, which live on lanes: the wave stages (delta^T, act^T) for
//              its 16 elements in LDS [unit][element] and accumulates the sixteen 16 x 16 tiles on the exact-f32 matrix
//              instruction (v_mfma_f32_16x16x4_f32), in registers across the whole launch (fc_resnet_hidden_backward.hip);
//              biases, the t column of W1 and the last layer's row are per-lane f32 sums over the lane's own rows
// The embedding columns of the first layer need only D1 = sum_points delta_1 per element: one W1[:, 1:]^T D1 product
// (-> gh) and one D1 (x) h tile update per element after the point loop.
//
// A lane past the end repeats the last element with gz = gj = 0: every seed, hence every delta, is an exact zero and
// the element is not counted twice.  Zero-padded units have act = 0, so ReLU' masks their delta to an exact zero; zero
// rows of the transposed fragments give the padded embedding slots exact zeros (and nothing is stored for them).
//
// No atomics: the four waves of a workgroup add their sums in wave order into one LDS image, the workgroup stores it as
// row blockIdx.x of the workspace, and a second kernel adds the rows in index order.  gx / gz / gh depend on the lane's
// own element only (per-row scales), so a row of the batch gets the same bits wherever it stands.
//
// One wave per SIMD (launch bounds 256, one workgroup per CU): the three-hidden-layer instantiation keeps 160 tile
// registers and ~100 per-lane sums beside the activation stack (462 registers, 206 of them AGPRs, no scratch), and
// 122 KiB of LDS: both images (80 KiB), the float32 part, and 10 KiB of staging per wave.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>
#include "fc_split.h"
#include "fc_lane.h"
#include "fc_math.h"
#include "fc_device.h"
#include "fc_partial_sum.h"
#include "../../include/flowcon_hip.h"

namespace fc {

constexpr int kUbThreads = 256;
constexpr int kUbWaves = kUbThreads / 64;
constexpr int kUbPoints = FC_UMNN_POINTS;
constexpr int kUbLd = 20;                        // floats per unit row of a staging image (16 elements + padding)

struct UmnnBwdArgs {
  const float* x;       // [total] the input of the forward map, or the root of the inverse
  const float* h;       // [total, cond]
  const f16x8* frag;    // forward image (fc_umnn)
  const float* aux;
  const f16x8* fragt;   // transposed image
  const float* gup;     // [total] gz (forward direction) / gx (inverse)
  const float* gj;      // [total]
  float* gout;          // [total] gx / gz
  float* gh;            // [total, cond]
  float* ws;            // [grid][kParams]
  int64_t total;
  int cond, nb, inverse;
};

// gradient image (include/flowcon_hip.h), natural unit order, widths padded to 64 and the first layer's columns to 32
template <int NL>
struct UmnnGrad {
  static constexpr int kW1 = 0;                          // [64][32]
  static constexpr int kWh = 64 * 32;                    // [NL - 1][64][64]
  static constexpr int kB = kWh + (NL - 1) * 64 * 64;    // [NL][64]
  static constexpr int kWlast = kB + NL * 64;            // [64]
  static constexpr int kBlast = kWlast + 64;             // [1] (+ 3 of padding)
  static constexpr int kParams = kBlast + 4;
};

template <int NL>
struct UmnnBwdImage {
  static constexpr int kFrags = 8 + 16 * (NL - 1);        // forward: fc_umnn's
  static constexpr int kFragsT = 16 * (NL - 1) + 8;       // hidden layers transposed (64 x 64), then W1[:, 1:]^T (32 x 64)
  static constexpr int kBias = 0, kW1t = NL * 64, kWlast = kW1t + 64, kMisc = kWlast + 64, kTt = kMisc + 4,
                       kWw = kTt + kUbPoints, kFloats = kWw + kUbPoints;
  static constexpr size_t kStage = (size_t)kUbWaves * 2 * 64 * kUbLd * 4;
  static constexpr size_t kBytes = (size_t)(kFrags + kFragsT) * 1024 + (size_t)kFloats * 4 + kStage;
};

__device__ __forceinline__ constexpr int ub_feat(int t, int g, int r) { return 32 * (t >> 1) + 8 * g + 4 * (t & 1) + r; }

template <int NL>
__global__ __launch_bounds__(kUbThreads, 1) void umnn_backward_kernel(UmnnBwdArgs a) {
  using I = UmnnBwdImage<NL>;
  using G = UmnnGrad<NL>;
  static_assert((size_t)G::kParams * 4 <= (size_t)(I::kFrags + I::kFragsT) * 1024, "the reduction image reuses the fragments");
  extern __shared__ __attribute__((aligned(16))) unsigned char ubsm[];
  f16x8* wfrag = reinterpret_cast<f16x8*>(ubsm);
  f16x8* wfragt = wfrag + I::kFrags * 64;
  float* aux = reinterpret_cast<float*>(ubsm + (size_t)(I::kFrags + I::kFragsT) * 1024);

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int s16 = lane & 15, g = lane >> 4;
  float* dT = aux + I::kFloats + wave * (2 * 64 * kUbLd);       // this wave's staging images [unit][element]
  float* aT = dT + 64 * kUbLd;
  for (int i = tid; i < I::kFrags * 64; i += kUbThreads) wfrag[i] = a.frag[i];
  for (int i = tid; i < I::kFragsT * 64; i += kUbThreads) wfragt[i] = a.fragt[i];
  for (int i = tid; i < I::kFloats; i += kUbThreads) aux[i] = a.aux[i];
  __syncthreads();

  const float* tt = aux + I::kTt;
  const float* ww = aux + I::kWw;
  const float blast = aux[I::kMisc + 3];
  const int C = a.cond, nb = a.nb;

  // B operand of one 64-wide product from this lane's 16 values v[t][r]: scale by the row maximum, split (fc_umnn.hip)
  auto make_operand = [&](const f32x4 (&v)[4], f16x8 (&bh)[2], f16x8 (&bl)[2]) {
    float m = 0.f;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) m = fmaxf(m, fabsf(v[t][r]));
    m = rows4_allmax(m, lane);
    float sc, un;
    pow2_scale(m, sc, un);
    u32x4 hh[2], ll[2];
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
  // acc = (scaled W) (scaled operand)^T for the first `tiles` 16-row tiles of an image [ks][tile][piece]
  auto layer = [&](const f16x8* image, int base, auto ntiles, auto nksteps, const f16x8 (&bh)[2], const f16x8 (&bl)[2],
                   f32x4 (&acc)[4]) {
    constexpr int NT = decltype(ntiles)::value, NKS = decltype(nksteps)::value;
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    const f16x8* wf = image + base * 64 + lane;
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) {
      f16x8 wl[NT], wh[NT];
#pragma unroll
      for (int t = 0; t < NT; ++t) wl[t] = wf[((ks * NT + t) * 2 + 1) * 64];
#pragma unroll
      for (int t = 0; t < NT; ++t) wh[t] = wf[((ks * NT + t) * 2 + 0) * 64];
#pragma unroll
      for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wl[t], bh[ks], acc[t], 0, 0, 0);
#pragma unroll
      for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh[t], bl[ks], acc[t], 0, 0, 0);
#pragma unroll
      for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh[t], bh[ks], acc[t], 0, 0, 0);
    }
  };
  // dw[16 ot + 4 g + r][16 it + s16] += sum over the wave's 16 elements of dv (unit) * av (unit): the images are staged
  // [unit][element], the contraction index of one instruction is the lane group (elements 4 g + j, j the instruction)
  auto stage = [&](float* img, const f32x4 (&v)[4]) {
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) img[ub_feat(t, g, r) * kUbLd + s16] = v[t][r];
  };
  auto outer = [&](auto in_tiles, auto& dw) {
    constexpr int IT = decltype(in_tiles)::value;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    float4 b4[IT];
#pragma unroll
    for (int it = 0; it < IT; ++it) b4[it] = *reinterpret_cast<const float4*>(aT + (16 * it + s16) * kUbLd + 4 * g);
#pragma unroll
    for (int ot = 0; ot < 4; ++ot) {
      const float4 a4 = *reinterpret_cast<const float4*>(dT + (16 * ot + s16) * kUbLd + 4 * g);
      const float av[4] = {a4.x, a4.y, a4.z, a4.w};
#pragma unroll
      for (int it = 0; it < IT; ++it) {
        const float bv[4] = {b4[it].x, b4[it].y, b4[it].z, b4[it].w};
#pragma unroll
        for (int j = 0; j < 4; ++j)
          dw[ot * IT + it] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[j], bv[j], dw[ot * IT + it], 0, 0, 0);
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  };

  // ---- sums of this wave over the whole launch --------------------------------------------------------------------------
  f32x4 dwh[NL > 1 ? NL - 1 : 1][16];      // hidden layers' tiles [ot][it]
  f32x4 dw1[8];                            // first layer, embedding columns: [ot][it], 32 slots
  f32x4 gb[NL][4], gw1t[4], gwl[4];        // per-lane: biases, W1[:, 0], last row -- unit (t, g, r), summed over this lane's rows
  float gbl = 0.f;
#pragma unroll
  for (int l = 0; l < (NL > 1 ? NL - 1 : 1); ++l)
#pragma unroll
    for (int i = 0; i < 16; ++i) dwh[l][i] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int i = 0; i < 8; ++i) dw1[i] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int t = 0; t < 4; ++t) {
#pragma unroll
    for (int l = 0; l < NL; ++l) gb[l][t] = f32x4{0.f, 0.f, 0.f, 0.f};
    gw1t[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    gwl[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  }

  const int64_t blocks = (a.total + 15) / 16;
  for (int64_t blk = (int64_t)blockIdx.x * kUbWaves + wave; blk < blocks; blk += (int64_t)gridDim.x * kUbWaves) {
    const int64_t e = blk * 16 + s16;
    const bool real = e < a.total;
    const int64_t ec = real ? e : a.total - 1;      // a lane past the end repeats the last element with zero seeds
    const float xin = a.x[ec];
    const float* hrow = a.h + ec * C;
    const float gup = real ? a.gup[ec] : 0.f;
    const float gjv = real ? a.gj[ec] : 0.f;
    const float halfx = 0.5f * xin;

    // ---- once per element: pre = W1[:, 1:] h + b1 (fc_umnn.hip) ---------------------------------------------------------
    f32x4 pre[4];
    float hv[8];
    {
      float m = 0.f;
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
      f16x8 ch[2] = {}, cl[2] = {};
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        _Float16 ph, pl;
        split2(hv[j] * sc, ph, pl);
        ch[0][j] = ph;
        cl[0][j] = pl;
      }
      f32x4 acc0[4];
      layer(wfrag, 0, std::integral_constant<int, 4>{}, std::integral_constant<int, 1>{}, ch, cl, acc0);
      const float c = un * aux[I::kMisc];
      const f32x4* bsrc = reinterpret_cast<const f32x4*>(aux + I::kBias + g * 16);
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const f32x4 b = bsrc[t];
#pragma unroll
        for (int r = 0; r < 4; ++r) pre[t][r] = __builtin_fmaf(acc0[t][r], c, b[r]);
      }
    }

    f32x4 d1sum[4];                          // sum over the points of delta_1
#pragma unroll
    for (int t = 0; t < 4; ++t) d1sum[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    float sseed = 0.f;                       // the quadrature points' common factor, known after the point t = x
    float gres = 0.f;

    // step 0 is the point t = x (table entry nb + 1: t = x, weight 0), steps 1 .. nb + 1 the quadrature points 0 .. nb
    for (int step = 0; step < nb + 2; ++step) {
      // the weight fragments are loop-invariant LDS loads: without this fence the compiler hoists them and spills
      asm volatile("" ::: "memory");
      const int p = step == 0 ? nb + 1 : step - 1;
      const float t = xin * tt[p];
      const float c = step == 0 ? gjv : sseed * halfx * ww[p];

      // ---- forward, every layer's activations kept --------------------------------------------------------------------
      f32x4 act[NL][4];
      {
        const f32x4* w1 = reinterpret_cast<const f32x4*>(aux + I::kW1t + g * 16);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const f32x4 w = w1[q];
#pragma unroll
          for (int r = 0; r < 4; ++r) act[0][q][r] = fmaxf(__builtin_fmaf(w[r], t, pre[q][r]), 0.f);
        }
      }
#pragma unroll
      for (int l = 1; l < NL; ++l) {
        f16x8 bh[2], bl[2];
        f32x4 acc[4];
        const float un = make_operand(act[l - 1], bh, bl);
        layer(wfrag, 8 + 16 * (l - 1), std::integral_constant<int, 4>{}, std::integral_constant<int, 2>{}, bh, bl, acc);
        const float cs = un * aux[I::kMisc + l];
        const f32x4* bsrc = reinterpret_cast<const f32x4*>(aux + I::kBias + l * 64 + g * 16);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const f32x4 b = bsrc[q];
#pragma unroll
          for (int r = 0; r < 4; ++r) act[l][q][r] = fmaxf(__builtin_fmaf(acc[q][r], cs, b[r]), 0.f);
        }
      }
      const f32x4* wlp = reinterpret_cast<const f32x4*>(aux + I::kWlast + g * 16);
      float part = 0.f;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const f32x4 w = wlp[q];
#pragma unroll
        for (int r = 0; r < 4; ++r) part = __builtin_fmaf(act[NL - 1][q][r], w[r], part);
      }
      const float v = rows4_allsum(part, lane) + blast;
      const float ev = exp_lean(fminf(v, 0.f));
      const float fval = v > 0.f ? v + 1.f : ev;          // ELU(v) + 1
      const float seed = c * (v > 0.f ? 1.f : ev);        // c ELU'(v)

      // ---- backward ---------------------------------------------------------------------------------------------------
      f32x4 delta[4];
      if (g == 0) gbl += seed;                            // the four lanes of an element hold the same seed
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const f32x4 w = wlp[q];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          gwl[q][r] = __builtin_fmaf(seed, act[NL - 1][q][r], gwl[q][r]);
          delta[q][r] = act[NL - 1][q][r] > 0.f ? seed * w[r] : 0.f;
        }
      }
#pragma unroll
      for (int l = NL - 1; l >= 1; --l) {
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
          for (int r = 0; r < 4; ++r) gb[l][q][r] += delta[q][r];
        stage(dT, delta);
        stage(aT, act[l - 1]);
        outer(std::integral_constant<int, 4>{}, dwh[l - 1]);
        f16x8 bh[2], bl[2];
        f32x4 acc[4];
        const float un = make_operand(delta, bh, bl);
        layer(wfragt, 16 * (l - 1), std::integral_constant<int, 4>{}, std::integral_constant<int, 2>{}, bh, bl, acc);
        const float cs = un * aux[I::kMisc + l];
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
          for (int r = 0; r < 4; ++r) delta[q][r] = act[l - 1][q][r] > 0.f ? acc[q][r] * cs : 0.f;
      }
      float qpart = 0.f;
      {
        const f32x4* w1 = reinterpret_cast<const f32x4*>(aux + I::kW1t + g * 16);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const f32x4 w = w1[q];
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            gb[0][q][r] += delta[q][r];
            gw1t[q][r] = __builtin_fmaf(delta[q][r], t, gw1t[q][r]);
            d1sum[q][r] += delta[q][r];
            qpart = __builtin_fmaf(w[r], delta[q][r], qpart);
          }
        }
      }
      if (step == 0) {
        const float q = rows4_allsum(qpart, lane);        // gj df/dt(x, h)
        if (!a.inverse) {
          gres = __builtin_fmaf(gup, fval, q);
          sseed = gup;
        } else {
          gres = (gup + q) / fval;
          sseed = -gres;
        }
      }
    }

    // ---- once per element: the embedding columns ------------------------------------------------------------------------
    {
      stage(dT, d1sum);
#pragma unroll
      for (int j = 0; j < 8; ++j) aT[(8 * g + j) * kUbLd + s16] = hv[j];       // slot 0 (t's) holds 0
      outer(std::integral_constant<int, 2>{}, dw1);
      f16x8 bh[2], bl[2];
      f32x4 acc[4];
      const float un = make_operand(d1sum, bh, bl);
      layer(wfragt, 16 * (NL - 1), std::integral_constant<int, 2>{}, std::integral_constant<int, 2>{}, bh, bl, acc);
      const float cs = un * aux[I::kMisc];
      if (real) {
        a.gout[e] = gres;
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int k = 8 * g + 4 * t + r - 1;           // tile t, row 4 g + r of W1[:, 1:]^T is slot 8 g + 4 t + r
            if (k >= 0 && k < C) a.gh[e * C + k] = acc[t][r] * cs + (k == 0 ? sseed : 0.f);
          }
      }
    }
  }

  // ---- this workgroup's sums: the waves add into one image in wave order ------------------------------------------------
  __syncthreads();                                         // the fragments have been read for the last time
  float* red = reinterpret_cast<float*>(ubsm);
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
#pragma unroll
      for (int l = 0; l < NL; ++l) gb[l][t][r] = row16_allsum(gb[l][t][r]);
      gw1t[t][r] = row16_allsum(gw1t[t][r]);
      gwl[t][r] = row16_allsum(gwl[t][r]);
    }
  gbl = row16_allsum(gbl);                                 // lanes g == 0 hold the sums, the other rows zeros
  for (int w = 0; w < kUbWaves; ++w) {
    if (wave == w) {
      auto put = [&](int i, float v) { red[i] = w == 0 ? v : red[i] + v; };
#pragma unroll
      for (int ot = 0; ot < 4; ++ot)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = 16 * ot + 4 * g + r;
#pragma unroll
          for (int it = 0; it < 2; ++it) put(G::kW1 + row * 32 + 16 * it + s16, dw1[ot * 2 + it][r]);
#pragma unroll
          for (int l = 0; l < NL - 1; ++l)
#pragma unroll
            for (int it = 0; it < 4; ++it) put(G::kWh + l * 4096 + row * 64 + 16 * it + s16, dwh[l][ot * 4 + it][r]);
        }
      if (s16 == 0) {
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int u = ub_feat(t, g, r);
#pragma unroll
            for (int l = 0; l < NL; ++l) put(G::kB + l * 64 + u, gb[l][t][r]);
            put(G::kWlast + u, gwl[t][r]);
          }
      }
      if (lane < 4) put(G::kBlast + lane, lane == 0 ? gbl : 0.f);
    }
    __syncthreads();
    if (wave == w && s16 == 0) {                           // column 0 of the first layer: t's (the tiles put zeros there)
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) red[G::kW1 + ub_feat(t, g, r) * 32] += gw1t[t][r];
    }
    __syncthreads();
  }
  float* dst = a.ws + (size_t)blockIdx.x * G::kParams;
  for (int i = tid; i < G::kParams; i += kUbThreads) dst[i] = red[i];
}

static int64_t umnn_backward_grid(int64_t total) {
  const int64_t blocks = (total + 15) / 16;
  const int64_t need = (blocks + kUbWaves - 1) / kUbWaves;
  const int64_t grid = device_cu_count();                  // one workgroup per CU: one wave per SIMD
  return grid < need ? grid : need;
}

static int umnn_grad_params(int hidden_layers) {
  return hidden_layers == 1 ? UmnnGrad<1>::kParams : hidden_layers == 2 ? UmnnGrad<2>::kParams : UmnnGrad<3>::kParams;
}

template <int NL>
hipError_t launch_umnn_backward(const UmnnBwdArgs& a, float* g_params, hipStream_t s) {
  using I = UmnnBwdImage<NL>;
  using G = UmnnGrad<NL>;
  static PerDeviceOnce attr;
  const hipError_t ea = ensure_max_dynamic_lds(attr, reinterpret_cast<const void*>(&umnn_backward_kernel<NL>), 160 * 1024);
  if (ea != hipSuccess) return ea;
  const int64_t grid = umnn_backward_grid(a.total);
  hipLaunchKernelGGL((umnn_backward_kernel<NL>), dim3((unsigned)grid), dim3(kUbThreads), I::kBytes, s, a);
  hipError_t err = hipGetLastError();
  if (err != hipSuccess) return err;
  // the workspace rows added in index order
  return (hipError_t)launch_partial_sum<float>(a.ws, g_params, (int)grid, (int)G::kParams, 1.f, s);
}

}  // namespace fc

extern "C" int fc_umnn_backward_workspace(int64_t n, int32_t d, int32_t hidden_layers) {
  if (n < 0 || d <= 0 || hidden_layers < 1 || hidden_layers > FC_UMNN_MAX_HIDDEN_LAYERS) return -1;
  if (n == 0) return 0;
  return (int)(fc::umnn_backward_grid(n * (int64_t)d) * fc::umnn_grad_params(hidden_layers));
}

extern "C" int fc_umnn_backward(const float* x, const float* h, const void* w_frag, const float* aux, const void* wt_frag,
                                const float* grad_out, const float* grad_jac, float* grad_in, float* grad_h,
                                float* grad_params, float* workspace, int64_t n, int32_t d, int32_t cond_size,
                                int32_t hidden_layers, int32_t nb_steps, int32_t inverse, void* stream) {
  if (n < 0 || d <= 0 || cond_size < 1 || cond_size > FC_UMNN_MAX_COND || hidden_layers < 1 ||
      hidden_layers > FC_UMNN_MAX_HIDDEN_LAYERS || nb_steps < 1 || nb_steps > FC_UMNN_MAX_STEPS)
    return hipErrorInvalidValue;
  if (!grad_params) return hipErrorInvalidValue;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (n == 0) return hipMemsetAsync(grad_params, 0, (size_t)fc::umnn_grad_params(hidden_layers) * 4, s);
  if (!x || !h || !w_frag || !aux || !wt_frag || !grad_out || !grad_jac || !grad_in || !grad_h || !workspace)
    return hipErrorInvalidValue;
  if ((((uintptr_t)w_frag | (uintptr_t)wt_frag) & 15u) != 0) return hipErrorInvalidValue;
  fc::UmnnBwdArgs a{x, h, static_cast<const fc::f16x8*>(w_frag), aux, static_cast<const fc::f16x8*>(wt_frag), grad_out,
                    grad_jac, grad_in, grad_h, workspace, n * (int64_t)d, cond_size, nb_steps, inverse ? 1 : 0};
  switch (hidden_layers) {
    case 1: return fc::launch_umnn_backward<1>(a, grad_params, s);
    case 2: return fc::launch_umnn_backward<2>(a, grad_params, s);
    default: return fc::launch_umnn_backward<3>(a, grad_params, s);
  }
}
