// Autoregressive INVERSE of a MADE-conditioned layer as one kernel: the D passes run on the device (round 4), gfx950.
//
// The reference's sampling direction (flowcon/transforms/autoregressive/autoregressive.py:44-53) runs D conditioner
// passes, each recomputing all D x P parameters although pass d only fixes column d; rounds 1-3 cut the final-layer and
// bijector work to column d but kept the loop on the HOST: D x (hidden stack + ~5 launches), ~85 us per pass.  Here a wave
// keeps 16 rows for ALL passes:
//
//   * the pre-masked MADE (made.py:205-283: initial layer + residual blocks, masks multiplied into the weights once)
//     sits in LDS as ready-made matrix-core A fragments, exactly the image and the register dataflow of fc_resnet_hidden.hip
//     (products transposed, the C layout of one layer is the B operand of the next, split-f16 with f32 accumulation);
//   * pass d: hidden stack on the columns found so far (the others still zero: they only meet zeroed weights) -> the
//     P final-layer rows of dim d (their fragments stream from L2: 2 KB per 16-row tile, the whole final layer would
//     not fit in LDS) -> the 16 samples' parameters through a wave-private LDS strip to ONE lane per sample -> the
//     element-wise inverse of column d (affine: autoregressive.py:97-129; rational-quadratic spline: :529-621 via
//     RQOp<0>::eval_core, every K and both tail modes) -> the new column goes back into the lanes that feed it to the
//     initial layer of pass d + 1;
//   * the per-column log-determinants add up in the evaluating lane; rows and logabsdet leave once, after pass D - 1.
//
// hidden <= 64 (zero-padded), <= 3 residual blocks, ReLU, D <= 64, P <= 48 parameters per dim (<= 96 for the
// sum-of-sigmoids form, whose final-layer fragments then arrive in two halves).
//
// A context (made.py:153-162 and the blocks' context_layer, the FC_CONTEXT_ADDITIVE form of fc_resnet_hidden_context)
// reaches the stack only through terms that do not change from pass to pass:
//   h  = W0 x + b0 + relu(Wc[0] c + bc[0])                      initial layer
//   h += W2 relu(W1 relu(h) + b1 + Wc[1 + i] c + bc[1 + i]) + b2   block i
// kCtx: the 16 context rows of a block become ONE matrix-core operand (two f16 pieces under their own row scale) before
// pass 0; every pass redoes only the products Wc[l] c for the unit tiles it computes (one k-step per context layer, the
// fragments sit in LDS behind the parameter strips) and adds them where made.py does.  Dim 0 reads no hidden unit, so
// the context never reaches it.  The kernel is shared: fc_made_inverse.hip instantiates it without a context,
// fc_made_inverse_context.hip with one; nothing of the context is left in the former (if constexpr).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>
#include "fc_device.h"
#include "fc_lane.h"
#include "fc_math.h"
#include "fc_mog_op.h"
#include "fc_rq_op.h"
#include "fc_sos_op.h"
#include "fc_spline_ops.h"
#include "fc_split.h"
#include "../../include/flowcon_hip.h"

namespace fc {

constexpr int kMiThreads = 512;
// floats per sample row of the parameter strip (16 per parameter tile + 4: rows 16 bytes apart in banks)
constexpr int mi_strip_row(int pt) { return 16 * pt + 4; }
constexpr size_t mi_lds_bytes(int nb, int k0s, int pt, int bpw) {
  return (size_t)(k0s * 8 + 2 * nb * 16) * 64 * 16 + (1 + 2 * nb) * 64 * 4 + 16 * 4 + (size_t)8 * bpw * 16 * mi_strip_row(pt) * 4;
}
// the context layers behind it: 1 + nb images of [4 tiles][2 pieces] fragments (one k-step: <= 32 context features),
// their biases in accumulator order, their scales
constexpr size_t mi_ctx_lds_bytes(int nb) { return (size_t)(1 + nb) * 8 * 64 * 16 + (1 + nb) * 64 * 4 + 16 * 4; }

struct MadeInvArgs {
  const float* z;           // [N, D] inputs of the inverse
  float* y;                 // [N, D] outputs
  float* lad;               // [N]
  const f16x8* image;       // hidden stack: [layer][ks][t][piece][lane] fragments (accumulator row order)
  const float* image_un;    // [layers]
  const float* image_bias;  // [layers][64], accumulator order
  const f16x8* ffrag;       // final layer: [D][ks 2][PT][piece 2][lane] fragments, rows of tile t = parameters 16 t ..
  const float* fun;         // [D] 2^-S of each dim's rows
  const float* fbias;       // [D][16 PT]
  uint32_t* err;
  const int32_t* need;      // [D] hidden units pass d reads (a prefix of the packed unit order), or null: all 64
  int64_t blocks16;
  int D, P, accumulate;
};

struct MadeInvCtxArgs : MadeInvArgs {
  const float* context;     // [N, C] rows of the context, C <= 32
  const f16x8* cimage;      // context layers: [1 + NB][t 4][piece][lane] fragments, rows in the hidden stack's unit order
  const float* cimage_un;   // [1 + NB]
  const float* cimage_bias; // [1 + NB][64], accumulator order
  int C;
};

// the sampler of a mixture-of-Gaussians MADE (FC_MADE_MOG, nn/nde/made.py:355-388): z is the normal noise, `uniform` picks the
// component of every column, P = 3 c parameters per dim; the [N] output is the log-density of the draw
struct MadeMogNoise {
  const float* uniform;     // [N, D]
  float eps;                // std = softplus(ustd) + eps
  int c;                    // components, <= 16
};
struct MadeMogArgs : MadeInvArgs, MadeMogNoise {};
struct MadeMogCtxArgs : MadeInvCtxArgs, MadeMogNoise {};
constexpr int kMiMog = -1;  // kKind of the mixture column step (the host's FC_MADE_MOG)

// the forms whose stand-alone kernels evaluate an element on a parameter row in LDS (fc_sos_op.h, fc_spline_ops.h: SoSOp,
// LinearSplineOp, QuadraticSplineOp, CubicSplineOp with `inverse` set): the lane's strip row IS such a row (j = 0, d_t = 1),
// so the column step is the op's own prepare (raw conditioner outputs -> derived values, in place; every op writes only
// the P <= 16 PT floats it reads) followed by its eval
template <class Op>
struct MadeFormArgs : MadeInvArgs {
  Op form;
};
constexpr int kMiForm = -2;  // kKind of that column step (the host's FC_MADE_SOS / FC_MADE_SPLINE)
// parameter tiles whose final-layer fragments are requested before the hidden stack; beyond three tiles the rest follows
// once the stack is through (six tiles at once are 96 registers held across the whole stack)
constexpr int mi_first_tiles(int pt) { return pt > 3 ? (pt + 1) / 2 : pt; }

// kind: 0 = affine (P = 2: unconstrained scale, shift), 1 = rational-quadratic spline with a run-time bin count (parameters read
// from the strip as they are needed), 8 / 10 = the same with K = 8 / 10 bins fixed at compile time: the lane copies its 3K -/+ 1
// parameters from its strip and runs the unrolled evaluation of the stand-alone kernels (RQOp<K>::eval_core, two-sided knot walk);
// kMiMog = mixture of Gaussians: inverse-CDF choice of a component on `uniform`, the draw, and the column's log mixture
// density at the draw in the place of the log-determinant (fc_mog_op.h).  Its context enters the initial layer WITHOUT an
// activation (nn/nde/made.py:274-281, unlike transforms/made.py)
// BPW: 16-row blocks a wave carries together -- every pass is a serial chain (five layers, each row maximum -> split ->
// products -> bias), so a second, independent block fills its waits, and each weight fragment read from LDS serves both
// Args: MadeInvArgs, or MadeInvCtxArgs for the conditional form (the context code below is compiled for that one only);
// MadeMogArgs / MadeMogCtxArgs for the mixture sampler
template <int NB, int K0S, int PT, int kKind, int BPW, class Args = MadeInvArgs>
__global__ __launch_bounds__(kMiThreads) __attribute__((amdgpu_waves_per_eu(2, 2))) void made_inverse_kernel(Args a, RQOp<(kKind > 1 ? kKind : 0)> op) {
  constexpr bool kCtx = std::is_base_of<MadeInvCtxArgs, Args>::value;
  constexpr bool kMog = kKind == kMiMog;
  constexpr bool kForm = kKind == kMiForm;
  constexpr int PH = mi_first_tiles(PT);
  constexpr int kLayers = 1 + 2 * NB, kMiPS = mi_strip_row(PT);
  constexpr int kFrag0 = K0S * 4 * 2, kFragL = 2 * 4 * 2, kFrags = kFrag0 + 2 * NB * kFragL;
  extern __shared__ __attribute__((aligned(16))) unsigned char msm[];
  f16x8* wfrag = reinterpret_cast<f16x8*>(msm);
  float* bias = reinterpret_cast<float*>(msm + (size_t)kFrags * 64 * 16);      // [layer][g][16]
  float* wun = bias + kLayers * 64;                                              // [layer] (padded to 16)
  float* strips = wun + 16;                                                      // [8 waves][BPW][16][16 PT + 4]

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int s16 = lane & 15, g = lane >> 4;
  const int D = a.D;
  for (int f = wave; f < kFrags; f += kMiThreads / 64)
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(a.image + (size_t)f * 64 + lane),
                                     (__attribute__((address_space(3))) void*)(wfrag + f * 64), 16, 0, 0);
  for (int i = tid; i < kLayers * 64; i += kMiThreads) bias[i] = a.image_bias[i];
  if (tid < kLayers) wun[tid] = a.image_un[tid];
  // context layers: [layer][t][piece] fragments, [layer][g][16] biases, [layer] scales
  f16x8* cfrag = nullptr;
  float *cbias = nullptr, *cwun = nullptr;
  if constexpr (kCtx) {
    cfrag = reinterpret_cast<f16x8*>(strips + (size_t)(kMiThreads / 64) * BPW * 16 * kMiPS);
    cbias = reinterpret_cast<float*>(cfrag + (1 + NB) * 8 * 64);
    cwun = cbias + (1 + NB) * 64;
    for (int f = wave; f < (1 + NB) * 8; f += kMiThreads / 64)
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(a.cimage + (size_t)f * 64 + lane),
                                       (__attribute__((address_space(3))) void*)(cfrag + f * 64), 16, 0, 0);
    for (int i = tid; i < (1 + NB) * 64; i += kMiThreads) cbias[i] = a.cimage_bias[i];
    if (tid < 1 + NB) cwun[tid] = a.cimage_un[tid];
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  float* strip = strips + (size_t)wave * BPW * 16 * kMiPS;

  // B operand of one layer from this lane's activations v[t][r], t < NT (k = 32 (t >> 1) + 8 g + 4 (t & 1) + r; the
  // tiles beyond NT count as zero): row maximum over the sample's four lanes, power-of-two scale, two f16 pieces
  auto make_operand = [&](auto nt_c, const f32x4 (&v)[4], f16x8 (&bh)[2], f16x8 (&bl)[2]) {
    constexpr int NT = decltype(nt_c)::value;
    float m = 0.f;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) m = fmaxf(m, fabsf(v[t][r]));
    m = rows4_allmax(m, lane);
    float sc, un;
    pow2_scale(m, sc, un);
#pragma unroll
    for (int ks = 0; ks < (NT + 1) / 2; ++ks) {
      u32x4 hh, ll;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        uint32_t ph = 0, pl = 0;
        if (2 * ks + (q >> 1) < NT) split2_pair(v[2 * ks + (q >> 1)][2 * (q & 1)], v[2 * ks + (q >> 1)][2 * (q & 1) + 1], sc, ph, pl);
        hh[q] = ph;
        ll[q] = pl;
      }
      bh[ks] = __builtin_bit_cast(f16x8, hh);
      bl[ks] = __builtin_bit_cast(f16x8, ll);
    }
    return un;
  };
  // a layer's products: NKS k-steps of the operand, the first NTS 16-unit tiles of the outputs
  auto layer = [&](auto nts_c, auto nks_c, int base, const f16x8 (&bh)[BPW][2], const f16x8 (&bl)[BPW][2], f32x4 (&acc)[BPW][4]) {
    constexpr int NTS = decltype(nts_c)::value, NKS = decltype(nks_c)::value;
#pragma unroll
    for (int b = 0; b < BPW; ++b)
#pragma unroll
      for (int t = 0; t < NTS; ++t) acc[b][t] = f32x4{0.f, 0.f, 0.f, 0.f};
    const f16x8* wf = wfrag + base * 64 + lane;
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) {
      f16x8 wl[NTS], wh[NTS];
#pragma unroll
      for (int t = 0; t < NTS; ++t) {
        wl[t] = wf[((ks * 4 + t) * 2 + 1) * 64];
        wh[t] = wf[((ks * 4 + t) * 2 + 0) * 64];
      }
#pragma unroll
      for (int t = 0; t < NTS; ++t)
#pragma unroll
        for (int b = 0; b < BPW; ++b) acc[b][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wl[t], bh[b][ks], acc[b][t], 0, 0, 0);
#pragma unroll
      for (int t = 0; t < NTS; ++t)
#pragma unroll
        for (int b = 0; b < BPW; ++b) acc[b][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh[t], bl[b][ks], acc[b][t], 0, 0, 0);
#pragma unroll
      for (int t = 0; t < NTS; ++t)
#pragma unroll
        for (int b = 0; b < BPW; ++b) acc[b][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh[t], bh[b][ks], acc[b][t], 0, 0, 0);
    }
  };
  auto finish = [&](auto nts_c, int l, float un_act, const f32x4 (&acc)[4], f32x4 (&out)[4]) {
    constexpr int NTS = decltype(nts_c)::value;
    const float c = un_act * wun[l];
    const f32x4* bsrc = reinterpret_cast<const f32x4*>(bias + l * 64 + g * 16);
#pragma unroll
    for (int t = 0; t < NTS; ++t) {
      const f32x4 b = bsrc[t];
#pragma unroll
      for (int r = 0; r < 4; ++r) out[t][r] = __builtin_fmaf(acc[t][r], c, b[r]);
    }
  };
  auto relu_tiles = [&](auto nts_c, const f32x4 (&in)[4], f32x4 (&out)[4]) {
    constexpr int NTS = decltype(nts_c)::value;
#pragma unroll
    for (int t = 0; t < NTS; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) out[t][r] = fmaxf(in[t][r], 0.f);
  };

  uint32_t err = 0;
  const int64_t nwaves = (int64_t)gridDim.x * (kMiThreads / 64);
  const int64_t groups = (a.blocks16 + BPW - 1) / BPW;
  // block b of group grp; the last group of an odd count repeats its first block (computed twice, stored once)
  auto blk_of = [&](int64_t grp, int b) {
    const int64_t blk = grp * BPW + b;
    return blk < a.blocks16 ? blk : a.blocks16 - 1;
  };
#define FC_EACH_BLOCK _Pragma("unroll") for (int b = 0; b < BPW; ++b)
  for (int64_t grp = (int64_t)blockIdx.x * (kMiThreads / 64) + wave; grp < groups; grp += nwaves) {
    asm volatile("" ::: "memory");      // (the weight fragments are loop-invariant LDS loads: do not hoist them)
    const float* zrow[BPW];
    f32x4 xin[BPW][4];                   // the columns found so far, laid out as the initial layer's B operand
    float lad_sum[BPW], znext[BPW];
    FC_EACH_BLOCK {
      zrow[b] = a.z + (blk_of(grp, b) * 16 + s16) * D;
#pragma unroll
      for (int t = 0; t < 4; ++t) xin[b][t] = f32x4{0.f, 0.f, 0.f, 0.f};
      lad_sum[b] = 0.f;
      znext[b] = zrow[b][0];
    }
    [[maybe_unused]] const float* urow[BPW];
    [[maybe_unused]] float unext[BPW];
    if constexpr (kMog) {
      FC_EACH_BLOCK {
        urow[b] = a.uniform + (blk_of(grp, b) * 16 + s16) * D;
        unext[b] = urow[b][0];
      }
    }
    // the block's context rows as one operand (k = 8 g + j < C), under their own row scale
    f16x8 ch[BPW][2], cl[BPW][2];
    float cun[BPW];
    if constexpr (kCtx) {
      FC_EACH_BLOCK {
        const float* crow = a.context + (blk_of(grp, b) * 16 + s16) * a.C;
        f32x4 cv[4];
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
          for (int r = 0; r < 4; ++r) cv[t][r] = 8 * g + 4 * t + r < a.C ? crow[8 * g + 4 * t + r] : 0.f;
        cun[b] = make_operand(std::integral_constant<int, 2>{}, cv, ch[b], cl[b]);
      }
    }
    for (int d = 0; d < D; ++d) {
      asm volatile("" ::: "memory");
      float zval[BPW];
      FC_EACH_BLOCK {
        zval[b] = znext[b];
        znext[b] = zrow[b][d + 1 < D ? d + 1 : d];      // next pass's input, one pass ahead
      }
      [[maybe_unused]] float uval[BPW];
      if constexpr (kMog) {
        FC_EACH_BLOCK {
          uval[b] = unext[b];
          unext[b] = urow[b][d + 1 < D ? d + 1 : d];
        }
      }
      // the final-layer fragments of dim d: requested now, used after the hidden stack
      f16x8 fh[2][PH], fl[2][PH];
      const f16x8* fr = a.ffrag + (size_t)d * 2 * PT * 2 * 64 + lane;
      {
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
#pragma unroll
          for (int t = 0; t < PH; ++t) {
            fh[ks][t] = fr[((ks * PT + t) * 2 + 0) * 64];
            fl[ks][t] = fr[((ks * PT + t) * 2 + 1) * 64];
          }
      }
      const float f_un = a.fun[d];
      // pass d reads `units` hidden units (the packed order puts them first) and the d columns found so far
      const int units = a.need ? __builtin_amdgcn_readfirstlane(a.need[d]) : 64;
      // ---- hidden stack (fc_resnet_hidden.hip's dataflow) on the first NTS 16-unit tiles, then the P final-layer rows of
      // dim d (no activation in front: made.py:281); one copy of the code per tile count, the pass picks its own
      f32x4 pacc[BPW][PT];
      float un[BPW];
      FC_EACH_BLOCK {
        un[b] = 0.f;
#pragma unroll
        for (int t = 0; t < PT; ++t) pacc[b][t] = f32x4{0.f, 0.f, 0.f, 0.f};
      }
      // into[b] += Wc[l] c + bc[l] on the first NTS unit tiles (through ReLU for the initial layer: made.py:157)
      auto add_context = [&](auto nts_c, auto relu_c, int l, f32x4 (&into)[BPW][4]) {
        constexpr int NTS = decltype(nts_c)::value;
        f32x4 cacc[BPW][4];
        {      // `layer` with one k-step on the context operand
          const f16x8* wf = cfrag + l * 8 * 64 + lane;
          f16x8 wl[NTS], wh[NTS];
#pragma unroll
          for (int t = 0; t < NTS; ++t) {
            wl[t] = wf[(t * 2 + 1) * 64];
            wh[t] = wf[(t * 2 + 0) * 64];
          }
#pragma unroll
          for (int t = 0; t < NTS; ++t)
            FC_EACH_BLOCK cacc[b][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wl[t], ch[b][0], f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
#pragma unroll
          for (int t = 0; t < NTS; ++t)
            FC_EACH_BLOCK cacc[b][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh[t], cl[b][0], cacc[b][t], 0, 0, 0);
#pragma unroll
          for (int t = 0; t < NTS; ++t)
            FC_EACH_BLOCK cacc[b][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh[t], ch[b][0], cacc[b][t], 0, 0, 0);
        }
        const f32x4* bsrc = reinterpret_cast<const f32x4*>(cbias + l * 64 + g * 16);
        FC_EACH_BLOCK {
          const float c = cun[b] * cwun[l];
#pragma unroll
          for (int t = 0; t < NTS; ++t) {
            const f32x4 bv = bsrc[t];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const float term = __builtin_fmaf(cacc[b][t][r], c, bv[r]);
              into[b][t][r] += decltype(relu_c)::value ? fmaxf(term, 0.f) : term;
            }
          }
        }
      };
      auto stack = [&](auto nts_c) {
        constexpr int NTS = decltype(nts_c)::value, NKS = (NTS + 1) / 2;
        const std::integral_constant<int, NKS> nks_c;
        f16x8 bh[BPW][2], bl[BPW][2];
        f32x4 acc[BPW][4], h[BPW][4], tmid[BPW][4];
        FC_EACH_BLOCK un[b] = make_operand(std::integral_constant<int, 2 * K0S>{}, xin[b], bh[b], bl[b]);
        layer(nts_c, std::integral_constant<int, K0S>{}, 0, bh, bl, acc);
        FC_EACH_BLOCK finish(nts_c, 0, un[b], acc[b], h[b]);
        if constexpr (kCtx) add_context(nts_c, std::integral_constant<bool, !kMog>{}, 0, h);
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
          FC_EACH_BLOCK {
            f32x4 act[4];
            relu_tiles(nts_c, h[b], act);
            un[b] = make_operand(nts_c, act, bh[b], bl[b]);
          }
          layer(nts_c, nks_c, kFrag0 + (2 * nb) * kFragL, bh, bl, acc);
          if constexpr (kCtx) {
            FC_EACH_BLOCK finish(nts_c, 1 + 2 * nb, un[b], acc[b], tmid[b]);
            add_context(nts_c, std::false_type{}, 1 + nb, tmid);      // made.py:113-114: before the second activation
            FC_EACH_BLOCK {
              f32x4 act[4];
              relu_tiles(nts_c, tmid[b], act);
              un[b] = make_operand(nts_c, act, bh[b], bl[b]);
            }
          } else {
            FC_EACH_BLOCK {
              f32x4 act[4];
              finish(nts_c, 1 + 2 * nb, un[b], acc[b], tmid[b]);
              relu_tiles(nts_c, tmid[b], act);
              un[b] = make_operand(nts_c, act, bh[b], bl[b]);
            }
          }
          layer(nts_c, nks_c, kFrag0 + (2 * nb + 1) * kFragL, bh, bl, acc);
          FC_EACH_BLOCK {
            finish(nts_c, 2 + 2 * nb, un[b], acc[b], tmid[b]);
#pragma unroll
            for (int t = 0; t < NTS; ++t)
#pragma unroll
              for (int r = 0; r < 4; ++r) h[b][t][r] += tmid[b][t][r];
          }
        }
        FC_EACH_BLOCK un[b] = make_operand(nts_c, h[b], bh[b], bl[b]);
        // the other PT - PH tiles' fragments: requested here, multiplied after the first PH
        [[maybe_unused]] f16x8 gh[2][PT > PH ? PT - PH : 1], gl[2][PT > PH ? PT - PH : 1];
        if constexpr (PT > PH) {
#pragma unroll
          for (int ks = 0; ks < NKS; ++ks)
#pragma unroll
            for (int t = PH; t < PT; ++t) {
              gh[ks][t - PH] = fr[((ks * PT + t) * 2 + 0) * 64];
              gl[ks][t - PH] = fr[((ks * PT + t) * 2 + 1) * 64];
            }
        }
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) {
#pragma unroll
          for (int t = 0; t < PH; ++t)
            FC_EACH_BLOCK pacc[b][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fl[ks][t], bh[b][ks], pacc[b][t], 0, 0, 0);
#pragma unroll
          for (int t = 0; t < PH; ++t)
            FC_EACH_BLOCK pacc[b][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fh[ks][t], bl[b][ks], pacc[b][t], 0, 0, 0);
#pragma unroll
          for (int t = 0; t < PH; ++t)
            FC_EACH_BLOCK pacc[b][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fh[ks][t], bh[b][ks], pacc[b][t], 0, 0, 0);
        }
        if constexpr (PT > PH) {
#pragma unroll
          for (int ks = 0; ks < NKS; ++ks) {
#pragma unroll
            for (int t = PH; t < PT; ++t)
              FC_EACH_BLOCK pacc[b][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(gl[ks][t - PH], bh[b][ks], pacc[b][t], 0, 0, 0);
#pragma unroll
            for (int t = PH; t < PT; ++t)
              FC_EACH_BLOCK pacc[b][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(gh[ks][t - PH], bl[b][ks], pacc[b][t], 0, 0, 0);
#pragma unroll
            for (int t = PH; t < PT; ++t)
              FC_EACH_BLOCK pacc[b][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(gh[ks][t - PH], bh[b][ks], pacc[b][t], 0, 0, 0);
          }
        }
      };
      switch ((units + 15) >> 4) {
        case 0: break;                 // no unit feeds this dim (dim 0): its parameters are the final layer's biases
        case 1: stack(std::integral_constant<int, 1>{}); break;
        case 2: stack(std::integral_constant<int, 2>{}); break;
        case 3: stack(std::integral_constant<int, 3>{}); break;
        default: stack(std::integral_constant<int, 4>{}); break;
      }
      // lane (s, g) holds parameters 16 t + 4 g + r of sample s: into the strip, one lane per sample reads them back
      {
        const f32x4* fb = reinterpret_cast<const f32x4*>(a.fbias + (size_t)d * 16 * PT + 4 * g);
        FC_EACH_BLOCK {
          const float c = un[b] * f_un;
#pragma unroll
          for (int t = 0; t < PT; ++t) {
            const f32x4 bv = fb[4 * t];
            *reinterpret_cast<float4*>(strip + (b * 16 + s16) * kMiPS + 16 * t + 4 * g) =
                float4{__builtin_fmaf(pacc[b][t][0], c, bv[0]), __builtin_fmaf(pacc[b][t][1], c, bv[1]),
                       __builtin_fmaf(pacc[b][t][2], c, bv[2]), __builtin_fmaf(pacc[b][t][3], c, bv[3])};
          }
        }
      }
      __builtin_amdgcn_wave_barrier();
      // the element-wise inverse of column d: lane 16 b + s evaluates sample s of block b (BPW <= 4 blocks: every lane group
      // has a block to serve at BPW = 4, the first BPW groups otherwise)
      float yv = 0.f;
      if (g < BPW) {
        const float* p = strip + (g * 16 + s16) * kMiPS;
        float zmine = zval[0];
#pragma unroll
        for (int b = 1; b < BPW; ++b) zmine = g == b ? zval[b] : zmine;
        float ladv;
        if constexpr (kKind == 0) {
          // autoregressive.py:124-128: scale = softplus(p[0]) + 1e-3, shift = p[1]; inverse (x - shift) / scale
          const float sc = softplus_lean(p[0], 1.f) + 1e-3f;
          yv = div_lean(zmine - p[1], sc);
          ladv = -log_lean(sc);
        } else if constexpr (kMog) {
          float umine = uval[0];
#pragma unroll
          for (int b = 1; b < BPW; ++b) umine = g == b ? uval[b] : umine;
          yv = mog_draw(p, a.c, a.eps, zmine, umine);
          // (the density pass reuses the lane's strip row as scratch: the next pass rewrites it)
          ladv = mog_log_density(strip + (g * 16 + s16) * kMiPS, a.c, a.eps, yv);
        } else if constexpr (kForm) {
          // the lane's strip row is private to it: derived parameters in place, then the op's inverse on them
          float* prow = strip + (g * 16 + s16) * kMiPS;
          a.form.prepare(prow, 0, 1);
          a.form.eval(prow, 0, 1, zmine, yv, ladv, err);
        } else {
          static_assert(kKind == 1 || PT == 2, "3K -/+ 1 parameters in two 16-row tiles");
          op.template eval_core<false>(p, zmine, yv, ladv, err);     // K static (8 / 10): the unrolled two-sided walk on the strip
        }
#pragma unroll
        for (int b = 0; b < BPW; ++b) lad_sum[b] += g == b ? ladv : 0.f;
      }
      __builtin_amdgcn_wave_barrier();
      // the new column to the lanes of its sample (lane 16 b + s16 holds it), then into the operand slot of feature d
      const int slot = d & 31;                         // k within its k-step: 8 g' + j
      const bool mine = (slot >> 3) == g;
      const int reg = 8 * (d >> 5) + (slot & 7);       // t = 2 (d >> 5) + ((slot & 7) >> 2), r = slot & 3  ->  4 t + r
      FC_EACH_BLOCK {
        const float yb = __shfl(yv, 16 * b + s16);
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
          for (int r = 0; r < 4; ++r) xin[b][t][r] = (mine && reg == 4 * t + r) ? yb : xin[b][t][r];
      }
    }
    // rows out: lane (s, g) holds columns 32 ks + 8 g + j
    FC_EACH_BLOCK {
      if (grp * BPW + b >= a.blocks16) continue;      // (the repeated block of an odd tail is not stored twice)
      const int64_t row = (grp * BPW + b) * 16 + s16;
      float* yrow = a.y + row * D;
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int c = 32 * (t >> 1) + 8 * g + 4 * (t & 1) + r;
          if ((t >> 1) < K0S && c < D) yrow[c] = xin[b][t][r];
        }
      // the block's log-determinants sit in lane group b
      const float l = __shfl(lad_sum[b], 16 * b + s16);
      if (g == 0) a.lad[row] = a.accumulate ? a.lad[row] + l : l;
    }
  }
#undef FC_EACH_BLOCK
  if (err && a.err) atomicOr(a.err, err);
}

// context form: the instantiations that hold two blocks' context operands next to everything else without spilling
// (kernel-resource-usage of every candidate, DESIGN.md "Conditional device loop")
constexpr bool mi_ctx_pairs_fit_registers(int nb, int k0s, int pt, int kind) {
  return nb == 0 || (k0s == 1 && pt == 1 && kind <= 1);
}

template <class Args>
constexpr bool kMiHasContext = std::is_base_of<MadeInvCtxArgs, Args>::value;
// LDS of an instantiation; the context form carries its layers' images behind the strips
template <class Args>
constexpr size_t mi_total_lds(int nb, int k0s, int pt, int bpw) {
  return mi_lds_bytes(nb, k0s, pt, bpw) + (kMiHasContext<Args> ? mi_ctx_lds_bytes(nb) : 0);
}

// two blocks per wave need their registers: the affine and rational-quadratic forms without a context carry a pair; with a
// context the table above decides, whatever the form (mi_pairs_fit_registers asks it first); see the .hip file's table
// mixture sampler without a context: the pair spills (20-76 bytes of scratch per lane) with two k-steps of inputs (D > 32) and
// one or two blocks at three parameter tiles, or three blocks at two (kernel-resource-usage, DESIGN.md "Mixture-of-Gaussians
// MADE"); with a context the table above holds for it as well
constexpr bool mi_mog_pairs_fit_registers(int nb, int k0s, int pt) {
  return !(k0s == 2 && ((nb >= 1 && pt == 3) || (nb == 3 && pt == 2)));
}
// sum-of-sigmoids and sibling-spline forms: every one-block instantiation is free of scratch; the pair is kept where it is
// too, and dropped where it spills 8-100 bytes per lane (kernel-resource-usage of every candidate, DESIGN.md "Device loop:
// sum-of-sigmoids and sibling splines"; shapes whose pair does not fit the LDS never get here)
template <class Op>
constexpr bool mi_form_pairs_fit_registers(int nb, int k0s, int pt);
template <>
constexpr bool mi_form_pairs_fit_registers<SoSOp>(int nb, int k0s, int pt) {
  return !((pt == 3 && ((k0s == 2 && (nb == 1 || nb == 2)) || (k0s == 1 && nb == 3))) || (pt >= 5 && nb == 1 && k0s == 2) ||
           (pt == 5 && nb == 2 && k0s == 1));
}
template <>
constexpr bool mi_form_pairs_fit_registers<LinearSplineOp>(int nb, int k0s, int pt) {
  return !(k0s == 2 && ((pt == 3 && (nb == 1 || nb == 2)) || (pt == 2 && nb == 3)));
}
template <>
constexpr bool mi_form_pairs_fit_registers<QuadraticSplineOp>(int nb, int k0s, int pt) {
  return !(nb >= 1 && ((k0s == 2 && pt >= 2) || (k0s == 1 && pt == 3 && nb >= 2)));
}
template <>
constexpr bool mi_form_pairs_fit_registers<CubicSplineOp>(int nb, int k0s, int pt) {
  return !(nb >= 1 && ((k0s == 2 && pt >= 2) || (k0s == 1 && pt == 3)));
}
template <class Args>
struct MiFormOf {
  using type = void;
};
template <class Op>
struct MiFormOf<MadeFormArgs<Op>> {
  using type = Op;
};
template <class Args>
constexpr bool mi_pairs_fit_registers(int nb, int k0s, int pt, int kind) {
  if (kMiHasContext<Args>) return mi_ctx_pairs_fit_registers(nb, k0s, pt, kind);
  using Form = typename MiFormOf<Args>::type;
  if constexpr (!std::is_void<Form>::value) return mi_form_pairs_fit_registers<Form>(nb, k0s, pt);
  return kind != kMiMog || mi_mog_pairs_fit_registers(nb, k0s, pt);
}

template <int NB, int K0S, int PT, int kKind, int BPW, class Args>
hipError_t launch_made_inverse_bpw(const Args& a, const RQOp<0>& op, hipStream_t s) {
  constexpr size_t lds = mi_total_lds<Args>(NB, K0S, PT, BPW);
  static_assert(lds <= 160 * 1024, "weight image exceeds the CU's LDS");
  static PerDeviceOnce attr;
  const hipError_t ea =
      ensure_max_dynamic_lds(attr, reinterpret_cast<const void*>(&made_inverse_kernel<NB, K0S, PT, kKind, BPW, Args>), 160 * 1024);
  if (ea != hipSuccess) return ea;
  int64_t grid = device_cu_count();
  const int64_t need = ((a.blocks16 + BPW - 1) / BPW + 7) / 8;
  if (grid > need) grid = need;
  RQOp<(kKind > 1 ? kKind : 0)> opk;       // same fields; the static-K form is the type the unrolled evaluation is written on
  opk.q = op.q;
  opk.inv_beta = op.inv_beta;
  opk.inv_div = op.inv_div;
  hipLaunchKernelGGL((made_inverse_kernel<NB, K0S, PT, kKind, BPW, Args>), dim3((unsigned)grid), dim3(kMiThreads), lds, s, a, opk);
  return hipGetLastError();
}

template <int NB, int K0S, int PT, int kKind, class Args>
hipError_t launch_made_inverse(const Args& a, const RQOp<0>& op, hipStream_t s) {
  // two blocks per wave once every wave of the chip has a pair to carry (small batches: one block per wave fills more CUs)
  // (the pair route is run by tests/test_gpu_ar_sampler_rows.py::test_rows_of_the_two_block_route_against_float64 at this size)
  if constexpr (mi_total_lds<Args>(NB, K0S, PT, 2) <= 160 * 1024 && mi_pairs_fit_registers<Args>(NB, K0S, PT, kKind)) {
    if (a.blocks16 >= 2 * 8 * (int64_t)device_cu_count()) return launch_made_inverse_bpw<NB, K0S, PT, kKind, 2>(a, op, s);
  }
  if constexpr (mi_total_lds<Args>(NB, K0S, PT, 1) <= 160 * 1024) return launch_made_inverse_bpw<NB, K0S, PT, kKind, 1>(a, op, s);
  return hipErrorInvalidValue;       // (context form only: the image does not fit next to its context layers)
}

// ---- the host path of the six entries: form-specific checks, made_args_prepare, (made_context_prepare,) dispatch ---------
// All refusals are hipErrorInvalidValue.  Sizes are checked whatever n is; pointers, and what a configuration says, only when
// there are rows: n == 0 with valid sizes is a success before any of them is looked at.

// the checks all six entries share, at most `max_params` parameters per dim (the form's own limit), and the MadeInvArgs base
// of their arguments; hipSuccess with *run = false: nothing to do (n == 0)
inline hipError_t made_args_prepare(MadeInvArgs& a, const float* z, float* y, float* logabsdet, const void* hidden_frag,
                                    const float* hidden_unscale, const float* hidden_bias, const void* final_frag,
                                    const float* final_unscale, const float* final_bias, const int32_t* units_needed,
                                    uint32_t* err_flag, int64_t n, int32_t d, int32_t num_blocks, int32_t params_per_dim,
                                    int32_t max_params, bool accumulate, bool* run) {
  *run = false;
  if (n < 0 || d < 1 || d > 64 || num_blocks < 0 || num_blocks > 3) return hipErrorInvalidValue;
  if (params_per_dim < 1 || params_per_dim > max_params || n % 16 != 0) return hipErrorInvalidValue;
  if (n == 0) return hipSuccess;
  if (!z || !y || !logabsdet || !hidden_frag || !hidden_unscale || !hidden_bias || !final_frag || !final_unscale || !final_bias)
    return hipErrorInvalidValue;
  if ((((uintptr_t)hidden_frag | (uintptr_t)final_frag | (uintptr_t)final_bias) & 15u) != 0) return hipErrorInvalidValue;
  a = MadeInvArgs{z, y, logabsdet, static_cast<const f16x8*>(hidden_frag), hidden_unscale, hidden_bias,
                  static_cast<const f16x8*>(final_frag), final_unscale, final_bias, err_flag, units_needed, n / 16, d,
                  params_per_dim, accumulate ? 1 : 0};
  *run = true;
  return hipSuccess;
}

// the conditional entries' own arguments, into `a` once made_args_prepare has passed: the size whatever n is, the pointers
// when there are rows (`run`)
inline bool made_context_prepare(MadeInvCtxArgs& a, const float* context, const void* context_frag, const float* context_unscale,
                                 const float* context_bias, int32_t context_features, bool run) {
  if (context_features < 1 || context_features > 32) return false;
  if (run && (!context || !context_frag || !context_unscale || !context_bias || ((uintptr_t)context_frag & 15u) != 0)) return false;
  a.context = context;
  a.cimage = static_cast<const f16x8*>(context_frag);
  a.cimage_un = context_unscale;
  a.cimage_bias = context_bias;
  a.C = context_features;
  return true;
}

// what only fc_made_inverse(_context) check: kind (0 affine, P = 2; 1 rational-quadratic, with its configuration), and the
// spline of that configuration: K <= 16 bins, 3K -/+ 1 parameters per dim
inline bool made_rq_prepare(int32_t kind, int32_t params_per_dim, const fc_rq_config* cfg, int64_t n, RQOp<0>& op) {
  if (kind < 0 || kind > 1 || (kind == 0 && params_per_dim != 2) || (kind == 1 && !cfg)) return false;
  if (kind == 0 || n == 0) return true;
  RQParams& q = op.q;
  q = rq_params_from_config(*cfg, 1);
  if (q.K < 1 || q.K > 16 || params_per_dim != (q.tails ? 3 * q.K - 1 : 3 * q.K + 1)) return false;
  op.inv_div = 1.f / q.wh_div;
  op.inv_beta = 1.f / q.beta;
  return true;
}

// num_blocks x k-steps of the initial layer (two for D > 32): `form(NB, K0S)`, both integral constants, picks the parameter
// tile count and kKind of its form and launches
template <int V>
using MiInt = std::integral_constant<int, V>;
template <class Form>
hipError_t dispatch_made_blocks(int num_blocks, int d, Form&& form) {
  switch (num_blocks) {
    case 0: return d > 32 ? form(MiInt<0>{}, MiInt<2>{}) : form(MiInt<0>{}, MiInt<1>{});
    case 1: return d > 32 ? form(MiInt<1>{}, MiInt<2>{}) : form(MiInt<1>{}, MiInt<1>{});
    case 2: return d > 32 ? form(MiInt<2>{}, MiInt<2>{}) : form(MiInt<2>{}, MiInt<1>{});
    case 3: return d > 32 ? form(MiInt<3>{}, MiInt<2>{}) : form(MiInt<3>{}, MiInt<1>{});
    default: return hipErrorInvalidValue;
  }
}

// the instantiation of kKind with PT .. LAST parameter tiles that holds a.P parameters per dim
template <int NB, int K0S, int PT, int LAST, int kKind, class Args>
hipError_t launch_made_tiles(const Args& a, const RQOp<0>& op, hipStream_t s) {
  if ((a.P + 15) / 16 == PT) return launch_made_inverse<NB, K0S, PT, kKind>(a, op, s);
  if constexpr (PT < LAST) return launch_made_tiles<NB, K0S, PT + 1, LAST, kKind>(a, op, s);
  return hipErrorInvalidValue;
}

// affine / rational-quadratic form (fc_made_inverse.hip, fc_made_inverse_context.hip)
template <class Args>
hipError_t dispatch_made_inverse(const Args& a, const RQOp<0>& op, int num_blocks, int kind, hipStream_t s) {
  return dispatch_made_blocks(num_blocks, a.D, [&](auto nb, auto k0s) {
    constexpr int NB = decltype(nb)::value, K0S = decltype(k0s)::value;
    if (kind == 0) return launch_made_inverse<NB, K0S, 1, 0>(a, op, s);
    if (op.q.K == 8) return launch_made_inverse<NB, K0S, 2, 8>(a, op, s);        // 23 / 25 parameters per dim
    if (op.q.K == 10) return launch_made_inverse<NB, K0S, 2, 10>(a, op, s);      // 29 / 31 (the reference's default bin count)
    return launch_made_tiles<NB, K0S, 1, 3, 1>(a, op, s);
  });
}

// one kKind at FIRST .. LAST parameter tiles: the mixture sampler (kMiMog, 3 c parameters per dim: c <= 5, <= 10, <= 16) and
// the sum-of-sigmoids and sibling-spline forms (kMiForm; one translation unit per form and tile range: compile time)
template <int FIRST, int LAST, int kKind, class Args>
hipError_t dispatch_made_tiles(const Args& a, int num_blocks, hipStream_t s) {
  return dispatch_made_blocks(num_blocks, a.D, [&](auto nb, auto k0s) {
    return launch_made_tiles<decltype(nb)::value, decltype(k0s)::value, FIRST, LAST, kKind>(a, RQOp<0>{}, s);
  });
}

// defined in the translation units that hold the instantiations
hipError_t dispatch_made_sos_wide(const MadeFormArgs<SoSOp>& a, int num_blocks, hipStream_t s);              // PT 4 .. 6
hipError_t dispatch_made_spline_linear(const MadeFormArgs<LinearSplineOp>& a, int num_blocks, hipStream_t s);
hipError_t dispatch_made_spline_quadratic(const MadeFormArgs<QuadraticSplineOp>& a, int num_blocks, hipStream_t s);
hipError_t dispatch_made_spline_cubic(const MadeFormArgs<CubicSplineOp>& a, int num_blocks, hipStream_t s);

}  // namespace fc
