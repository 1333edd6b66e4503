// Where the MFMA hooks sit in the straight-line RQ-spline evaluation of the fused final-Linear + spline kernels
// (fc_rq_eval_straight.inc, included by fc_rq_fused3.hip and fc_rq_fused4_body.h).
//
// hipcc's sched_group_barrier pipeline clusters about half of the MFMAs, so the interleave is explicit in the source:
// the evaluation is a sequence of chunks of a few instructions each, hook n issues MFMA number n of the NEXT block and
// pins its position with a sched_barrier, and this plan says after which chunk each hook goes: hook k follows the
// chunk at which the accumulated issue weight first reaches (k + 1) / HOOKS of the total; hooks left over follow the
// last chunk.
#pragma once
#include <hip/hip_runtime.h>
#include <utility>

// Probe builds (tools/probe/search_hooks.sh, build_f4_variants.sh): every hook moves FC_GEN_SHIFT hundredths of a
// hook's share of the weight towards the start of the evaluation.
#ifndef FC_GEN_SHIFT
#define FC_GEN_SHIFT 0
#endif

namespace fc {

template <class F, int... I>
__device__ __forceinline__ void static_for(F&& f, std::integer_sequence<int, I...>) {
  (f(std::integral_constant<int, I>{}), ...);
}

// K bins; HOOKS MFMAs per block; kBox: no tails (K + 1 derivative logits and the domain check).
// kHookReads: hooks may sit among the chunks that read the raw parameters (FC_WH / FC_UD).  A kernel with two
// accumulator sets (fc_rq_fused3.hip) spreads its hooks over the whole evaluation.  With ONE set (fc_rq_fused4_body.h)
// the next block's MFMAs may only start once the last raw parameter has left the accumulators: the reading chunks
// carry no hooks, and the total is taken over the chunks after them.
template <int K, int HOOKS, bool kHookReads, bool kBox>
struct EvalPlan {
  // Sections of the evaluation in order; the chunks of a section are numbered from first(section).
  enum Section {
    sInside, sBoxErr, sMaxInit, sRead, sDer,   // the accumulators are free after the last chunk of sDer
    sMax, sSub, sExp, sSumInit, sSum, sTot, sRcpX, sRcpY, sKnot, sSelect, sBin, sDelta, sTheta,
    sSoftExp, sSoftFix, sSoftLog, sSoftDer,          // softplus of the lower knot's derivative logit ...
    sSoftExp1, sSoftFix1, sSoftLog1, sSoftDer1,      // ... and of the upper knot's: section + 4
    sDsum, sQuadratic, sT1mt, sDn1, sDnum, sLog, sLval, sYs, sOut, kSections
  };
  struct Sec { int count, weight; };   // chunks in the section, VALU issue slots of each
  static constexpr Sec kSecs[kSections] = {
      {1, 3},                 // sInside
      {kBox ? 1 : 0, 1},      // sBoxErr
      {1, 1},                 // sMaxInit
      {K, 3},                 // sRead: one (width, height) logit pair and the running maxima
      {kBox ? K + 1 : K - 1, 1},   // sDer: one derivative logit to the lane's table
      {1, 0},                 // sMax
      {K, 1},                 // sSub
      {K, 4},                 // sExp
      {1, 0},                 // sSumInit
      {K - 2, 1},             // sSum: one addition of the left or the right chain
      {1, 1},                 // sTot
      {1, 5},                 // sRcpX
      {1, 6},                 // sRcpY
      {2 * (K - 1), 2},       // sKnot: per interior knot, fma + store, then the compare-count
      {1, 3}, {1, 2},         // sSelect, sBin
      {1, 5}, {1, 4},         // sDelta, sTheta (forward)
      {1, 6}, {1, 3}, {1, 10}, {1, 3},   // sSoftExp, sSoftFix, sSoftLog, sSoftDer
      {1, 6}, {1, 3}, {1, 10}, {1, 3},   // sSoftExp1 .. sSoftDer1
      {1, 3}, {1, 2},         // sDsum, sQuadratic (inverse)
      {1, 4}, {1, 5}, {1, 4}, // sT1mt, sDn1, sDnum
      {1, 3}, {1, 1},         // sLog, sLval
      {1, 8}, {1, 3},         // sYs, sOut
  };
  static constexpr int first(int section) {
    int c = 0;
    for (int s = 0; s < section; ++s) c += kSecs[s].count;
    return c;
  }
  static constexpr int kChunks = first(kSections);
  static constexpr int weight(int chunk) {
    int s = 0;
    while (chunk >= kSecs[s].count) chunk -= kSecs[s++].count;
    return kSecs[s].weight;
  }
  // number of hooks that precede the end of chunk `chunk` (hooks_until(-1) = 0): the hooks that follow chunk c are
  // hooks_until(c - 1) .. hooks_until(c) - 1.  All in integers: acc / total >= (k + 1 - shift) / HOOKS.
  static constexpr int hooks_until(int chunk) {
    if (chunk == kChunks - 1) return HOOKS;
    const int start = kHookReads ? 0 : first(sMax);
    int total = 0, acc = 0, hook = 0;
    for (int c = start; c < kChunks; ++c) total += weight(c);
    for (int c = start; c <= chunk; ++c) {
      acc += weight(c);
      while (hook < HOOKS && acc * HOOKS * 100 >= ((hook + 1) * 100 - (FC_GEN_SHIFT)) * total) ++hook;
    }
    return hook;
  }
};

}  // namespace fc
