// Dispatch of the K-generic resident-weight fused final-Linear + RQ-spline kernel (fc_rq_fused4_body.h; one translation
// unit per bin count and tail mode, fc_rq_fused4_<name>.hip).  Called from the general entry (fc_rq_fused_general.hip)
// for these shapes.
#include "fc_rq_fused_general.h"

namespace fc {

// The instances, (bins, has_tails, name): linear tails K = 4..7 and 9..11 -- K = 8 has its own kernel, fc_rq_fused3.hip --, no
// tails K = 4..10; beyond that the weights of 4 dims no longer fit a wave's registers.
#define FC_F4_INSTANCES(X)                                                                        \
  X(4, 1, k4) X(5, 1, k5) X(6, 1, k6) X(7, 1, k7) X(9, 1, k9) X(10, 1, k10) X(11, 1, k11)          \
  X(4, 0, k4_box) X(5, 0, k5_box) X(6, 0, k6_box) X(7, 0, k7_box) X(8, 0, k8_box) X(9, 0, k9_box) X(10, 0, k10_box)

#define FC_F4_DECLARE(bins, has_tails, name)                                                 \
  hipError_t launch_fused4_##name(const RQParams& q, const GenArgs& a, hipStream_t stream); \
  size_t fused4_lds_bytes_##name(int d);
FC_F4_INSTANCES(FC_F4_DECLARE)
#undef FC_F4_DECLARE

// hidden 64, a (bin count, tail mode) with an instance, and the LDS image of the tile fits
bool fused4_takes(const RQParams& q, const GenArgs& a) {
  if (a.H != 64) return false;
#define FC_F4_TAKES(bins, has_tails, name) \
  if (q.K == bins && (q.tails != 0) == (has_tails != 0)) return fused4_lds_bytes_##name(a.D) <= 160 * 1024;
  FC_F4_INSTANCES(FC_F4_TAKES)
#undef FC_F4_TAKES
  return false;
}

hipError_t launch_fused4(const RQParams& q, const GenArgs& a, hipStream_t stream) {
#define FC_F4_LAUNCH(bins, has_tails, name) \
  if (q.K == bins && (q.tails != 0) == (has_tails != 0)) return launch_fused4_##name(q, a, stream);
  FC_F4_INSTANCES(FC_F4_LAUNCH)
#undef FC_F4_LAUNCH
  return hipErrorInvalidValue;
}

}  // namespace fc
