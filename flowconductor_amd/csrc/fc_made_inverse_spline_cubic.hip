// fc_made_inverse_spline, piecewise-cubic form: its instantiations of fc_made_inverse.h (kMiForm on CubicSplineOp).
#include "fc_made_inverse.h"

namespace fc {
hipError_t dispatch_made_spline_cubic(const MadeFormArgs<CubicSplineOp>& a, int num_blocks, hipStream_t s) {
  return dispatch_made_tiles<1, 3, kMiForm>(a, num_blocks, s);
}
}  // namespace fc
