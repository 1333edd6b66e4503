// fc_made_inverse_spline, piecewise-quadratic form: its instantiations of fc_made_inverse.h (kMiForm on QuadraticSplineOp).
#include "fc_made_inverse.h"

namespace fc {
hipError_t dispatch_made_spline_quadratic(const MadeFormArgs<QuadraticSplineOp>& a, int num_blocks, hipStream_t s) {
  return dispatch_made_tiles<1, 3, kMiForm>(a, num_blocks, s);
}
}  // namespace fc
