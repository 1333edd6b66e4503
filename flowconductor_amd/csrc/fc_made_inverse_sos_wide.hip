// fc_made_inverse_sos with four to six parameter tiles (S = 16 .. 31; the reference's default S = 30 has 91 parameters per
// dim): the final-layer fragments of a dim arrive in two halves (fc_made_inverse.h, mi_first_tiles).
#include "fc_made_inverse.h"

namespace fc {
hipError_t dispatch_made_sos_wide(const MadeFormArgs<SoSOp>& a, int num_blocks, hipStream_t s) {
  return dispatch_made_tiles<4, 6, kMiForm>(a, num_blocks, s);
}
}  // namespace fc
