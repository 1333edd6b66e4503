// fc_hidden_route: the launch decisions of fc_hidden_route.h (the functions launch_coupling_tail, dispatch_hidden and
// launch_wide themselves call) readable from the host.  Host code only: no kernel; the only HIP call is the cached CU
// count of the current device (256 without one).
#include "fc_device.h"
#include "fc_hidden_route.h"
#include "../../include/flowcon_hip.h"

extern "C" int fc_hidden_route(int32_t kind, int64_t n, int32_t d, int32_t in_features, int32_t context_features,
                               int32_t num_blocks, int32_t hidden, int64_t* out) {
  if (!out) return hipErrorInvalidValue;
  for (int i = 0; i < 8; ++i) out[i] = 0;
  out[7] = hipErrorInvalidValue;
  if (kind < FC_ROUTE_HIDDEN || kind > FC_ROUTE_HIDDEN_WIDE) return hipErrorInvalidValue;
  // the argument checks of the entry behind each kind (fc_resnet_hidden, fc_resnet_hidden_context,
  // fc_affine_coupling_resnet, fc_resnet_hidden_wide), pointers aside
  if (n < 0 || d <= 0 || num_blocks < 0 || in_features <= 0 || in_features > d) return hipErrorInvalidValue;
  const bool context = kind == FC_ROUTE_HIDDEN_GLU || kind == FC_ROUTE_HIDDEN_ADDITIVE;
  if (context ? context_features <= 0 || context_features > 32 : context_features != 0) return hipErrorInvalidValue;
  const int inputs = in_features + (kind == FC_ROUTE_HIDDEN_GLU ? context_features : 0);
  if (inputs > 64) return hipErrorInvalidValue;
  const int rows = kind == FC_ROUTE_HIDDEN_WIDE ? 64 : 16;
  if (n % rows != 0) return hipErrorInvalidValue;
  if (kind == FC_ROUTE_HIDDEN_WIDE ? (hidden != 128 && hidden != 256) || num_blocks > 16
                                   : hidden != 64 || num_blocks > (kind == FC_ROUTE_HIDDEN ? 4 : 3))
    return hipErrorInvalidValue;
  if (kind == FC_ROUTE_COUPLING_TAIL && d > 128) return hipErrorInvalidValue;
  out[7] = hipSuccess;
  if (n == 0) return hipSuccess;

  const int64_t cus = fc::device_cu_count(), units = n / rows;
  fc::HiddenRoute r;
  if (kind == FC_ROUTE_COUPLING_TAIL)
    r = fc::coupling_tail_route(units, d, num_blocks, in_features > 32 ? 2 : 1, cus);
  else if (kind == FC_ROUTE_HIDDEN_WIDE)
    r = fc::wide_route(units, hidden, cus);
  else
    r = fc::hidden_stack_route(kind == FC_ROUTE_HIDDEN ? 0 : kind == FC_ROUTE_HIDDEN_GLU ? 1 : 2, units, inputs, num_blocks, cus);
  // what one walker takes per pass: a wave a group of r.bpw blocks, a workgroup of the wide kernel a 64-row tile
  const bool tiles = kind == FC_ROUTE_HIDDEN_WIDE;
  const int64_t groups = tiles ? units : (units + r.bpw - 1) / r.bpw;
  const int64_t walkers = tiles ? r.grid : r.grid * fc::kHidWaves;
  out[0] = r.bpw;
  out[1] = r.xvt;
  out[2] = r.grid;
  out[3] = r.grid * fc::kHidWaves;
  out[4] = (int64_t)r.lds;
  out[5] = walkers > 0 ? (groups + walkers - 1) / walkers : 0;
  out[6] = !tiles && r.bpw == 2 && units % 2 != 0;
  out[7] = r.code;
  return r.code;
}
