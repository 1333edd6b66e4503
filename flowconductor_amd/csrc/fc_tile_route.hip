// fc_tile_route: the launch decision of fc_tile.h (tile_route, the function launch_tile itself calls) readable from
// the host.  Host code only: no kernel, no HIP call, no device.
#include "fc_tile.h"
#include "../../include/flowcon_hip.h"

extern "C" int fc_tile_route(int64_t n, int32_t d, int32_t d_t, int32_t rowlen, int32_t shared_params,
                             int32_t aligned16, int64_t* out) {
  if (!out || n < 0 || d <= 0 || d_t <= 0 || d_t > d || rowlen <= 0) return hipErrorInvalidValue;
  // plan_tile reads the pointers' low four bits only; these stand-ins are never dereferenced.  Well above zero so that a
  // null logabsdet keeps meaning "none" and the leftover hand-over advances them like real ones.
  const uintptr_t base = (uintptr_t)1 << 40;
  const uintptr_t skew = aligned16 ? 0 : sizeof(float);
  fc::TileArgs a{};
  a.x = reinterpret_cast<const float*>(base + skew);
  a.y = reinterpret_cast<float*>(2 * base + skew);
  a.params = reinterpret_cast<const float*>(3 * base + skew);
  a.N = n; a.D = d; a.d_t = d_t; a.rowlen = rowlen;
  a.shared_params = shared_params ? 1 : 0;
  fc::TileRoute r;
  const hipError_t e = fc::tile_route(a, &r);
  out[0] = r.pf_kind;
  out[1] = r.pf_kind ? r.body_plan.S : 0;
  out[2] = r.pf_kind ? r.full_tiles : 0;
  out[3] = r.pf_kind && r.has_rest ? r.rest.N : 0;
  out[4] = r.has_rest ? (r.rest_plan.vec_ok ? 1 : 2) : 0;
  out[5] = r.has_rest ? r.rest_plan.S : 0;
  out[6] = r.has_rest ? r.rest_plan.grid : 0;
  out[7] = r.has_rest ? r.rest_plan.block : 0;
  return e;
}
