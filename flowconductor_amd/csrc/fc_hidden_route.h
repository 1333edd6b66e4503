// Launch decisions of the hidden-stack kernels (fc_resnet_hidden.hip, fc_resnet_hidden_wide.hip) as host functions: the
// launches call them, and fc_hidden_route (fc_hidden_route.hip) exports them so that a test can ask which route a shape
// takes -- blocks per wave, row pieces per lane, grid, LDS bytes -- without a device.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fc {

constexpr int kHidWaves = 8;                       // waves of a 512-thread workgroup: a wave owns 16-row blocks
constexpr size_t kLdsPerCu = 160 * 1024;

// Bytes of the LDS weight image HiddenLds<NB, K0S, kCtx, kTail> lays out: 1 KB fragments [layer][k-step][tile][piece],
// then bias [layer][64], unscale [16], ids [32 K0S], the build-time reduction scratch [16][8].
constexpr size_t hidden_image_bytes(int nb, int k0s, int ctx, int tail) {
  const int main_layers = 1 + 2 * nb + tail;
  const int ctx_layers = ctx == 1 ? nb : ctx == 2 ? nb + 1 : 0;
  const int frags = k0s * 4 * 2 + (2 * nb + tail) * (2 * 4 * 2) + ctx_layers * (1 * 4 * 2);
  return (size_t)frags * 64 * 16 + (size_t)(main_layers + ctx_layers) * 64 * 4 + 16 * 4 + 32 * k0s * 4 + 16 * 8 * 4;
}

// the coupling-tail kernels add a [16][D | 1] float tile per block and wave behind the image
constexpr size_t tail_lds_bytes(size_t image, int bpw, int D) {
  return ((image + 15) & ~size_t(15)) + (size_t)kHidWaves * bpw * 16 * (D | 1) * 4;
}

constexpr size_t wide_lds_bytes(int H) { return (size_t)2 * 64 * (H + 8) * 2 + 64 * 4 + 2 * 64 * 4 + 64 * 4; }

struct HiddenRoute {
  int bpw = 0;          // 16-row blocks a wave pushes through the layers together (wide: the 4 blocks of a 64-row tile)
  int xvt = 0;          // coupling tail: 16-byte pieces of a 16-row chunk of x a lane keeps in registers
  int64_t grid = 0;     // workgroups
  size_t lds = 0;       // dynamic LDS bytes per workgroup
  hipError_t code = hipSuccess;   // what the launch returns before it launches
};

// One affine coupling layer per launch (launch_coupling_tail): two blocks per wave when there is work for them (>= two
// rounds of single blocks over the chip) and the second row tile fits next to the weight image; one workgroup per CU.
inline HiddenRoute coupling_tail_route(int64_t blocks16, int D, int nb, int k0s, int64_t cus) {
  HiddenRoute r;
  const size_t image = hidden_image_bytes(nb, k0s, 0, 1);
  const bool pairs = blocks16 >= 2 * cus * kHidWaves && tail_lds_bytes(image, 2, D) <= kLdsPerCu &&
                     D <= 64;   // (wider rows: the second block's pieces spill)
  r.bpw = pairs ? 2 : 1;
  // (the two-block kernels carry 2 x XVT row pieces per lane across the layers: instantiated per input width)
  r.xvt = !pairs ? 8 : D <= 32 ? 2 : 4;
  const int64_t units = pairs ? (blocks16 + 1) / 2 : blocks16;
  const int64_t need = (units + kHidWaves - 1) / kHidWaves;
  r.grid = cus < need ? cus : need;
  r.lds = tail_lds_bytes(image, r.bpw, D);
  if (D > 16 * r.xvt) r.code = hipErrorInvalidValue;
  else if (r.lds > kLdsPerCu) r.code = hipErrorInvalidConfiguration;
  return r;
}

// The hidden stack alone (dispatch_hidden): one block per wave; two workgroups per CU when two weight images fit in LDS
// (<= 2 blocks at <= 32 inputs, no context).  `inputs`: operand columns of the initial layer (identity features, plus the
// context features where they are concatenated: kCtx == 1).  `pairs`: probe builds only (FC_HID_FORCE_BPW).
inline HiddenRoute hidden_stack_route(int kCtx, int64_t blocks16, int inputs, int nb, int64_t cus, bool pairs = false) {
  HiddenRoute r;
  const bool wide = inputs > 32;
  const size_t frags = (size_t)(wide ? 16 : 8) + (size_t)nb * (2 * 16 + (kCtx ? 8 : 0));   // 1 KB each
  r.bpw = pairs ? 2 : 1;
  r.grid = cus * (!pairs && !kCtx && frags * 1024 + 2048 <= 80 * 1024 ? 2 : 1);
  const int64_t need = ((pairs ? (blocks16 + 1) / 2 : blocks16) + kHidWaves - 1) / kHidWaves;
  if (r.grid > need) r.grid = need;
  r.lds = hidden_image_bytes(nb, wide ? 2 : 1, kCtx, 0);
  if (nb < 0 || nb > (kCtx ? 3 : 4)) r.code = hipErrorInvalidValue;
  else if (r.lds > kLdsPerCu) r.code = hipErrorInvalidConfiguration;
  return r;
}

// The 128- / 256-wide stack (launch_wide): a workgroup walks 64-row tiles; two workgroups per CU (H = 128: 35 KB of
// activation images each; H = 256: 68 KB each).
inline HiddenRoute wide_route(int64_t tiles, int H, int64_t cus) {
  HiddenRoute r;
  r.bpw = 4;
  r.grid = cus * 2 < tiles ? cus * 2 : tiles;
  r.lds = wide_lds_bytes(H);
  return r;
}

}  // namespace fc
