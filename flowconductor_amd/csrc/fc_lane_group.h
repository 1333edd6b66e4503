// The lane-group MLP scaffold: what the kernels share that run a small MLP with forward-mode tangents, whatever the
// layers compute (the continuous-normalizing-flow kernels through fc_cnf.h, the iResBlock kernels in fc_iresblock.hip).
//
// The net is handed over as a packed float32 image that a block copies into LDS once.  A row is carried by a
// power-of-two group of G lanes: lane 0 runs the value stream, lanes 1..d the tangent streams (G == 1: a value stream on
// its own).  The activations sit in LDS as st[k][thread].  Every sum is a float64 fma chain over float4 weight reads,
// rounded once by the caller.  The block is the largest of 256 / 128 / 64 threads that fits the LDS, the grid a capped
// walk over row tiles.  The image layouts and the layer arithmetic are each family's own.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>
#include "fc_device.h"

namespace fc {

__host__ __device__ inline int pad4(int v) { return (v + 3) & ~3; }

// the largest d a group of G lanes carries, and that d rounded up to 4: the length of a lane's register vectors
template <int G>
struct LaneGroup {
  static constexpr int DMAX = G == 32 ? 16 : G - 1;
  static constexpr int DP = (DMAX + 3) & ~3;
};

// The smallest power of two >= d + 1 lanes carry a row: the value stream and d tangents.
inline int lane_group(int d) { return d < 2 ? 2 : d < 4 ? 4 : d < 8 ? 8 : d < 16 ? 16 : 32; }

// f(std::integral_constant<int, N>) for the N of the list that v equals
template <int... Ns, class F>
inline int with_constant(int v, F&& f) {
  int result = hipErrorInvalidConfiguration;
  (void)((v == Ns && ((result = f(std::integral_constant<int, Ns>{})), true)) || ...);
  return result;
}

// Sum over the W lanes of a row group / of a wave, in the fixed order of the butterfly; the same in every lane.
template <int W>
__device__ __forceinline__ double lane_sum(double v) {
#pragma unroll
  for (int off = W / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, W);
  return v;
}

// ---- the block ------------------------------------------------------------------------------------------------------

// Dynamic LDS of every kernel: the image | `mid`, the doubles between (none, a table of the block's, or a strip per
// row) | the state columns st[k][thread], and whatever a kernel keeps behind them.  Lane s of row r of the block.
struct GroupBlock {
  float* img;
  double* mid;
  float* st;
  float* mine;  // st + tid: this lane's entry of a column, the columns T apart
  int T, tid, s, r, rows;
  int64_t tiles;
};

// The set-up in two steps, for a kernel that has something of its own to compute between them (CNF's ping-pong offset):
// where this thread sits ...
template <int G>
__device__ __forceinline__ GroupBlock group_lanes() {
  GroupBlock b;
  b.T = blockDim.x;
  b.tid = threadIdx.x;
  b.s = b.tid % G;
  b.r = b.tid / G;
  b.rows = b.T / G;
  return b;
}

// ... and the LDS carved and the image copy started.  It ends WITHOUT a barrier, which the caller owes before the image
// is read.
__device__ __forceinline__ void group_carve(GroupBlock& b, float* lds, const float* __restrict__ image, int image_floats,
                                            int block_doubles, int row_doubles, int64_t n) {
  b.img = lds;
  b.mid = reinterpret_cast<double*>(lds + image_floats);
  b.st = lds + image_floats + 2 * (block_doubles + b.rows * row_doubles);
  b.mine = b.st + b.tid;
  b.tiles = (n + b.rows - 1) / b.rows;
  for (int i = b.tid; i < image_floats; i += b.T) b.img[i] = image[i];
}

template <int G>
__device__ __forceinline__ GroupBlock group_block(float* lds, const float* __restrict__ image, int image_floats,
                                                  int block_doubles, int row_doubles, int64_t n) {
  GroupBlock b = group_lanes<G>();
  group_carve(b, lds, image, image_floats, block_doubles, row_doubles, n);
  return b;
}

// The row of this lane's group in `tile`.  A group past the end runs along on the last row (the shuffles, and the
// barriers where a kernel has them, need every lane); only live rows are stored.
__device__ __forceinline__ int64_t tile_row(const GroupBlock& b, int64_t tile, int64_t n, bool& live) {
  const int64_t row = tile * b.rows + b.r;
  live = row < n;
  return live ? row : n - 1;
}

// ---- the sum of a hidden layer ---------------------------------------------------------------------------------------

// sum[c] = (value ? bias(o + c) : 0) + sum_k wt[k][o + c] x[k], c < 4: a hidden layer's outputs o .. o + 3 on the
// column x (stride T), the weights in rows of op floats.  A tangent stream has no bias.
template <class Bias>
__device__ __forceinline__ void weight_sum4(const float* wt, const float* x, int T, int in, int op, int o, bool value,
                                            Bias bias, double (&sum)[4]) {
#pragma unroll
  for (int c = 0; c < 4; ++c) sum[c] = value ? bias(o + c) : 0.0;
  for (int k = 0; k < in; ++k) {
    const double v = (double)x[k * T];
    const float4 w4 = *reinterpret_cast<const float4*>(wt + k * op + o);
    sum[0] = fma((double)w4.x, v, sum[0]);
    sum[1] = fma((double)w4.y, v, sum[1]);
    sum[2] = fma((double)w4.z, v, sum[2]);
    sum[3] = fma((double)w4.w, v, sum[3]);
  }
}

// ---- launch ---------------------------------------------------------------------------------------------------------

constexpr int kGroupLdsLimit = 128 * 1024;
constexpr int kGroupMaxBlocks = 2048;
constexpr int kGroupBackwardMaxBlocks = 256;  // a block of a backward kernel owns an image-shaped partial

// What a kernel keeps in dynamic LDS besides the image.
struct GroupLds {
  size_t block_bytes;  // once per block
  int thread_floats;   // per thread: the state columns
  int row_doubles;     // per row
  int wave_doubles;    // per wave of 64 threads
};

enum GroupFit {
  kPrefer64K,     // the largest block within 64 KiB, else the smallest block if it fits the limit
  kLargestBlock,  // the largest block that fits the limit
};

struct GroupLaunch {
  int threads;  // 0: not even the smallest block fits kGroupLdsLimit
  size_t lds;
  int64_t grid;
};

// Blocks of 256, 128 or 64 threads, a block per tile of threads / group rows up to max_blocks.
inline GroupLaunch group_launch_plan(int image_floats, int group, const GroupLds& need, GroupFit fit, int64_t n,
                                     int max_blocks) {
  const size_t aim = fit == kPrefer64K ? 64 * 1024 : (size_t)kGroupLdsLimit;
  GroupLaunch plan{256, 0, 0};
  for (;; plan.threads >>= 1) {
    plan.lds = sizeof(float) * ((size_t)image_floats + (size_t)need.thread_floats * plan.threads) + need.block_bytes +
               sizeof(double) * ((size_t)need.row_doubles * (size_t)(plan.threads / group) +
                                 (size_t)need.wave_doubles * (size_t)(plan.threads / 64));
    if (plan.lds <= aim || plan.threads <= 64) break;
  }
  if (plan.lds > (size_t)kGroupLdsLimit) plan.threads = 0;
  const int rows = plan.threads ? plan.threads / group : 1;
  const int64_t tiles = (n + rows - 1) / rows;
  plan.grid = tiles < max_blocks ? tiles : max_blocks;
  return plan;
}

// Raises the kernel's dynamic-LDS limit once per device and launches it.
template <auto Kernel, class... Args>
inline int group_launch(const GroupLaunch& plan, hipStream_t s, Args... args) {
  if (!plan.threads) return hipErrorInvalidConfiguration;
  static PerDeviceOnce once;
  const hipError_t e = ensure_max_dynamic_lds(once, reinterpret_cast<const void*>(Kernel), kGroupLdsLimit);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(Kernel, dim3((unsigned)plan.grid), dim3(plan.threads), plan.lds, s, args...);
  return hipGetLastError();
}

}  // namespace fc
