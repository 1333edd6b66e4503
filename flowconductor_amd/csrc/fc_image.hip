// Layers of flows on images (reference flowcon/transforms/reshape.py and conv.py).
//
//   fc_squeeze   [B, C, H, W] <-> [B, C f^2, H/f, W/f] in the order of the reference's
//                view(B, C, H/f, f, W/f, f).permute(0, 1, 3, 5, 2, 4); bit-exact (pure data movement)
//   fc_conv1x1   per image Y[C, HW] = M[C, C] (X[C, HW] - pre) + post, NCHW in and out (OneByOneConvolution)
//
// Squeeze: one input channel plane [H, W] becomes f^2 consecutive output planes [H/f, W/f], so plane p of the input and
// the f^2 output planes of p cover the same H W floats at the same offset.  A block owns R output rows of one plane:
// on the "plane side" that is one contiguous run of R f W floats, on the "squeezed side" f^2 contiguous runs of R W/f
// floats.  A plane that fits the tile whole goes with its neighbours: the block owns np consecutive planes.  The
// contiguous side is copied through an LDS tile with 16-byte accesses; the other side is gathered from (forward) or
// scattered into (inverse) the tile, one 16-byte piece per lane across all its runs, so both HBM streams stay
// coalesced.  The inverse is the same kernel
// with the two sides swapped, and each direction is the other's backward.
//
// 1x1 convolution: a thread owns 4 consecutive pixels of one image (one 16-byte access per channel when HW % 4 == 0)
// and CO = 4/8/16/24/32 output channels; the block stages the CO rows of M it needs in LDS as [C][CO] (one broadcast ds_read_b128 per 4
// weights).  The sum over input channels is one f32 fma chain in channel order; "pre" is subtracted from x before the
// product (the inverse's x - b), "post" is added after it (the forward's bias).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/flowcon_hip.h"

namespace fc {

constexpr int kImageThreads = 256;
constexpr int kSqueezeTileFloats = 4096;  // 16 KiB of LDS per block in the common case

// MODE 0: src = plane side [planes][H][W], dst = squeezed side [planes][f f][H/f][W/f]; MODE 1: the other way.
// A block owns R output rows of one plane, or np whole consecutive planes when a plane fits the tile (tiles == 1).
// F > 0: the factor as a compile-time constant (2, 3, 4); F == 0 reads it from f_rt.
template <int MODE, int F>
__global__ __launch_bounds__(kImageThreads) void squeeze_kernel(const float* __restrict__ src, float* __restrict__ dst,
                                                                int64_t planes, int h, int w, int f_rt, int rows,
                                                                int tiles, int np) {
  extern __shared__ __attribute__((aligned(16))) float tile[];
  const int f = F > 0 ? F : f_rt;
  const int ho = h / f, wo = w / f, ff = f * f;
  const int64_t group = blockIdx.x / tiles;
  const int64_t plane0 = group * np;
  const int np_eff = (int)(planes - plane0 < np ? planes - plane0 : np);
  const int i0 = (int)(blockIdx.x - group * tiles) * rows;
  const int r_eff = ho - i0 < rows ? ho - i0 : rows;
  const int64_t hw = (int64_t)h * w;
  const int pcount = r_eff * f * w;     // floats of one plane's part of the tile
  const int count = np_eff * pcount;    // floats of the tile
  const int seg = r_eff * wo;           // floats of one squeezed-side run
  // plane side: one contiguous run of `count` floats (np_eff > 1 only for whole planes)
  const int64_t run = plane0 * hw + (int64_t)i0 * f * w;
  // squeezed side: run (pl, s = a f + b) starts at (plane0 + pl) h w + s ho wo + i0 wo; all runs are 16-byte aligned
  // when the first one is and both seg and ho wo are multiples of 4
  const float* sq_src = MODE == 1 ? src : nullptr;
  float* sq_dst = MODE == 0 ? dst : nullptr;
  const int64_t sq0 = plane0 * hw + (int64_t)i0 * wo;
  const bool sq_vec = seg % 4 == 0 && (ho * wo) % 4 == 0 &&
                      ((((uintptr_t)(MODE == 0 ? (const float*)(sq_dst + sq0) : sq_src + sq0)) & 15u) == 0);
  const int per_seg = sq_vec ? seg >> 2 : seg;
  const int units = np_eff * ff * per_seg;

  if (MODE == 0) {
    const float* p = src + run;
    const bool vec = ((((uintptr_t)p) & 15u) == 0);
    const int nvec = vec ? count >> 2 : 0;
    for (int i = threadIdx.x; i < nvec; i += kImageThreads)
      reinterpret_cast<float4*>(tile)[i] = reinterpret_cast<const float4*>(p)[i];
    for (int i = (nvec << 2) + threadIdx.x; i < count; i += kImageThreads) tile[i] = p[i];
  } else {
    for (int u = threadIdx.x; u < units; u += kImageThreads) {
      const int sid = u / per_seg, k = u - sid * per_seg;
      const int pl = sid / ff, s = sid - pl * ff;
      const int a = s / f, b = s - a * f;
      const float* p = sq_src + sq0 + (int64_t)pl * hw + (int64_t)s * ho * wo;
      float* t = tile + pl * pcount;
      if (sq_vec) {
        const float4 v = reinterpret_cast<const float4*>(p)[k];
        const float* vp = reinterpret_cast<const float*>(&v);
        int e = k << 2, r = e / wo, j = e - r * wo;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          t[(r * f + a) * w + j * f + b] = vp[q];
          if (++j == wo) { j = 0; ++r; }
        }
      } else {
        const int r = k / wo, j = k - r * wo;
        t[(r * f + a) * w + j * f + b] = p[k];
      }
    }
  }
  __syncthreads();
  if (MODE == 0) {
    for (int u = threadIdx.x; u < units; u += kImageThreads) {
      const int sid = u / per_seg, k = u - sid * per_seg;
      const int pl = sid / ff, s = sid - pl * ff;
      const int a = s / f, b = s - a * f;
      float* p = sq_dst + sq0 + (int64_t)pl * hw + (int64_t)s * ho * wo;
      const float* t = tile + pl * pcount;
      if (sq_vec) {
        float4 v;
        float* vp = reinterpret_cast<float*>(&v);
        int e = k << 2, r = e / wo, j = e - r * wo;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          vp[q] = t[(r * f + a) * w + j * f + b];
          if (++j == wo) { j = 0; ++r; }
        }
        reinterpret_cast<float4*>(p)[k] = v;
      } else {
        const int r = k / wo, j = k - r * wo;
        p[k] = t[(r * f + a) * w + j * f + b];
      }
    }
  } else {
    float* p = dst + run;
    const bool vec = ((((uintptr_t)p) & 15u) == 0);
    const int nvec = vec ? count >> 2 : 0;
    for (int i = threadIdx.x; i < nvec; i += kImageThreads)
      reinterpret_cast<float4*>(p)[i] = reinterpret_cast<const float4*>(tile)[i];
    for (int i = (nvec << 2) + threadIdx.x; i < count; i += kImageThreads) p[i] = tile[i];
  }
}

// Planes too wide for one LDS row block (f W > 16384): a direct element-wise gather, still bit-exact.
template <int MODE>
__global__ __launch_bounds__(kImageThreads) void squeeze_direct_kernel(const float* __restrict__ src,
                                                                       float* __restrict__ dst, int64_t total, int h,
                                                                       int w, int f) {
  const int ho = h / f, wo = w / f;
  const int64_t hw = (int64_t)h * w;
  const int64_t stride = (int64_t)gridDim.x * kImageThreads;
  for (int64_t e = (int64_t)blockIdx.x * kImageThreads + threadIdx.x; e < total; e += stride) {
    const int64_t plane = e / hw;
    const int64_t q = e - plane * hw;  // index on the squeezed side: (s, i, j)
    const int s = (int)(q / ((int64_t)ho * wo));
    const int64_t ij = q - (int64_t)s * ho * wo;
    const int i = (int)(ij / wo), j = (int)(ij - (int64_t)i * wo);
    const int a = s / f, b = s - a * f;
    const int64_t pl = plane * hw + (int64_t)(i * f + a) * w + (int64_t)j * f + b;
    if (MODE == 0)
      dst[e] = src[pl];
    else
      dst[pl] = src[e];
  }
}

template <int CO, bool VEC>
__global__ __launch_bounds__(kImageThreads) void conv1x1_kernel(const float* __restrict__ x,
                                                                const float* __restrict__ m,
                                                                const float* __restrict__ pre,
                                                                const float* __restrict__ post, float* __restrict__ y,
                                                                int64_t quads, int64_t nq, int c, int64_t hw,
                                                                int groups) {
  extern __shared__ __attribute__((aligned(16))) float wt[];  // [c][CO]: wt[k CO + o] = m[(g CO + o) c + k]
  const int g = blockIdx.x % groups;
  const int64_t tile = blockIdx.x / groups;
  for (int i = threadIdx.x; i < c * CO; i += kImageThreads) {
    const int k = i / CO, o = i - k * CO, row = g * CO + o;
    wt[i] = row < c ? m[(int64_t)row * c + k] : 0.f;
  }
  __syncthreads();
  const int64_t q = tile * kImageThreads + threadIdx.x;
  if (q >= quads) return;
  const int64_t b = q / nq;
  const int64_t p0 = (q - b * nq) * 4;
  const float* xb = x + b * c * hw + p0;
  float acc[CO][4];
#pragma unroll
  for (int o = 0; o < CO; ++o)
#pragma unroll
    for (int u = 0; u < 4; ++u) acc[o][u] = 0.f;
  const int valid = VEC ? 4 : (int)(hw - p0 < 4 ? hw - p0 : 4);
#pragma unroll 2
  for (int k = 0; k < c; ++k) {
    float v[4];
    if (VEC) {
      const float4 t = *reinterpret_cast<const float4*>(xb + (int64_t)k * hw);
      v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u] = u < valid ? xb[(int64_t)k * hw + u] : 0.f;
    }
    const float sub = pre ? pre[k] : 0.f;
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = v[u] - sub;
    const float4* wk = reinterpret_cast<const float4*>(wt + k * CO);
#pragma unroll
    for (int o4 = 0; o4 < CO / 4; ++o4) {
      const float4 wv = wk[o4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        acc[4 * o4 + 0][u] = fmaf(wv.x, v[u], acc[4 * o4 + 0][u]);
        acc[4 * o4 + 1][u] = fmaf(wv.y, v[u], acc[4 * o4 + 1][u]);
        acc[4 * o4 + 2][u] = fmaf(wv.z, v[u], acc[4 * o4 + 2][u]);
        acc[4 * o4 + 3][u] = fmaf(wv.w, v[u], acc[4 * o4 + 3][u]);
      }
    }
  }
  float* yb = y + b * c * hw + p0;
#pragma unroll
  for (int o = 0; o < CO; ++o) {
    const int row = g * CO + o;
    if (row >= c) break;
    const float add = post ? post[row] : 0.f;
    float* dst = yb + (int64_t)row * hw;
    if (VEC) {
      *reinterpret_cast<float4*>(dst) =
          make_float4(acc[o][0] + add, acc[o][1] + add, acc[o][2] + add, acc[o][3] + add);
    } else {
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (u < valid) dst[u] = acc[o][u] + add;
    }
  }
}

template <int CO>
static int launch_conv1x1(const float* x, const float* m, const float* pre, const float* post, float* y,
                          int64_t batch, int c, int64_t hw, hipStream_t s) {
  const int64_t nq = (hw + 3) / 4;
  const int64_t quads = batch * nq;
  const int groups = (c + CO - 1) / CO;
  const int64_t grid = (quads + kImageThreads - 1) / kImageThreads * groups;
  if (grid > 0x7fffffffLL) return hipErrorInvalidConfiguration;
  const size_t lds = sizeof(float) * (size_t)c * CO;
  const bool vec = hw % 4 == 0 && ((((uintptr_t)x) | ((uintptr_t)y)) & 15u) == 0;
  if (vec)
    hipLaunchKernelGGL((conv1x1_kernel<CO, true>), dim3((unsigned)grid), dim3(kImageThreads), lds, s, x, m, pre, post,
                       y, quads, nq, c, hw, groups);
  else
    hipLaunchKernelGGL((conv1x1_kernel<CO, false>), dim3((unsigned)grid), dim3(kImageThreads), lds, s, x, m, pre,
                       post, y, quads, nq, c, hw, groups);
  return hipGetLastError();
}

template <int F>
static int launch_squeeze_f(const float* x, float* y, int64_t planes, int h, int w, int f, int rows, int tiles, int np,
                            int mode, int64_t grid, size_t lds, hipStream_t s) {
  if (mode == 0)
    hipLaunchKernelGGL((squeeze_kernel<0, F>), dim3((unsigned)grid), dim3(kImageThreads), lds, s, x, y, planes, h, w, f,
                       rows, tiles, np);
  else
    hipLaunchKernelGGL((squeeze_kernel<1, F>), dim3((unsigned)grid), dim3(kImageThreads), lds, s, x, y, planes, h, w, f,
                       rows, tiles, np);
  return hipGetLastError();
}

static int launch_squeeze(const float* x, float* y, int64_t planes, int h, int w, int f, int rows, int tiles, int np,
                          int mode, int64_t grid, size_t lds, hipStream_t s) {
  switch (f) {
    case 2: return launch_squeeze_f<2>(x, y, planes, h, w, f, rows, tiles, np, mode, grid, lds, s);
    case 3: return launch_squeeze_f<3>(x, y, planes, h, w, f, rows, tiles, np, mode, grid, lds, s);
    case 4: return launch_squeeze_f<4>(x, y, planes, h, w, f, rows, tiles, np, mode, grid, lds, s);
    default: return launch_squeeze_f<0>(x, y, planes, h, w, f, rows, tiles, np, mode, grid, lds, s);
  }
}

}  // namespace fc

extern "C" int fc_squeeze(const float* x, float* y, int64_t planes, int32_t h, int32_t w, int32_t factor, int32_t mode,
                          void* stream) {
  if (planes < 0 || h <= 0 || w <= 0 || factor < 2 || (mode != 0 && mode != 1)) return hipErrorInvalidValue;
  if (h % factor != 0 || w % factor != 0) return hipErrorInvalidValue;
  if (planes == 0) return hipSuccess;
  if (!x || !y || x == y) return hipErrorInvalidValue;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int ho = h / factor;
  const int row_floats = factor * w;  // floats of one output row's worth of the plane side
  if (row_floats <= 4 * fc::kSqueezeTileFloats) {
    int rows = fc::kSqueezeTileFloats / row_floats;
    if (rows < 1) rows = 1;
    int np = 1;
    if (rows >= ho) {  // whole planes fit: a block takes np consecutive planes
      rows = ho;
      np = (int)(fc::kSqueezeTileFloats / ((int64_t)h * w));
      if (np < 1) np = 1;
      if (np > planes) np = (int)planes;
    }
    const int tiles = (ho + rows - 1) / rows;
    const int64_t grid = (planes + np - 1) / np * tiles;
    if (grid > 0x7fffffffLL) return hipErrorInvalidConfiguration;
    const size_t lds = sizeof(float) * (size_t)np * rows * row_floats;
    return fc::launch_squeeze(x, y, planes, h, w, factor, rows, tiles, np, mode, grid, lds, s);
  } else {
    const int64_t total = planes * (int64_t)h * w;
    int64_t grid = (total + fc::kImageThreads - 1) / fc::kImageThreads;
    if (grid > 256 * 32) grid = 256 * 32;
    if (mode == 0)
      hipLaunchKernelGGL(fc::squeeze_direct_kernel<0>, dim3((unsigned)grid), dim3(fc::kImageThreads), 0, s, x, y,
                         total, h, w, factor);
    else
      hipLaunchKernelGGL(fc::squeeze_direct_kernel<1>, dim3((unsigned)grid), dim3(fc::kImageThreads), 0, s, x, y,
                         total, h, w, factor);
  }
  return hipGetLastError();
}

extern "C" int fc_conv1x1(const float* x, const float* weight, const float* pre, const float* post, float* y,
                          int64_t batch, int32_t c, int64_t hw, void* stream) {
  if (batch < 0 || c <= 0 || c > FC_CONV1X1_MAX_CHANNELS || hw <= 0) return hipErrorInvalidValue;
  if (batch == 0) return hipSuccess;
  if (!x || !weight || !y || x == y) return hipErrorInvalidValue;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (c <= 4) return fc::launch_conv1x1<4>(x, weight, pre, post, y, batch, c, hw, s);
  if (c <= 8) return fc::launch_conv1x1<8>(x, weight, pre, post, y, batch, c, hw, s);
  if (c <= 16) return fc::launch_conv1x1<16>(x, weight, pre, post, y, batch, c, hw, s);
  // as few groups of <= 32 rows as possible, each as narrow as the channel count allows (C = 48: two groups of 24, no
  // all-zero padding rows)
  const int groups = (c + 31) / 32;
  if ((c + groups - 1) / groups <= 24) return fc::launch_conv1x1<24>(x, weight, pre, post, y, batch, c, hw, s);
  return fc::launch_conv1x1<32>(x, weight, pre, post, y, batch, c, hw, s);
}
