// Density of a mixture-of-Gaussians MADE (flowcon/nn/nde/made.py:328-353) on the final layer's output, and its backward.
//
// Streaming kernels in the scheme of the per-sample-parameter bijectors (fc_tile.h): a workgroup owns a tile of S
// consecutive samples x dc dims whose parameter runs (3c floats per element, contiguous in HBM) and inputs are copied
// to LDS with coalesced 16-byte loads; one thread then evaluates one (sample, dim) element out of LDS -- no lane walks a
// strided 12c-byte run in global memory -- the per-element terms are summed per sample in dim order (deterministic), and
// the backward writes its gradients over the staged parameters and sends the tile back with coalesced stores.
// HBM sees 12c + 4 bytes in per element and 4 bytes out per row (backward: the same again out).
//
// d <= 256: a tile holds whole rows (S = 256 / d of them); wider rows take one sample per workgroup in chunks of 256 dims.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "fc_mog_op.h"
#include "../../include/flowcon_hip.h"

namespace fc {

constexpr int kMogBlock = 256;

struct MogArgs {
  const float* x;          // [n, d]
  const float* params;     // [n, d 3c]
  float* logp;             // [n]                   (forward)
  const float* grad_logp;  // [n]                   (backward)
  float* grad_x;           // [n, d]
  float* grad_params;      // [n, d 3c]
  int64_t n;
  int d, c, S, dc, accumulate;
  float eps;
};

__device__ __forceinline__ void mog_copy(float* __restrict__ dst, const float* __restrict__ src, int count) {
  const int tid = threadIdx.x;
  if (((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15u) == 0) {
    const int nvec = count >> 2;
    for (int i = tid; i < nvec; i += kMogBlock) reinterpret_cast<float4*>(dst)[i] = reinterpret_cast<const float4*>(src)[i];
    for (int i = (nvec << 2) + tid; i < count; i += kMogBlock) dst[i] = src[i];
  } else {
    for (int i = tid; i < count; i += kMogBlock) dst[i] = src[i];
  }
}

// LDS: [ params S dc 3c | x S dc | terms S dc ], every region a multiple of 4 floats
__host__ __device__ inline int mog_round4(int v) { return (v + 3) & ~3; }

template <bool kBackward>
__global__ __launch_bounds__(kMogBlock) void mog_kernel(MogArgs a) {
  extern __shared__ __attribute__((aligned(16))) float msm[];
  const int S = a.S, dc = a.dc, d = a.d, c = a.c, P = 3 * a.c;
  const int tid = threadIdx.x;
  const int64_t n0 = (int64_t)blockIdx.x * S;
  const int s_eff = (int)((a.n - n0) < (int64_t)S ? (a.n - n0) : (int64_t)S);
  float* ps = msm;
  float* xs = ps + mog_round4(S * dc * P);
  float* ls = xs + mog_round4(S * dc);
  float total = 0.f;                        // thread s < s_eff: the row sum of sample n0 + s
  // (a tile is contiguous in HBM: whole rows when dc == d, one sample's chunk otherwise)
  for (int j0 = 0; j0 < d; j0 += dc) {
    const int dcur = d - j0 < dc ? d - j0 : dc;
    const int elems = s_eff * dcur;
    const int64_t first = n0 * d + j0;
    mog_copy(ps, a.params + first * P, elems * P);
    mog_copy(xs, a.x + first, elems);
    __syncthreads();
    if (tid < elems) {
      float* p = ps + tid * P;
      const float xv = xs[tid];
      if constexpr (!kBackward) {
        ls[tid] = mog_log_density(p, c, a.eps, xv);
      } else {
        // responsibilities r_k = softmax(t)_k and mixture weights w_k = softmax(logit)_k, recomputed from the inputs:
        // dlogit_k = r_k - w_k, dmean_k = r_k z_k / std_k, dustd_k = r_k (z_k^2 - 1) / std_k * sigmoid(ustd_k),
        // dx = -sum_k r_k z_k / std_k, all times the row's grad_logp.  Pass 1 leaves z_k in the place of mean_k; pass 2
        // sums; pass 3 rebuilds std_k and t_k from ustd_k and z_k and overwrites the run with its gradient.
        const float ml = mog_max_logit(p, c);
        float mt = 0.f;
#pragma nounroll
        for (int k = 0; k < c; ++k) {
          float sd, z;
          mog_component(p, k, a.eps, xv, sd, z);
          const float t = (p[3 * k] - ml) - 0.5f * (kLog2Pi + 2.f * log_lean(sd) + z * z);
          p[3 * k + 1] = z;
          mt = k == 0 ? t : fmaxf(mt, t);
        }
        float sl = 0.f, st = 0.f;
#pragma nounroll
        for (int k = 0; k < c; ++k) {
          const float sd = softplus_lean(p[3 * k + 2], 1.f) + a.eps, z = p[3 * k + 1];
          sl += exp_lean(p[3 * k] - ml);
          st += exp_lean(((p[3 * k] - ml) - 0.5f * (kLog2Pi + 2.f * log_lean(sd) + z * z)) - mt);
        }
        const float g = a.grad_logp[n0 + tid / dcur];
        const float rsl = div_lean(1.f, sl), rst = div_lean(1.f, st);
        float gx = 0.f;
#pragma nounroll
        for (int k = 0; k < c; ++k) {
          const float u = p[3 * k + 2], z = p[3 * k + 1];
          const float sd = softplus_lean(u, 1.f) + a.eps, rstd = div_lean(1.f, sd);
          const float t = (p[3 * k] - ml) - 0.5f * (kLog2Pi + 2.f * log_lean(sd) + z * z);
          const float r = exp_lean(t - mt) * rst, w = exp_lean(p[3 * k] - ml) * rsl;
          const float dmean = r * z * rstd;
          const float dsd = r * (z * z - 1.f) * rstd;
          p[3 * k] = g * (r - w);
          p[3 * k + 1] = g * dmean;
          p[3 * k + 2] = g * (u > 20.f ? dsd : dsd * sigmoid_lean(u));      // F.softplus: identity beyond its threshold
          gx -= dmean;
        }
        xs[tid] = g * gx;
      }
    }
    __syncthreads();
    if constexpr (!kBackward) {
      if (S == 1) {
        // one sample per workgroup: wave sums, then the (at most four) partial sums in wave order
        float v = tid < elems ? ls[tid] : 0.f;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        __syncthreads();
        if ((tid & 63) == 0) ls[tid >> 6] = v;
        __syncthreads();
        if (tid == 0) total += (ls[0] + ls[1]) + (ls[2] + ls[3]);
      } else if (tid < s_eff) {
        const float* r = ls + tid * dcur;
        for (int j = 0; j < dcur; ++j) total += r[j];
      }
    } else {
      mog_copy(a.grad_params + first * P, ps, elems * P);
      mog_copy(a.grad_x + first, xs, elems);
    }
    __syncthreads();
  }
  if constexpr (!kBackward) {
    if (tid < s_eff) a.logp[n0 + tid] = a.accumulate ? a.logp[n0 + tid] + total : total;
  }
}

static hipError_t mog_launch(MogArgs a, bool backward, hipStream_t s) {
  if (a.n < 0 || a.d < 1 || a.c < 1 || a.c > kMogMaxComponents) return hipErrorInvalidValue;
  if (a.n == 0) return hipSuccess;
  if (!a.x || !a.params) return hipErrorInvalidValue;
  if (backward ? (!a.grad_logp || !a.grad_x || !a.grad_params) : !a.logp) return hipErrorInvalidValue;
  a.dc = a.d < kMogBlock ? a.d : kMogBlock;
  a.S = kMogBlock / a.dc;                                  // >= 1; 1 for every d > 128
  if ((int64_t)a.S > a.n) a.S = (int)a.n;
  const int64_t grid = (a.n + a.S - 1) / a.S;
  if (grid > 0x7fffffffLL) return hipErrorInvalidValue;
  // <= 256 elements x 48 floats + 2 x 256 floats: 51 KB, under the default dynamic LDS limit
  const size_t lds = sizeof(float) * (size_t)(mog_round4(a.S * a.dc * 3 * a.c) + 2 * mog_round4(a.S * a.dc) + 4);
  if (backward)
    hipLaunchKernelGGL((mog_kernel<true>), dim3((unsigned)grid), dim3(kMogBlock), lds, s, a);
  else
    hipLaunchKernelGGL((mog_kernel<false>), dim3((unsigned)grid), dim3(kMogBlock), lds, s, a);
  return hipGetLastError();
}

}  // namespace fc

extern "C" int fc_mog_log_prob(const float* x, const float* params, float* logp, int64_t n, int32_t d, int32_t c, float epsilon,
                               int32_t flags, void* stream) {
  fc::MogArgs a{x, params, logp, nullptr, nullptr, nullptr, n, d, c, 0, 0, (flags & FC_RQ_ACCUMULATE_LOGABSDET) ? 1 : 0, epsilon};
  return fc::mog_launch(a, false, static_cast<hipStream_t>(stream));
}

extern "C" int fc_mog_log_prob_backward(const float* grad_logp, const float* x, const float* params, float* grad_x,
                                        float* grad_params, int64_t n, int32_t d, int32_t c, float epsilon, void* stream) {
  fc::MogArgs a{x, params, nullptr, grad_logp, grad_x, grad_params, n, d, c, 0, 0, 0, epsilon};
  return fc::mog_launch(a, true, static_cast<hipStream_t>(stream));
}
