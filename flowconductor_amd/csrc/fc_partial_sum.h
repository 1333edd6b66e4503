// The second launch of the backward kernels whose blocks each write a partial of the parameter gradient: the partials
// added in block order, so that the result does not depend on which block ran when (no atomics).
#pragma once
#include <hip/hip_runtime.h>

namespace fc {

// out[i] = (float)(scale * sum_b partial[b * count + i]), b ascending, accumulated in the partials' type
template <class Acc>
__global__ __launch_bounds__(256) void partial_sum_kernel(const Acc* __restrict__ partial, float* __restrict__ out,
                                                          int blocks, int count, Acc scale) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  Acc sum = 0;
  for (int b = 0; b < blocks; ++b) sum += partial[(size_t)b * (size_t)count + i];
  out[i] = (float)(sum * scale);
}

// scale 1 is exact: a caller without a scale gets the plain sum, bit for bit
template <class Acc>
inline int launch_partial_sum(const Acc* partial, float* out, int blocks, int count, Acc scale, hipStream_t s) {
  hipLaunchKernelGGL(partial_sum_kernel<Acc>, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, s, partial, out,
                     blocks, count, scale);
  return hipGetLastError();
}

}  // namespace fc
