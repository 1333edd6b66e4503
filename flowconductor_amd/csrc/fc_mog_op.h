// One element of a mixture-of-Gaussians MADE (flowcon/nn/nde/made.py:328-353): the c <= 16 components of one dim of one
// sample as the final layer emits them, interleaved (logit, mean, unconstrained std) x c.  Shared by the streaming density
// kernels (fc_mog.hip) and the column step of the one-kernel sampler (fc_made_inverse.h, FC_MADE_MOG).
//
// log p(x) = logsumexp_k( log_softmax(logit)_k - 0.5 (log 2 pi + 2 log std_k + ((x - mean_k) / std_k)^2) ),
// std_k = softplus(ustd_k) + epsilon.  Two passes: the maximum of the logits (log_softmax) and of the summed terms are
// taken first, so logits spread by +-30 and points 50 standard deviations out stay finite and keep their digits.
// The lean exp / log / softplus of fc_math.h (<= ~1 ulp each) serve: every argument is finite, exp only meets
// arguments <= 0, log only sums in [1, 16] and standard deviations >= epsilon.
#pragma once
#include <hip/hip_runtime.h>
#include "fc_math.h"

namespace fc {

constexpr int kMogMaxComponents = 16;
constexpr float kLog2Pi = 1.8378770664093453f;

// std_k and z_k = (x - mean_k) / std_k of component k
__device__ __forceinline__ void mog_component(const float* p, int k, float eps, float x, float& sd, float& z) {
  sd = softplus_lean(p[3 * k + 2], 1.f) + eps;
  z = div_lean(x - p[3 * k + 1], sd);
}

__device__ __forceinline__ float mog_max_logit(const float* p, int c) {
  float ml = p[0];
#pragma nounroll
  for (int k = 1; k < c; ++k) ml = fmaxf(ml, p[3 * k]);
  return ml;
}

// log mixture density of x under the element's components.  p is the element's run in LDS and is CLOBBERED: the term
// t_k = (logit_k - max logit) - 0.5 (log 2 pi + 2 log std_k + z_k^2) takes the place of ustd_k between the two passes
// (run-time loops on purpose: unrolled over 16 components the evaluation needs more registers than a wave has).
__device__ __forceinline__ float mog_log_density(float* p, int c, float eps, float x) {
  const float ml = mog_max_logit(p, c);
  float mt = 0.f;
#pragma nounroll
  for (int k = 0; k < c; ++k) {
    float sd, z;
    mog_component(p, k, eps, x, sd, z);
    const float t = (p[3 * k] - ml) - 0.5f * (kLog2Pi + 2.f * log_lean(sd) + z * z);
    p[3 * k + 2] = t;
    mt = k == 0 ? t : fmaxf(mt, t);
  }
  float sl = 0.f, st = 0.f;
#pragma nounroll
  for (int k = 0; k < c; ++k) {
    sl += exp_lean(p[3 * k] - ml);
    st += exp_lean(p[3 * k + 2] - mt);
  }
  return (mt + log_lean(st)) - log_lean(sl);
}

// Inverse-CDF choice of a component: k = min{k : u S < sum_{j <= k} e_j}, e_j = exp(logit_j - max logit), S = sum_j e_j
// (the running sum in component order); the last component when no partial sum exceeds u S.  Then the draw
// mean_k + std_k * normal.
__device__ __forceinline__ float mog_draw(const float* p, int c, float eps, float normal, float u) {
  const float ml = mog_max_logit(p, c);
  float total = 0.f;
#pragma nounroll
  for (int k = 0; k < c; ++k) total += exp_lean(p[3 * k] - ml);
  const float target = u * total;
  float partial = 0.f, mean = p[3 * (c - 1) + 1], ustd = p[3 * (c - 1) + 2];
  bool found = false;
#pragma nounroll
  for (int k = 0; k < c; ++k) {
    partial += exp_lean(p[3 * k] - ml);
    const bool take = !found && target < partial;
    mean = take ? p[3 * k + 1] : mean;
    ustd = take ? p[3 * k + 2] : ustd;
    found = found || take;
  }
  return mean + (softplus_lean(ustd, 1.f) + eps) * normal;
}

}  // namespace fc
