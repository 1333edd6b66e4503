// Backward of the piecewise linear / quadratic / cubic spline bijectors (forward direction), gfx950.
//
// What torch.autograd yields for flowcon/transforms/splines/linear.py:38-105, quadratic.py:55-159 and cubic.py:63-267
// (+ their `unconstrained_*` wrappers): grad_x [N, D] (transformed columns; the caller adds the identity columns) and
// grad_params [N, d_t P] from grad_y [N, D] and grad_logabsdet [N].
//
// These splines renormalise their parameters several times (softmax, trapezoid area, boundary heights, monotone knot
// slopes), so instead of a hand-derived adjoint per spline the kernel differentiates the forward evaluation itself in
// FORWARD mode: one thread per (element, direction) runs the element's evaluation on dual numbers (value, tangent) with
// the tangent seeded on ONE of the element's P raw parameters or on x, and writes that one gradient entry
//     grad = grad_y dy/dtheta + grad_logabsdet dlad/dtheta.
// P + 1 evaluations per element instead of one, but every thread is independent (no atomics, no reductions) and the
// writes are coalesced.  Working set: P dual numbers per thread in LDS.
//
// The evaluation is not restated here: the kernel instantiates fc_spline_ops.h's `*_prepare`, `cubic_bin`, `*_spline_forward`
// and `quadratic_spline_eval` templates, the very source the forward kernel (fc_splines.hip) compiles with T = float, with T = Dual (fc_dual.h).
// The value part of every Dual operation is the float operation, knot sums included (double value, float tangent), so
// each thread picks the bin and takes the branches the forward kernel took for that element, and the tangent is the
// derivative of that arithmetic.  What stays in the kernel is what the forward's tile launcher does around an Op:
// the gate on [left, right], the normalisation of x (tangent seed 1 / span_in) and the span_out factor of the output.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "fc_device.h"
#include "fc_spline_ops.h"
#include "../../include/flowcon_hip.h"

namespace fc {

struct SplineBwdArgs {
  const float* x;        // [N, D]
  const float* params;   // [N, d_t P]
  const int32_t* cols;   // [d_t] or null
  const float* gy;       // [N, D]
  const float* gl;       // [N] or null
  float* gx;             // [N, D] (transformed columns written)
  float* gp;             // [N, d_t P]
  int64_t total;         // N d_t (P + 1)
  int D, d_t, P, kind;
  SplineParams q;        // (q.inverse = 0: the entry point refuses the inverse)
};

// (6 waves per SIMD: the 80 VGPRs the kernel had on float knot sums; left alone the double sums take it to 100 and 4 waves,
//  below the 5 that its LDS allows at P = 15.  The bound pins the register allocator: it costs 16 bytes of scratch today,
//  and after any edit to the templates of fc_spline_ops.h that figure has to be read again with tools/kernel_stats.py)
__global__ __launch_bounds__(256, 6) void splines_backward_kernel(SplineBwdArgs a) {
  extern __shared__ Dual dual_smem[];
  const SplineParams& q = a.q;
  const int P = a.P, dirs = P + 1;
  Dual* p = dual_smem + (size_t)threadIdx.x * P;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < a.total; t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t elem = t / dirs;
    const int dir = (int)(t - elem * dirs);              // < P: raw parameter `dir`;  == P: the input
    const int64_t n = elem / a.d_t;
    const int j = (int)(elem - n * a.d_t);
    const int col = a.cols ? a.cols[j] : j;
    const float x = a.x[n * a.D + col];
    const float gy = a.gy[n * a.D + col], gl = a.gl ? a.gl[n] : 0.f;
    const bool inside = (x >= q.left) && (x <= q.right);
    float g;
    if (!inside) {
      g = dir == P ? gy : 0.f;                            // identity outside the interval, no logabsdet
    } else {
      const float* raw = a.params + elem * P;
      for (int i = 0; i < P; ++i) p[i] = Dual{raw[i], i == dir ? 1.f : 0.f};
      const float span_in = q.right - q.left, span_out = q.top - q.bottom;
      const Dual xn = Dual{(x - q.left) / span_in, dir == P ? 1.f / span_in : 0.f};
      Dual out, lad;
      if (a.kind == FC_SPLINE_LINEAR) {
        linear_prepare(q, p);
        linear_spline_forward(q, p, xn, out, lad);
        out.d *= span_out;
      } else if (a.kind == FC_SPLINE_QUADRATIC) {
        // (the quadratic's element function gates, normalises and scales by itself: the same arithmetic on x)
        uint32_t err = 0;
        quadratic_prepare(q, p);
        quadratic_spline_eval(q, p, p + q.K, Dual{x, dir == P ? 1.f : 0.f}, out, lad, err);
      } else {
        cubic_prepare(q, p);
        cubic_spline_forward(cubic_bin(q, p, p + q.K, xn.v, false), xn, out, lad);
        out.d *= span_out;
      }
      g = gy * out.d + gl * lad.d;
    }
    if (dir == P) a.gx[n * a.D + col] = g;
    else a.gp[elem * P + dir] = g;
  }
}

}  // namespace fc

extern "C" int fc_piecewise_spline_backward(const float* x, const float* params, const int32_t* cols, const float* grad_y,
                                            const float* grad_logabsdet, float* grad_x, float* grad_params, int64_t n,
                                            int32_t d, int32_t d_t, const fc_spline_config* cfg, void* stream) {
  if (!cfg || n < 0 || d <= 0 || d_t <= 0 || d_t > d || cfg->num_bins <= 0 || cfg->inverse) return hipErrorInvalidValue;
  if (n == 0) return hipSuccess;
  if (!x || !params || !grad_y || !grad_x || !grad_params) return hipErrorInvalidValue;
  const int P = fc::spline_params_per_dim(cfg->kind, cfg->num_bins, cfg->tails);
  if (P < 0) return hipErrorInvalidValue;
  const size_t lds = (size_t)256 * P * sizeof(fc::Dual);
  if (lds > 64 * 1024) return hipErrorInvalidValue;      // P <= 32 parameters per element
  fc::SplineBwdArgs a{};
  a.x = x; a.params = params; a.cols = cols; a.gy = grad_y; a.gl = grad_logabsdet; a.gx = grad_x; a.gp = grad_params;
  a.total = n * (int64_t)d_t * (P + 1);
  a.D = d; a.d_t = d_t; a.P = P; a.kind = cfg->kind;
  a.q = fc::spline_params_from_config(*cfg);
  int64_t grid = (a.total + 255) / 256;
  const int64_t cap = (int64_t)fc::device_cu_count() * 8;
  if (grid > cap) grid = cap;
  hipLaunchKernelGGL(fc::splines_backward_kernel, dim3((unsigned)grid), dim3(256), lds, static_cast<hipStream_t>(stream), a);
  return hipGetLastError();
}
