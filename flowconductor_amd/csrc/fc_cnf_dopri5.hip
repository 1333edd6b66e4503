// fc_cnf_dopri5: a whole adaptive solve of a continuous normalizing flow in one launch, every row with its own time,
// step size, accept / reject decisions and attempt count (CNF/odeint.py, _Dopri5.advance, with the batch-wide error
// norm replaced by the row's own).
//
// The net, the image, the row-group layout and the numerics are fc_cnf.hip's (fc_cnf.h: cnf_net / cnf_field_row).  Two
// things differ from the fixed-step kernel there:
//
// * The state and the seven stage slopes are spread over the group: lane i owns component i of (z_0 .. z_{d-1}, logp)
//   (G >= d + 1) and holds y_i, k1_i .. k7_i, the candidate y_new_i and its share of the error, all float64.  For an
//   evaluation every owner rounds its stage state to float32 once and the lanes gather xin[] from the owners with
//   shuffles; the value lane's slopes and -div go back to the owners the same way.  The error norm is a butterfly sum
//   over the group; lane 0's ratio is broadcast, so that every lane of a group takes the same decision and runs the
//   same trip count (the shuffles need the whole group).  Groups of one wave may run different trip counts; the
//   finished ones idle.
// * Every row has its own t, so there is no block-wide time table and no barrier after the image copy: CnfRowTime
//   computes the fma terms where they are used and the gates per layer into an LDS strip of the row's own.
//
// A row ends with NaN outputs, at once, when it has used up max_attempts before reaching t1, when its error ratio is
// not finite, or when its step no longer moves t: the attempt counter grows on every trip of the loop, so the loop is
// bounded by max_attempts <= FC_CNF_DOPRI5_MAX_ATTEMPTS.
#include "fc_cnf.h"

namespace fc {

// Dormand-Prince 5(4), as selects on the stage (a run-time index into a local array would put it in scratch memory).
// Stage `st` (1 .. 6) reads the slopes 1 .. st with the coefficients a(st, 1 .. st); stage 6 is the candidate itself
// (first same as last: its coefficients are the fifth-order weights).
__device__ __forceinline__ double dopri5_node(int st) {
  return st == 1 ? 1.0 / 5.0 : st == 2 ? 3.0 / 10.0 : st == 3 ? 4.0 / 5.0 : st == 4 ? 8.0 / 9.0 : 1.0;
}
__device__ __forceinline__ double dopri5_a1(int st) {
  return st == 1   ? 1.0 / 5.0
         : st == 2 ? 3.0 / 40.0
         : st == 3 ? 44.0 / 45.0
         : st == 4 ? 19372.0 / 6561.0
         : st == 5 ? 9017.0 / 3168.0
                   : 35.0 / 384.0;
}
__device__ __forceinline__ double dopri5_a2(int st) {
  return st == 2 ? 9.0 / 40.0 : st == 3 ? -56.0 / 15.0 : st == 4 ? -25360.0 / 2187.0 : st == 5 ? -355.0 / 33.0 : 0.0;
}
__device__ __forceinline__ double dopri5_a3(int st) {
  return st == 3 ? 32.0 / 9.0 : st == 4 ? 64448.0 / 6561.0 : st == 5 ? 46732.0 / 5247.0 : st == 6 ? 500.0 / 1113.0 : 0.0;
}
__device__ __forceinline__ double dopri5_a4(int st) {
  return st == 4 ? -212.0 / 729.0 : st == 5 ? 49.0 / 176.0 : st == 6 ? 125.0 / 192.0 : 0.0;
}
__device__ __forceinline__ double dopri5_a5(int st) {
  return st == 5 ? -5103.0 / 18656.0 : st == 6 ? -2187.0 / 6784.0 : 0.0;
}
__device__ __forceinline__ double dopri5_a6(int st) { return st == 6 ? 11.0 / 84.0 : 0.0; }

// sqrt(mean over the row's d + 1 entries of v^2); v is 0 in the lanes that own nothing.  The same in every lane.
template <int G>
__device__ __forceinline__ double dopri5_rms(double v, int d) {
  double sq = v * v;
#pragma unroll
  for (int off = G / 2; off > 0; off >>= 1) sq += __shfl_xor(sq, off, G);
  return sqrt(sq / (double)(d + 1));
}

// The slope of this lane's component at time t, where `ys` is this lane's component of the stage state (float64;
// rounded to float32 here, the one rounding of a stage).
template <int G, int DP>
__device__ __forceinline__ double dopri5_slope(const float* img, double* strip, float* mine, int T, int half,
                                               const CnfShape& sh, int s, double t, double ys) {
  const float mine32 = (float)ys;
  float xin[DP];
#pragma unroll
  for (int i = 0; i < DP; ++i) {
    const float v = __shfl(mine32, i & (G - 1), G);
    xin[i] = i < sh.d ? v : 0.f;
  }
  double k[DP], negdiv;
  cnf_field_row<G, DP>(img, CnfRowTime<G>{t, strip, s, sh.gated}, CnfExactDiv{}, mine, T, half, sh, s, xin, k, negdiv);
  double slope = s == sh.d ? negdiv : 0.0;
#pragma unroll
  for (int i = 0; i < DP; ++i) {
    const double v = __shfl(k[i], 0, G);  // the value lane's
    if (i == s && i < sh.d) slope = v;
  }
  return slope;
}

template <int G>
__global__ __launch_bounds__(256) void cnf_dopri5_kernel(const float* __restrict__ z, const float* __restrict__ logp,
                                                         const float* __restrict__ image, float* __restrict__ z_out,
                                                         float* __restrict__ logp_out, int32_t* __restrict__ attempts_out,
                                                         float* __restrict__ evals, int64_t n, CnfShape sh,
                                                         int image_floats, int strip_doubles, double t0, double t1,
                                                         double atol, double rtol, double first_step,
                                                         int max_attempts) {
  constexpr int DP = LaneGroup<G>::DP;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const CnfBlock b = cnf_block<G>(lds, image, image_floats, 0, strip_doubles, n, sh);
  __syncthreads();  // the only barrier (cnf_block has none): the tile loop below has none
  const float* img = b.img;
  double* strip = b.mid + (size_t)b.r * strip_doubles;  // this row's
  float* mine = b.mine;
  const int T = b.T, tid = b.tid, d = sh.d, s = b.s, half = b.half;
  const bool owner = s <= d;
  const double span = t1 - t0, aspan = fabs(span), direction = span > 0.0 ? 1.0 : -1.0;
  const double reach = 1e-12 * fmax(1.0, aspan);
  const bool probe = !(first_step > 0.0);
  int most = -1;  // the largest attempt count of this lane's live rows

  for (int64_t tile = blockIdx.x; tile < b.tiles; tile += gridDim.x) {
    bool live;
    const int64_t row = tile_row(b, tile, n, live);
    double y = 0.0;
    if (s < d) y = (double)z[row * d + s];
    if (s == d && logp) y = (double)logp[row];
    double t = t0, done = 0.0, hmag = first_step;
    int attempts = 0;
    bool failed = false;
    bool active = aspan > reach;
    double k1 = 0.0, k2 = 0.0, k3 = 0.0, k4 = 0.0, k5 = 0.0, k6 = 0.0, k7 = 0.0;

    if (active) {  // the same for every row of the launch
      k1 = dopri5_slope<G, DP>(img, strip, mine, T, half, sh, s, t0, y);
      if (probe) {  // Hairer, Norsett & Wanner II.4 in the row's own scaled norm
        const double scale = atol + rtol * fabs(y);
        const double d0 = dopri5_rms<G>(owner ? y / scale : 0.0, d);
        const double d1 = dopri5_rms<G>(owner ? k1 / scale : 0.0, d);
        const double h0 = (d0 < 1e-5 || d1 < 1e-5) ? 1e-6 : 0.01 * d0 / d1;
        const double dh = direction * h0;
        const double f1 = dopri5_slope<G, DP>(img, strip, mine, T, half, sh, s, t0 + dh, y + dh * k1);
        const double d2 = dopri5_rms<G>(owner ? (f1 - k1) / scale : 0.0, d) / h0;
        const double top = fmax(d1, d2);
        const double h1 = top <= 1e-15 ? fmax(1e-6, h0 * 1e-3) : pow(0.01 / top, 1.0 / 5.0);
        hmag = __shfl(fmin(100.0 * h0, h1), 0, G);
      }
    }

    while (active) {
      if (attempts >= max_attempts) {
        failed = true;
        break;
      }
      ++attempts;
      const bool last = hmag >= aspan - done;
      const double h = last ? t1 - t : direction * hmag;
      if (!last && t + h == t) {  // the step no longer moves t
        failed = true;
        break;
      }
      double ynew = y;
#pragma unroll 1
      for (int stage = 1; stage <= 6; ++stage) {
        double total = dopri5_a1(stage) * k1;
        total += dopri5_a2(stage) * k2;
        total += dopri5_a3(stage) * k3;
        total += dopri5_a4(stage) * k4;
        total += dopri5_a5(stage) * k5;
        total += dopri5_a6(stage) * k6;
        ynew = y + h * total;
        const double slope = dopri5_slope<G, DP>(img, strip, mine, T, half, sh, s, t + dopri5_node(stage) * h, ynew);
        if (stage == 1) k2 = slope;
        if (stage == 2) k3 = slope;
        if (stage == 3) k4 = slope;
        if (stage == 4) k5 = slope;
        if (stage == 5) k6 = slope;
        if (stage == 6) k7 = slope;
      }
      double err = (35.0 / 384.0 - 5179.0 / 57600.0) * k1;
      err += (500.0 / 1113.0 - 7571.0 / 16695.0) * k3;
      err += (125.0 / 192.0 - 393.0 / 640.0) * k4;
      err += (-2187.0 / 6784.0 + 92097.0 / 339200.0) * k5;
      err += (11.0 / 84.0 - 187.0 / 2100.0) * k6;
      err += (-1.0 / 40.0) * k7;
      err *= h;
      const double tol = atol + rtol * fmax(fabs(y), fabs(ynew));
      const double ratio = __shfl(dopri5_rms<G>(owner ? err / tol : 0.0, d), 0, G);  // lane 0 decides for the group
      if (!isfinite(ratio)) {
        failed = true;
        break;
      }
      const double factor = ratio == 0.0 ? 10.0 : fmin(10.0, fmax(0.2, 0.9 * pow(ratio, -1.0 / 5.0)));
      if (ratio <= 1.0) {
        done = last ? aspan : done + hmag;
        t = last ? t1 : t + h;
        y = ynew;
        k1 = k7;
        if (!last || factor < 1.0)
          hmag = hmag * factor;
        else  // a shortened last step says little about the next
          hmag = fmax(hmag, fabs(h) * factor);
      } else {
        hmag = fabs(h) * fmin(1.0, factor);
      }
      active = aspan - done > reach;
    }

    if (live) {
      const float result = failed ? __int_as_float(0x7fc00000) : (float)y;
      if (s < d) z_out[row * d + s] = result;
      if (s == d) logp_out[row] = result;
      if (s == 0) attempts_out[row] = attempts;
      most = attempts > most ? attempts : most;
    }
  }

  // max over rows of (2 + 6 attempts), or 1 + 6 attempts with first_step; non-negative floats order like their bits
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const int other = __shfl_xor(most, off, 64);
    most = other > most ? other : most;
  }
  if (evals && (tid & 63) == 0 && most >= 0) {
    const int count = aspan > reach ? (probe ? 2 : 1) + 6 * most : 0;  // an empty interval costs no evaluation
    atomicMax(reinterpret_cast<int*>(evals), __float_as_int((float)count));
  }
}

// a strip of the widest layer's gates per row in place of the block's time table, and the two ping-pong columns
static GroupLds cnf_dopri5_lds(const CnfShape& sh) { return {0, 2 * cnf_max_width(sh), pad4(cnf_max_width(sh)), 0}; }

}  // namespace fc

extern "C" int fc_cnf_dopri5(const float* z, const float* logp, const float* image, float* z_out, float* logp_out,
                             int32_t* attempts, float* evals, int64_t n, int32_t d, int32_t layers,
                             const int32_t* hidden, int32_t layer_kind, int32_t activation, int32_t residual,
                             float scale_output, float p0, int32_t image_floats, double t0, double t1, double atol,
                             double rtol, double first_step, int32_t max_attempts, void* stream) {
  fc::CnfShape sh;
  if (max_attempts < 1 || max_attempts > FC_CNF_DOPRI5_MAX_ATTEMPTS) return hipErrorInvalidValue;
  if (!(t0 - t0 == 0.0) || !(t1 - t1 == 0.0) || !(atol >= 0.0) || !(rtol >= 0.0) || !(atol + rtol > 0.0) ||
      !(first_step >= 0.0) || !(first_step - first_step == 0.0))
    return hipErrorInvalidValue;
  if (!fc::cnf_entry(n, d, layers, hidden, layer_kind, activation, residual, scale_output, p0, image_floats,
                     FC_CNF_MAX_HIDDEN_LAYERS + 1, &sh))
    return hipErrorInvalidValue;
  if (n == 0) return hipSuccess;
  if (!fc::cnf_operands(z, image, z_out, logp_out) || !attempts) return hipErrorInvalidValue;
  const fc::GroupLds need = fc::cnf_dopri5_lds(sh);
  const fc::GroupLaunch plan =
      fc::group_launch_plan(image_floats, fc::cnf_group(sh), need, fc::kPrefer64K, n, fc::kGroupMaxBlocks);
  return fc::with_constant<2, 4, 8, 16, 32>(fc::cnf_group(sh), [&](auto g) {
    return fc::group_launch<&fc::cnf_dopri5_kernel<decltype(g)::value>>(
        plan, static_cast<hipStream_t>(stream), z, logp, image, z_out, logp_out, attempts, evals, n, sh, image_floats,
        need.row_doubles, t0, t1, atol, rtol, first_step, max_attempts);
  });
}
