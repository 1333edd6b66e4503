// Backward of the row-per-wavefront bijectors with PER-SAMPLE parameters (a hyper-network's output): per-sample dense /
// LU matrices, per-sample Householder sequences, per-sample planar flow.  gfx950.  Forward kernels in fc_rowwave.hip, the
// batch-shared backward kernels in fc_rowwave_backward.hip.
//
// One wave owns one sample row (fc_row.h) and that sample's parameter block.  A per-sample parameter gradient belongs to
// one row only: it is written once, by the wave that owns the row -- no batch reduction, no atomics, no LDS, and two runs
// give the same bits.  Every global index stays inside the row's own block; matrix row indices past d are clamped to
// d - 1 (as load_rows does in the forward kernel) and their results discarded.
//
// Linear, M [d, d] raw per sample, sp = offdiag_scale, dg_j = softplus(M_jj) + eps:
//   mode 0  y = M x:      gx = M^T gy,  gM_ij = gy_i x_j                                    one pass over M
//   mode 1  y = M^T x:    gx = M gy,    gM_ij = x_i gy_j                                    one pass over M
//   mode 2  y = L U x,  L = sp tril(M, -1) + I,  U = sp triu(M, 1) + diag(dg),  lad = sum log dg:
//     t = U x,  g_t = L^T gy,  gx = U^T g_t
//     gM_ij = sp gy_i t_j (j < i),  sp g_t_i x_j (j > i),  (g_t_i x_i + gl / dg_i) sigmoid(M_ii) (j = i)
//     g_sp  = sum_{j<i} M_ij gy_i t_j + sum_{j>i} M_ij g_t_i x_j
//     pass A (rows ascending):  t_i by a row dot product (eight at a time, wave64_sum8), g_t += sp gy_i M_i,<i
//     pass B (rows descending): row i of gM, gx += sp g_t_i M_i,>i, the lane's share of g_sp
//   mode 3  x = U^-1 L^-1 y, lad = -sum log dg, from the saved OUTPUT x and the upstream gradient gx:
//     gy = L^-T U^-T gx as two column sweeps over coalesced rows of M: ascending, s_i = g_i / dg_i is final once the rows
//     before it are done, then g_j -= sp M_ij s_i (j > i); descending the same with L^T (unit diagonal), g_j -= sp M_ij r_i
//     (j < i).  No wave reduction.  The parameter gradients are mode 2's expressions at the input x with upstream -gy and
//     -gl (the implicit-function theorem on y = L U x), where g_t = L^T (-gy) = -s is already at hand: t = U x rides the
//     ascending sweep and row i of gM leaves in the descending one, as soon as r_i is final.
//   Modes 2 and 3 read M twice and write gM once.
//
// Householder (formulas: header of fc_rowwave_backward.hip): the walk back from the saved output with this row's q block;
// gq is stored per row and reflection, so neither the register chunking over reflections nor the re-walk is needed.
//
// Planar: planar_backward_row (fc_row.h), which planar_backward_kernel uses too, with this row's w, u_hat, b and u.w; gw, gu,
// gb stored per row.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "fc_math.h"
#include "fc_lane.h"
#include "fc_row.h"
#include "../../include/flowcon_hip.h"

namespace fc {

template <int E>
__global__ __launch_bounds__(256) void linear_ps_backward_kernel(const float* __restrict__ xs, const float* __restrict__ gs,
                                                                 const float* __restrict__ gl, const float* __restrict__ m,
                                                                 float* __restrict__ gin, float* __restrict__ gm,
                                                                 float* __restrict__ gsp, int64_t n, int d, int mode,
                                                                 float sp, float eps) {
  const int lane = threadIdx.x & 63;
  const int64_t stride = wave_unit_stride();
  for (int64_t row = wave_first_unit(); row < n; row += stride) {
    const float* mr = m + row * (int64_t)d * d;
    float* gr = gm + row * (int64_t)d * d;
    Row<E> x, g, out;
    load_row<E>(x, xs + row * d, d, lane);
    load_row<E>(g, gs + row * d, d, lane);
#pragma unroll
    for (int e = 0; e < E; ++e) out.v[e] = 0.f;
    float gspv = 0.f;
    // eight matrix rows per step, their loads issued together
    constexpr int kRows = 8;
    auto load_rows = [&](int i0, Row<E> (&mi)[kRows]) {
#pragma unroll
      for (int k = 0; k < kRows; ++k) load_row<E>(mi[k], mr + (int64_t)(i0 + k < d ? i0 + k : d - 1) * d, d, lane);
    };
    if (mode == 0) {          // gx_j = sum_i M_ij gy_i;  gM_i. = gy_i x
      for (int i0 = 0; i0 < d; i0 += kRows) {
        Row<E> mi[kRows];
        load_rows(i0, mi);
#pragma unroll
        for (int k = 0; k < kRows; ++k) {
          const int i = i0 + k;
          if (i >= d) continue;
          const float gi = bcast<E>(g, i);
          Row<E> o;
#pragma unroll
          for (int e = 0; e < E; ++e) {
            out.v[e] += mi[k].v[e] * gi;
            o.v[e] = gi * x.v[e];
          }
          store_row<E>(o, gr + (int64_t)i * d, d, lane);
        }
      }
    } else if (mode == 1) {   // gx_i = sum_j M_ij gy_j;  gM_i. = x_i gy
      for (int i0 = 0; i0 < d; i0 += kRows) {
        Row<E> mi[kRows];
        load_rows(i0, mi);
        float part[kRows], tot[kRows];
#pragma unroll
        for (int k = 0; k < kRows; ++k) {
          part[k] = 0.f;
#pragma unroll
          for (int e = 0; e < E; ++e) part[k] += mi[k].v[e] * g.v[e];
        }
        wave64_sum8(part, tot);
#pragma unroll
        for (int k = 0; k < kRows; ++k) {
          const int i = i0 + k;
          if (i >= d) continue;
          const float xi = bcast<E>(x, i);
          Row<E> o;
#pragma unroll
          for (int e = 0; e < E; ++e) {
            if (lane + 64 * e == i) out.v[e] = tot[k];
            o.v[e] = xi * g.v[e];
          }
          store_row<E>(o, gr + (int64_t)i * d, d, lane);
        }
      }
    } else {
      // lane j: dg_j, sigmoid(M_jj) and the log-determinant's share of gM_jj (one strided load per register)
      const float glu = gl ? (mode == 2 ? gl[row] : -gl[row]) : 0.f;
      Row<E> diag, sig, dterm, t, s;
#pragma unroll
      for (int e = 0; e < E; ++e) {
        const int j = lane + 64 * e;
        const float mjj = j < d ? mr[(int64_t)j * d + j] : 0.f;
        diag.v[e] = j < d ? softplus1(mjj) + eps : 1.f;
        sig.v[e] = j < d ? sigmoidf(mjj) : 0.f;
        dterm.v[e] = glu / diag.v[e];
        t.v[e] = 0.f;
      }
      s = g;      // mode 2: becomes g_t = L^T gy;  mode 3: becomes s = U^-T gx
      // ---- ascending pass: t = U x (both modes);  mode 2: g_t;  mode 3: the sweep with U^T
      for (int i0 = 0; i0 < d; i0 += kRows) {
        Row<E> mi[kRows];
        load_rows(i0, mi);
        float part[kRows], tot[kRows];
#pragma unroll
        for (int k = 0; k < kRows; ++k) {       // t_i = dg_i x_i + sp sum_{j>i} M_ij x_j
          const int i = i0 + k;
          part[k] = 0.f;
#pragma unroll
          for (int e = 0; e < E; ++e) {
            const int j = lane + 64 * e;
            part[k] += (j > i && j < d) ? sp * mi[k].v[e] * x.v[e] : (j == i ? diag.v[e] * x.v[e] : 0.f);
          }
        }
        wave64_sum8(part, tot);
#pragma unroll
        for (int k = 0; k < kRows; ++k) {
          const int i = i0 + k;
          if (i >= d) continue;
#pragma unroll
          for (int e = 0; e < E; ++e) if (lane + 64 * e == i) t.v[e] = tot[k];
          if (mode == 2) {
            const float gi = bcast<E>(g, i);
#pragma unroll
            for (int e = 0; e < E; ++e) if (lane + 64 * e < i) s.v[e] += sp * mi[k].v[e] * gi;
          } else {
#pragma unroll
            for (int e = 0; e < E; ++e) if (lane + 64 * e == i) s.v[e] = s.v[e] / diag.v[e];
            const float si = bcast<E>(s, i);      // final: every row before i has been taken off
#pragma unroll
            for (int e = 0; e < E; ++e) {
              const int j = lane + 64 * e;
              if (j > i && j < d) s.v[e] -= sp * mi[k].v[e] * si;
            }
          }
        }
      }
      // ---- descending pass: row i of gM, g_sp;  mode 2: gx = U^T g_t;  mode 3: the sweep with L^T
      if (mode == 2) {
#pragma unroll
        for (int e = 0; e < E; ++e) out.v[e] = diag.v[e] * s.v[e];
      } else {
        out = s;
      }
      for (int i0 = ((d - 1) / kRows) * kRows; i0 >= 0; i0 -= kRows) {
        Row<E> mi[kRows];
        load_rows(i0, mi);
#pragma unroll
        for (int k = kRows - 1; k >= 0; --k) {
          const int i = i0 + k;
          if (i >= d) continue;
          // upstream of the mode-2 expressions: (gy_i, g_t_i), in mode 3 (-r_i, -s_i) with r_i final here
          const float si = bcast<E>(s, i);
          const float up = mode == 2 ? bcast<E>(g, i) : -bcast<E>(out, i);
          const float gti = mode == 2 ? si : -si;
          Row<E> o;
#pragma unroll
          for (int e = 0; e < E; ++e) {
            const int j = lane + 64 * e;
            const float lo = up * t.v[e], hi = gti * x.v[e];
            o.v[e] = j < i ? sp * lo : (j > i ? sp * hi : (hi + dterm.v[e]) * sig.v[e]);
            gspv += j < i ? mi[k].v[e] * lo : ((j > i && j < d) ? mi[k].v[e] * hi : 0.f);
            if (mode == 2) {
              if (j > i && j < d) out.v[e] += sp * mi[k].v[e] * gti;
            } else {
              if (j < i) out.v[e] += sp * mi[k].v[e] * up;      // r_j -= sp M_ij r_i
            }
          }
          store_row<E>(o, gr + (int64_t)i * d, d, lane);
        }
      }
      gspv = wave_sum(gspv);
    }
    store_row<E>(out, gin + row * d, d, lane);
    if (gsp && lane == 0) gsp[row] = gspv;
  }
}

// The same four modes for matrices of <= 16 x 16 (the low-dimensional conditional flows): four samples per wave, one per
// 16-lane DPP row, as linear_per_sample_narrow_kernel.  Lane j of a row holds x_j, gy_j and column j of every matrix row
// in registers, so M is read from memory once in every mode; a dot product is four DPP rotations.
__global__ __launch_bounds__(256) void linear_ps_backward_narrow_kernel(const float* __restrict__ xs,
                                                                        const float* __restrict__ gs,
                                                                        const float* __restrict__ gl,
                                                                        const float* __restrict__ m, float* __restrict__ gin,
                                                                        float* __restrict__ gm, float* __restrict__ gsp,
                                                                        int64_t n, int d, int mode, float sp, float eps) {
  const int lane = threadIdx.x & 63, j = lane & 15, rowbase = lane & 48;
  const int64_t stride = wave_unit_stride() * 4;
  for (int64_t base = wave_first_unit() * 4; base < n; base += stride) {
    const int64_t row = base + (lane >> 4);
    const int64_t rr = row < n ? row : n - 1;
    const bool live = row < n && j < d;
    const float* mr = m + rr * (int64_t)d * d;
    float* gr = gm + rr * (int64_t)d * d;
    float mi[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) mi[i] = (i < d && j < d) ? mr[i * d + j] : 0.f;
    const float x = j < d ? xs[rr * d + j] : 0.f;
    const float g = j < d ? gs[rr * d + j] : 0.f;
    auto pick = [&](float v, int i) { return __shfl(v, rowbase | i, 64); };   // lane i of this sample's row
    float out = 0.f, gspv = 0.f;
    if (mode == 0) {
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const float gi = pick(g, i);
        out += mi[i] * gi;
        if (i < d && live) gr[i * d + j] = gi * x;
      }
    } else if (mode == 1) {
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const float sres = row16_allsum(mi[i] * g);
        if (j == i) out = sres;
        const float xi = pick(x, i);
        if (i < d && live) gr[i * d + j] = xi * g;
      }
    } else {
      const float glu = gl ? (mode == 2 ? gl[rr] : -gl[rr]) : 0.f;
      const float mjj = j < d ? mr[j * d + j] : 0.f;
      const float dg = j < d ? softplus1(mjj) + eps : 1.f;
      const float sig = j < d ? sigmoidf(mjj) : 0.f;
      const float dterm = glu / dg;
      float t = 0.f, s = g;
#pragma unroll
      for (int i = 0; i < 16; ++i) {       // t = U x
        const float part = row16_allsum(j > i ? sp * mi[i] * x : (j == i ? dg * x : 0.f));
        if (j == i) t = part;
      }
      if (mode == 2) {                     // g_t = L^T gy
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const float gi = pick(g, i);
          if (j < i) s += sp * mi[i] * gi;
        }
        out = dg * s;
      } else {                             // s = U^-T gx
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          if (j == i) s = s / dg;
          const float si = pick(s, i);
          if (j > i) s -= sp * mi[i] * si;
        }
        out = s;
      }
#pragma unroll
      for (int i = 15; i >= 0; --i) {
        const float si = pick(s, i);
        const float up = mode == 2 ? pick(g, i) : -pick(out, i);
        const float gti = mode == 2 ? si : -si;
        const float lo = up * t, hi = gti * x;
        if (i < d && live) gr[i * d + j] = j < i ? sp * lo : (j > i ? sp * hi : (hi + dterm) * sig);
        gspv += j < i ? mi[i] * lo : (j > i ? mi[i] * hi : 0.f);
        if (mode == 2) {
          if (j > i) out += sp * mi[i] * gti;
        } else {
          if (j < i) out += sp * mi[i] * up;
        }
      }
      gspv = row16_allsum(gspv);
    }
    if (live) gin[row * d + j] = out;
    if (gsp && row < n && j == 0) gsp[row] = gspv;
  }
}

template <int E>
__global__ __launch_bounds__(256) void householder_ps_backward_kernel(const float* __restrict__ y, const float* __restrict__ gy,
                                                                      const float* __restrict__ q, float* __restrict__ gx,
                                                                      float* __restrict__ gq, int64_t n, int d, int k_count,
                                                                      int reverse) {
  const int lane = threadIdx.x & 63;
  const int64_t stride = wave_unit_stride();
  for (int64_t row = wave_first_unit(); row < n; row += stride) {
    const float* qr = q + row * (int64_t)k_count * d;
    float* gqr = gq + row * (int64_t)k_count * d;
    Row<E> v, g;
    load_row<E>(v, y + row * d, d, lane);
    load_row<E>(g, gy + row * d, d, lane);
    // positions p0, p0 - 1, ... in application order (0 = first reflection applied), last first; eight q rows requested
    // together and their |q|^2 in one batched reduction
    constexpr int kB = 8;
    for (int p0 = k_count - 1; p0 >= 0; p0 -= kB) {
      Row<E> qv[kB];
      float part[kB], sq[kB];
#pragma unroll
      for (int b = 0; b < kB; ++b) {
        const int p = p0 - b >= 0 ? p0 - b : 0;
        load_row<E>(qv[b], qr + (int64_t)(reverse ? k_count - 1 - p : p) * d, d, lane);
        part[b] = 0.f;
#pragma unroll
        for (int e = 0; e < E; ++e) part[b] += qv[b].v[e] * qv[b].v[e];
      }
      wave64_sum8(part, sq);
#pragma unroll
      for (int b = 0; b < kB; ++b) {
        const int p = p0 - b;
        if (p < 0) continue;
        const float alpha = 2.f / sq[b];
        const float a_out = dot_rows<E>(v, qv[b]), c = dot_rows<E>(g, qv[b]);
        const float a = -a_out;      // y_prev = H v: y_prev.q = a_out - alpha a_out (q.q) = -a_out
        Row<E> o;
#pragma unroll
        for (int e = 0; e < E; ++e) {
          v.v[e] -= a_out * (alpha * qv[b].v[e]);        // v = y_prev
          o.v[e] = -alpha * (c * v.v[e] + a * g.v[e]) + (alpha * alpha) * (a * c) * qv[b].v[e];
          g.v[e] -= c * (alpha * qv[b].v[e]);            // gradient flowing to the previous reflection
        }
        store_row<E>(o, gqr + (int64_t)(reverse ? k_count - 1 - p : p) * d, d, lane);
      }
    }
    store_row<E>(g, gx + row * d, d, lane);
  }
}

template <int E>
__global__ __launch_bounds__(256) void planar_ps_backward_kernel(const float* __restrict__ x, const float* __restrict__ gy,
                                                                 const float* __restrict__ gl, const float* __restrict__ w,
                                                                 const float* __restrict__ u_hat, const float* __restrict__ b,
                                                                 float* __restrict__ gx, float* __restrict__ gw,
                                                                 float* __restrict__ gu, float* __restrict__ gb, int64_t n,
                                                                 int d) {
  const int lane = threadIdx.x & 63;
  const int64_t stride = wave_unit_stride();
  for (int64_t row = wave_first_unit(); row < n; row += stride) {
    Row<E> r, g, wv, uv, gwv, guv;
    load_row<E>(r, x + row * d, d, lane);
    load_row<E>(g, gy + row * d, d, lane);
    load_row<E>(wv, w + row * d, d, lane);
    load_row<E>(uv, u_hat + row * d, d, lane);
    const Row<E> gyv = g;
    const PlanarBackward k = planar_backward_row<E>(r, g, wv, uv, b[row], gl ? gl[row] : 0.f, dot_rows<E>(uv, wv));
#pragma unroll
    for (int e = 0; e < E; ++e) {
      gwv.v[e] = k.gw(r.v[e], uv.v[e]);
      guv.v[e] = k.gu(gyv.v[e], wv.v[e]);
    }
    store_row<E>(g, gx + row * d, d, lane);
    store_row<E>(gwv, gw + row * d, d, lane);
    store_row<E>(guv, gu + row * d, d, lane);
    if (lane == 0) gb[row] = k.g_a;
  }
}

}  // namespace fc

extern "C" int fc_linear_per_sample_backward(const float* x_or_out, const float* grad_out, const float* grad_logabsdet,
                                             const float* m, float* grad_in, float* grad_m, float* grad_sp_rows, int64_t n,
                                             int32_t d, int32_t mode, float offdiag_scale, float eps, void* stream) {
  if (n < 0 || d <= 0 || d > fc::kMaxRowFeatures || mode < 0 || mode > 3) return hipErrorInvalidValue;
  if (n == 0) return hipSuccess;
  if (!x_or_out || !grad_out || !m || !grad_in || !grad_m) return hipErrorInvalidValue;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (d <= 16) {
    hipLaunchKernelGGL(fc::linear_ps_backward_narrow_kernel, dim3(fc::row_grid((n + 3) / 4, fc::kStreamGridCap)), dim3(256), 0,
                       s, x_or_out, grad_out, grad_logabsdet, m, grad_in, grad_m, grad_sp_rows, n, d, mode, offdiag_scale, eps);
    return hipGetLastError();
  }
  FC_ROW_DISPATCH(d, hipLaunchKernelGGL(fc::linear_ps_backward_kernel<E>, dim3(fc::row_grid(n, fc::kStreamGridCap)), dim3(256),
                                        0, s, x_or_out, grad_out, grad_logabsdet, m, grad_in, grad_m, grad_sp_rows, n, d, mode,
                                        offdiag_scale, eps));
  return hipGetLastError();
}

extern "C" int fc_householder_backward_per_sample(const float* y, const float* grad_y, const float* q, float* grad_x,
                                                  float* grad_q, int64_t n, int32_t d, int32_t num_transforms,
                                                  int32_t reverse, void* stream) {
  if (n < 0 || d <= 0 || d > fc::kMaxRowFeatures || num_transforms < 0) return hipErrorInvalidValue;
  if (n == 0) return hipSuccess;
  if (!y || !grad_y || !grad_x || (num_transforms > 0 && (!q || !grad_q))) return hipErrorInvalidValue;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (num_transforms == 0) return hipMemcpyAsync(grad_x, grad_y, sizeof(float) * n * d, hipMemcpyDeviceToDevice, s);
  FC_ROW_DISPATCH(d, hipLaunchKernelGGL(fc::householder_ps_backward_kernel<E>, dim3(fc::row_grid(n, fc::kStreamGridCap)),
                                        dim3(256), 0, s, y, grad_y, q, grad_x, grad_q, n, d, num_transforms, reverse));
  return hipGetLastError();
}

extern "C" int fc_planar_backward_per_sample(const float* x, const float* grad_y, const float* grad_logabsdet,
                                             const float* w, const float* u_hat, const float* b, float* grad_x,
                                             float* grad_w, float* grad_u_hat, float* grad_b, int64_t n, int32_t d,
                                             void* stream) {
  if (n < 0 || d <= 0 || d > fc::kMaxRowFeatures) return hipErrorInvalidValue;
  if (n == 0) return hipSuccess;
  if (!x || !grad_y || !w || !u_hat || !b || !grad_x || !grad_w || !grad_u_hat || !grad_b) return hipErrorInvalidValue;
  hipStream_t s = static_cast<hipStream_t>(stream);
  FC_ROW_DISPATCH(d, hipLaunchKernelGGL(fc::planar_ps_backward_kernel<E>, dim3(fc::row_grid(n, fc::kStreamGridCap)), dim3(256),
                                        0, s, x, grad_y, grad_logabsdet, w, u_hat, b, grad_x, grad_w, grad_u_hat, grad_b, n,
                                        d));
  return hipGetLastError();
}
