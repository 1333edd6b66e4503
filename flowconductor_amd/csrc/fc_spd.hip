// Layers of flows on symmetric positive definite matrices (reference flowcon/transforms/matrix/ and
// FillTriangular, permutations.py:67-113).
//
//   fc_tril_pack        [B, d] <-> [B, m, m] lower-triangle fill / gather (np.tril_indices order), bit-exact
//   fc_matrix_diag      diagonal extract / copy with a new diagonal (torch.diagonal, diagonal_scatter), bit-exact
//   fc_cholesky_outer   Y = 0.5 (L L^T + (L L^T)^T), logabsdet = m log 2 + sum_i (m - i) log L_ii (cholesky.py:18-25)
//   fc_cholesky_outer_backward   grad_L = (G + G^T) L + diag((m - i) gl / L_ii), over the full m x m input
//   fc_cholesky         L = chol(A + eps I), logabsdet = -(m log 2 + sum_i (m - i) log L_ii) (cholesky.py:27-35)
//
// Matrix kernels: one lane owns row i (or column i) of a matrix padded to P = 8/16/32/64/128, kept in registers with
// compile-time indices.  P <= 64: one wave per block holding 64/P matrices; P = 128: a two-wave block.  The matrices
// are staged through an LDS tile (row stride P + 1: a lane reading its own row is conflict-free, a row read by the
// whole group is a broadcast) with coalesced global loads.  The padding is the identity for the factorisation
// (chol(diag(A, I)) = diag(chol(A), I) exactly) and zero for the products.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/flowcon_hip.h"
#include "fc_device.h"

namespace fc {

template <int P>
struct SpdShape {
  static constexpr int G = P >= 64 ? 1 : 64 / P;  // matrices per block
  static constexpr int T = P >= 64 ? P : 64;      // threads per block
  static constexpr int S = P + 1;                 // LDS row stride
  static constexpr int TILE = G * P * S;          // floats of the matrix tile
  static constexpr size_t lds_bytes() { return sizeof(float) * ((size_t)TILE + G + G * P); }
};

// Coalesced load of `nmat` consecutive m x m matrices into the tile; the rest of the tile is zero.
template <int P>
__device__ inline void load_tile(float* tile, const float* __restrict__ src, int nmat, int m) {
  using C = SpdShape<P>;
  const int mm = m * m;
  if (m != P || nmat != C::G) {
    for (int e = threadIdx.x; e < C::TILE; e += C::T) tile[e] = 0.f;
    __syncthreads();
  }
  const int count = nmat * mm;
  for (int e = threadIdx.x; e < count; e += C::T) {
    const int g = e / mm;
    const int rem = e - g * mm;
    const int i = rem / m;
    tile[g * P * C::S + i * C::S + (rem - i * m)] = src[e];
  }
  __syncthreads();
}

// Coalesced store of the tile's m x m matrices.
template <int P>
__device__ inline void store_tile(const float* tile, float* __restrict__ dst, int nmat, int m) {
  using C = SpdShape<P>;
  const int mm = m * m;
  const int count = nmat * mm;
  for (int e = threadIdx.x; e < count; e += C::T) {
    const int g = e / mm;
    const int rem = e - g * mm;
    const int i = rem / m;
    dst[e] = tile[g * P * C::S + i * C::S + (rem - i * m)];
  }
}

// sum_i (m - i) log d_i in index order, then m log 2 in front (the reference's float32 ops: powers * log(diag),
// .sum(-1), + N * log(2.)).  `terms` holds the group's P per-row terms.
__device__ inline float lad_sum(const float* terms, int m, float mlog2) {
  float s = 0.f;
  for (int i = 0; i < m; ++i) s += terms[i];
  return mlog2 + s;
}

template <int P>
__global__ __launch_bounds__(SpdShape<P>::T) void cholesky_outer_kernel(
    const float* __restrict__ L, float* __restrict__ Y, float* __restrict__ lad, uint32_t* __restrict__ err,
    int64_t batch, int m, float mlog2, int checkargs) {
  using C = SpdShape<P>;
  extern __shared__ float smem[];
  float* tile = smem;
  const int g = threadIdx.x / P, r = threadIdx.x % P;
  const int64_t b0 = (int64_t)blockIdx.x * C::G;
  const int nmat = (int)((batch - b0) < C::G ? (batch - b0) : C::G);
  const int64_t mm = (int64_t)m * m;
  load_tile<P>(tile, L + b0 * mm, nmat, m);

  const bool live = g < nmat && r < m;
  const float* gt = tile + g * P * C::S;
  float a[P];
  float dg = 1.f;
#pragma unroll
  for (int k = 0; k < P; ++k) {
    a[k] = gt[r * C::S + k];  // zero outside the matrix
    if (k == r) dg = a[k];
  }
  uint32_t bits = 0;
  if (checkargs && live) {
#pragma unroll
    for (int k = 0; k < P; ++k)
      if (k > r && k < m && !(a[k] == 0.f)) bits |= FC_ERR_NOT_LOWER_TRIANGULAR;
    if (!(dg > 0.f)) bits |= FC_ERR_DIAGONAL_NONPOSITIVE;
  }
  if (bits) atomicOr(err, bits);

  // lane r computes column r of Y: Y[j][r] = sum_k L[j][k] L[r][k] (the same fmaf sequence as Y[r][j]: exactly
  // symmetric, so 0.5 (P + P^T) = P) and stores it coalesced.
  if (g < nmat) {
    float* yg = Y + (b0 + g) * mm;
    for (int j = 0; j < m; ++j) {
      const float* row = gt + j * C::S;
      float acc = 0.f;
#pragma unroll
      for (int k = 0; k < P; ++k) acc = fmaf(row[k], a[k], acc);
      if (r < m) yg[j * m + r] = acc;
    }
  }
  if (lad) {
    float* terms = smem + C::TILE + g * P;
    terms[r] = live ? (float)(m - r) * logf(dg) : 0.f;
    __syncthreads();
    if (r == 0 && g < nmat) lad[b0 + g] = lad_sum(terms, m, mlog2);
  }
}

template <int P>
__global__ __launch_bounds__(SpdShape<P>::T) void cholesky_outer_backward_kernel(
    const float* __restrict__ L, const float* __restrict__ G_, const float* __restrict__ glad,
    float* __restrict__ gL, int64_t batch, int m) {
  using C = SpdShape<P>;
  extern __shared__ float smem[];
  float* tile = smem;
  const int g = threadIdx.x / P, r = threadIdx.x % P;
  const int64_t b0 = (int64_t)blockIdx.x * C::G;
  const int nmat = (int)((batch - b0) < C::G ? (batch - b0) : C::G);
  const int64_t mm = (int64_t)m * m;
  load_tile<P>(tile, L + b0 * mm, nmat, m);
  const float* gt = tile + g * P * C::S;
  // lane r keeps column r of L
  float c[P];
  float lrr = 1.f;
#pragma unroll
  for (int k = 0; k < P; ++k) {
    c[k] = gt[k * C::S + r];
    if (k == r) lrr = c[k];
  }
  float diag_term = 0.f;
  if (glad && g < nmat && r < m) diag_term = (glad[b0 + g] * (float)(m - r)) / lrr;
  __syncthreads();
  if (G_) load_tile<P>(tile, G_ + b0 * mm, nmat, m);
  if (g >= nmat) return;
  float* out = gL + (b0 + g) * mm;
  // grad_L[j][r] = sum_k (G[j][k] + G[k][j]) L[k][r]: both G reads are uniform over the group (broadcasts)
  for (int j = 0; j < m; ++j) {
    float acc = 0.f;
    if (G_) {
#pragma unroll
      for (int k = 0; k < P; ++k) acc = fmaf(gt[j * C::S + k] + gt[k * C::S + j], c[k], acc);
    }
    if (j == r) acc += diag_term;
    if (r < m) out[j * m + r] = acc;
  }
}

template <int P>
__global__ __launch_bounds__(SpdShape<P>::T) void cholesky_kernel(
    const float* __restrict__ A, float* __restrict__ Lout, float* __restrict__ lad, uint32_t* __restrict__ err,
    int64_t batch, int m, float eps, float mlog2, int checkargs) {
  using C = SpdShape<P>;
  extern __shared__ float smem[];
  float* tile = smem;
  const int g = threadIdx.x / P, r = threadIdx.x % P;
  const int64_t b0 = (int64_t)blockIdx.x * C::G;
  const int nmat = (int)((batch - b0) < C::G ? (batch - b0) : C::G);
  const int64_t mm = (int64_t)m * m;
  load_tile<P>(tile, A + b0 * mm, nmat, m);

  const bool live = g < nmat && r < m;
  float* gt = tile + g * P * C::S;
  uint32_t bits = 0;
  if (checkargs && live) {
    // inputs_jitter == inputs_jitter.mT: the jitter adds the same value to both sides (NaN compares unequal)
    for (int k = 0; k < m; ++k)
      if (!(gt[r * C::S + k] == gt[k * C::S + r])) bits |= FC_ERR_NOT_SYMMETRIC;
  }
  float a[P];
#pragma unroll
  for (int k = 0; k < P; ++k) {
    const float v = gt[r * C::S + k];
    a[k] = (k == r) ? (live ? v + eps : 1.f) : (live ? v : 0.f);
  }
  const uint32_t pivot_bit = checkargs ? FC_ERR_NOT_POSITIVE_DEFINITE : FC_ERR_CHOLESKY_FAILED;
  float* pivot = smem + C::TILE + g;
  float dg = 1.f;
  // column by column (left-looking Crout): step j forms L[r][j] = (A[r][j] - sum_{k<j} L[r][k] L[j][k]) / L[j][j]
  // from row j of L, which the tile holds by then (each lane overwrites its tile row with its L entries as they are
  // finished).  The padded pivots are exactly 1.
#pragma unroll
  for (int j = 0; j < P; ++j) {
    const float* lj = gt + j * C::S;
    float dot = 0.f;
#pragma unroll
    for (int k = 0; k < j; ++k) dot = fmaf(a[k], lj[k], dot);
    const float v = a[j] - dot;
    if (r == j) *pivot = v;
    __syncthreads();
    const float piv = *pivot;
    if (!(piv > 0.f)) bits |= pivot_bit;
    const float d = sqrtf(piv);
    const float inv = 1.f / d;  // one division per column, the scaling of LAPACK's potf2
    const float l = r > j ? v * inv : (r == j ? d : 0.f);
    if (r == j) dg = d;
    a[j] = l;
    gt[r * C::S + j] = l;
    __syncthreads();
  }
  if (live && bits) atomicOr(err, bits);
  // the tile now holds L (exact zeros above the diagonal)
  float* terms = smem + C::TILE + C::G + g * P;
  terms[r] = live ? (float)(m - r) * logf(dg) : 0.f;
  __syncthreads();
  if (lad && r == 0 && g < nmat) lad[b0 + g] = -lad_sum(terms, m, mlog2);
  store_tile<P>(tile, Lout + b0 * mm, nmat, m);
}

// ---- element layout kernels ---------------------------------------------------------------------------------------

template <typename I>
__global__ __launch_bounds__(256) void tril_pack_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                        I batch, int m, int mode) {
  const I mm = (I)m * m;
  const I d = (I)m * (m + 1) / 2;
  const I total = batch * mm;
  const I stride = (I)gridDim.x * blockDim.x;
  for (I e = (I)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += stride) {
    const I b = e / mm;
    const int rem = (int)(e - b * mm);
    const int i = rem / m, j = rem - i * m;
    const I t = b * d + (I)(i * (i + 1) / 2 + j);
    if (mode == 0) {
      y[e] = j <= i ? x[t] : 0.f;
    } else if (j <= i) {
      y[t] = x[e];
    }
  }
}

template <typename I>
__global__ __launch_bounds__(256) void matrix_diag_kernel(const float* __restrict__ x, float* __restrict__ diag,
                                                          float* __restrict__ y, I batch, int m, int mode) {
  const I mm = (I)m * m;
  const I stride = (I)gridDim.x * blockDim.x;
  if (mode == 0) {
    const I total = batch * m;
    for (I e = (I)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += stride) {
      const I b = e / m;
      const int i = (int)(e - b * m);
      diag[e] = x[b * mm + (I)i * (m + 1)];
    }
  } else {
    const I total = batch * mm;
    for (I e = (I)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += stride) {
      const I b = e / mm;
      const int rem = (int)(e - b * mm);
      const int i = rem / m, j = rem - i * m;
      y[e] = i == j ? diag[b * m + i] : (x ? x[e] : 0.f);
    }
  }
}

inline unsigned elementwise_grid(int64_t total) {
  int64_t grid = (total + 255) / 256;
  const int64_t cap = (int64_t)device_cu_count() * 32;
  return (unsigned)(grid < cap ? grid : cap);
}

template <int P, typename K, typename... Args>
hipError_t launch_matrix(K kernel, int64_t batch, hipStream_t s, Args... args) {
  using C = SpdShape<P>;
  const int64_t grid = (batch + C::G - 1) / C::G;
  if (grid > 0x7fffffffLL) return hipErrorInvalidConfiguration;
  const size_t bytes = C::lds_bytes();
  if (bytes > 65536) {
    static PerDeviceOnce once;
    const hipError_t e = ensure_max_dynamic_lds(once, reinterpret_cast<const void*>(kernel), (int)bytes);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(C::T), bytes, s, args...);
  return hipGetLastError();
}

inline int padded_size(int m) { return m <= 8 ? 8 : m <= 16 ? 16 : m <= 32 ? 32 : m <= 64 ? 64 : 128; }

}  // namespace fc

#define FC_SPD_DISPATCH(P_, KERNEL, ...)                                              \
  switch (P_) {                                                                       \
    case 8: return fc::launch_matrix<8>(KERNEL<8>, __VA_ARGS__);                      \
    case 16: return fc::launch_matrix<16>(KERNEL<16>, __VA_ARGS__);                   \
    case 32: return fc::launch_matrix<32>(KERNEL<32>, __VA_ARGS__);                   \
    case 64: return fc::launch_matrix<64>(KERNEL<64>, __VA_ARGS__);                   \
    default: return fc::launch_matrix<128>(KERNEL<128>, __VA_ARGS__);                 \
  }

extern "C" int fc_tril_pack(const float* x, float* y, int64_t batch, int32_t m, int32_t mode, void* stream) {
  if (batch < 0 || m <= 0 || (mode != 0 && mode != 1)) return hipErrorInvalidValue;
  if (batch == 0) return hipSuccess;
  if (!x || !y || x == y) return hipErrorInvalidValue;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int64_t total = batch * m * m;
  const unsigned grid = fc::elementwise_grid(total);
  if (total < (1ll << 31))
    hipLaunchKernelGGL(fc::tril_pack_kernel<int32_t>, dim3(grid), dim3(256), 0, s, x, y, (int32_t)batch, m, mode);
  else
    hipLaunchKernelGGL(fc::tril_pack_kernel<int64_t>, dim3(grid), dim3(256), 0, s, x, y, batch, m, mode);
  return hipGetLastError();
}

extern "C" int fc_matrix_diag(const float* x, float* diag, float* y, int64_t batch, int32_t m, int32_t mode,
                              void* stream) {
  if (batch < 0 || m <= 0 || (mode != 0 && mode != 1)) return hipErrorInvalidValue;
  if (batch == 0) return hipSuccess;
  if (!diag || (mode == 0 && !x) || (mode == 1 && (!y || x == y))) return hipErrorInvalidValue;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int64_t total = batch * m * (mode == 0 ? 1 : m);
  const unsigned grid = fc::elementwise_grid(total);
  if (batch * m * m < (1ll << 31))
    hipLaunchKernelGGL(fc::matrix_diag_kernel<int32_t>, dim3(grid), dim3(256), 0, s, x, diag, y, (int32_t)batch, m,
                       mode);
  else
    hipLaunchKernelGGL(fc::matrix_diag_kernel<int64_t>, dim3(grid), dim3(256), 0, s, x, diag, y, batch, m, mode);
  return hipGetLastError();
}

extern "C" int fc_cholesky_outer(const float* L, float* Y, float* logabsdet, uint32_t* err_flag, int64_t batch,
                                 int32_t m, int32_t checkargs, void* stream) {
  if (batch < 0 || m <= 0 || m > FC_SPD_MAX_DIM) return hipErrorInvalidValue;
  if (batch == 0) return hipSuccess;
  if (!L || !Y || L == Y || (checkargs && !err_flag)) return hipErrorInvalidValue;
  const float mlog2 = (float)(m * 0.69314718055994530942);
  FC_SPD_DISPATCH(fc::padded_size(m), fc::cholesky_outer_kernel, batch, static_cast<hipStream_t>(stream), L, Y,
                  logabsdet, err_flag, batch, (int)m, mlog2, (int)checkargs)
}

extern "C" int fc_cholesky_outer_backward(const float* L, const float* grad_outputs, const float* grad_logabsdet,
                                          float* grad_inputs, int64_t batch, int32_t m, void* stream) {
  if (batch < 0 || m <= 0 || m > FC_SPD_MAX_DIM) return hipErrorInvalidValue;
  if (batch == 0) return hipSuccess;
  if (!L || !grad_inputs || grad_inputs == L || grad_inputs == grad_outputs) return hipErrorInvalidValue;
  FC_SPD_DISPATCH(fc::padded_size(m), fc::cholesky_outer_backward_kernel, batch, static_cast<hipStream_t>(stream), L,
                  grad_outputs, grad_logabsdet, grad_inputs, batch, (int)m)
}

extern "C" int fc_cholesky(const float* A, float* L, float* logabsdet, uint32_t* err_flag, int64_t batch, int32_t m,
                           float eps, int32_t checkargs, void* stream) {
  if (batch < 0 || m <= 0 || m > FC_SPD_MAX_DIM) return hipErrorInvalidValue;
  if (batch == 0) return hipSuccess;
  if (!A || !L || A == L || !err_flag) return hipErrorInvalidValue;
  const float mlog2 = (float)(m * 0.69314718055994530942);
  FC_SPD_DISPATCH(fc::padded_size(m), fc::cholesky_kernel, batch, static_cast<hipStream_t>(stream), A, L, logabsdet,
                  err_flag, batch, (int)m, eps, mlog2, (int)checkargs)
}
