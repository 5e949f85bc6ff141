// Device kernels of the thick-restart Lanczos eigen-solver (recur.cpp, eigs_core): the in-place Ritz rotation
// of the basis and the block dots / block subtraction of its classical Gram-Schmidt (applied twice).  All three are single-pass
// HBM streams over columns of doubles (16-byte accesses where the leading dimension and the base addresses allow), capped grids
// with grid-stride loops, no atomics; reductions run in a fixed order (the same call gives the same bits).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "device_common.hpp"

namespace {

constexpr int BS = 256;
constexpr int EIGS_BLOCKS = SD_EIGS_MAX_BLOCKS;   // most blocks of a pass: the per-block partial lists are summed by ONE wave per output
constexpr int EIGS_B = SD_EIGS_BLOCK_COLS;        // columns of one Gram-Schmidt block

// ---- the Ritz rotation:  V[r, c] <- sum_{j < m} V[r, j] * Q[j, c]  for c < k, in place ----
// One owner thread per row (W = 1) or per pair of neighbouring rows (W = 2: 16-byte accesses; needs an even ld and a 16-byte
// aligned base).  The owner reads its rows of all m columns -- j outermost, KB accumulators per row in registers, each term one
// multiply then one add in ascending j from a zero accumulator -- and only then writes columns 0..k-1: every read of a row
// precedes every write of it, and no other thread touches the row.  Columns k..m-1 and the padding are never written.
// Q sits in LDS as [j][KB] (a wave reads one address at a time: a broadcast).
template <int KB, int W>
__global__ __launch_bounds__(BS) void k_basis_rotate(double *V, int64_t ld, int64_t n, int m, int k, const double *__restrict__ Qd) {
  extern __shared__ double q_lds[];                      // m * KB doubles
  for (int t = threadIdx.x; t < m * KB; t += BS) {
    const int j = t / KB, c = t - j * KB;
    q_lds[t] = c < k ? Qd[j + (size_t)m * c] : 0.0;
  }
  __syncthreads();
  const int64_t items = (n + W - 1) / W;
  const int64_t stride = (int64_t)gridDim.x * BS;
  for (int64_t i = (int64_t)blockIdx.x * BS + threadIdx.x; i < items; i += stride) {
    const int64_t r = i * W;
    const bool two = W == 2 && r + 1 < n;                // the odd tail row of the pair form is handled alone
    double a0[KB], a1[KB];
#pragma unroll
    for (int c = 0; c < KB; ++c) { a0[c] = 0.0; a1[c] = 0.0; }
    for (int j = 0; j < m; ++j) {
      const double *col = V + (int64_t)j * ld + r;
      double v0, v1 = 0.0;
      if (two) { const double2 v = *(const double2 *)col; v0 = v.x; v1 = v.y; }
      else v0 = *col;
      const double *q = q_lds + j * KB;
#pragma unroll
      for (int c = 0; c < KB; ++c)
        if (c < k) {
          const double qc = q[c];
          a0[c] = a0[c] + v0 * qc;
          if (W == 2) a1[c] = a1[c] + v1 * qc;
        }
    }
#pragma unroll
    for (int c = 0; c < KB; ++c)
      if (c < k) {
        double *col = V + (int64_t)c * ld + r;
        if (two) *(double2 *)col = make_double2(a0[c], a1[c]);
        else *col = a0[c];
      }
  }
}

// ---- block dots:  out[c] = <V[:, c] | w>  for c < nc <= EIGS_B in one pass over w ----
// NC = 1: real dots (imaginary slot 0); NC = 2: complex dots with the column conjugated.  Per-thread sums, the wave shuffle, the
// waves of a block in order -> partials[block][2 c + {0, 1}]; k_block_dots_reduce sums the blocks (one wave per output).
template <int NC>
__global__ __launch_bounds__(BS) void k_block_dots(const double *__restrict__ V, int64_t ld, int nc, const double *__restrict__ w,
                                                   int64_t N, double *__restrict__ partials) {
  __shared__ double red[BS / 64][2 * EIGS_B];
  double re[EIGS_B], im[EIGS_B];
#pragma unroll
  for (int c = 0; c < EIGS_B; ++c) { re[c] = 0.0; im[c] = 0.0; }
  const int64_t stride = (int64_t)gridDim.x * BS;
  const int64_t i0 = (int64_t)blockIdx.x * BS + threadIdx.x;
  if (NC == 2) {
    const double2 *w2 = (const double2 *)w;
    for (int64_t i = i0; i < N; i += stride) {
      const double2 x = w2[i];
#pragma unroll
      for (int c = 0; c < EIGS_B; ++c)
        if (c < nc) {
          const double2 v = ((const double2 *)(V + (int64_t)c * ld))[i];
          re[c] += v.x * x.x + v.y * x.y;                // conj(v) * x
          im[c] += v.x * x.y - v.y * x.x;
        }
    }
  } else {
    const bool vec = (ld % 2 == 0) && !(((uintptr_t)w | (uintptr_t)V) & 15);
    const int64_t n2 = vec ? N / 2 : 0;
    const double2 *w2 = (const double2 *)w;
    for (int64_t i = i0; i < n2; i += stride) {
      const double2 x = w2[i];
#pragma unroll
      for (int c = 0; c < EIGS_B; ++c)
        if (c < nc) { const double2 v = ((const double2 *)(V + (int64_t)c * ld))[i]; re[c] += v.x * x.x + v.y * x.y; }
    }
    for (int64_t i = 2 * n2 + i0; i < N; i += stride) {
      const double x = w[i];
#pragma unroll
      for (int c = 0; c < EIGS_B; ++c)
        if (c < nc) re[c] += V[(int64_t)c * ld + i] * x;
    }
  }
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int c = 0; c < EIGS_B; ++c) {
    double a = re[c], b = im[c];
    for (int off = 32; off > 0; off >>= 1) { a += __shfl_down(a, off, 64); b += __shfl_down(b, off, 64); }
    if (lane == 0) { red[wv][2 * c] = a; red[wv][2 * c + 1] = b; }
  }
  __syncthreads();
  if (threadIdx.x < 2 * EIGS_B) {
    double a = 0.0;
    for (int k = 0; k < BS / 64; ++k) a += red[k][threadIdx.x];
    partials[(size_t)blockIdx.x * 2 * EIGS_B + threadIdx.x] = a;
  }
}
// lists of nb entries with `width` values each -> dst[0 .. nout): one wave per value, lane-strided then shuffled (one fixed order)
__global__ __launch_bounds__(64 * 2 * EIGS_B) void k_eigs_reduce(const double *__restrict__ partials, int nb, int width, int nout,
                                                                 double *__restrict__ dst) {
  const int c = threadIdx.x >> 6, lane = threadIdx.x & 63;
  double a = 0.0;
  if (c < nout) for (int b = lane; b < nb; b += 64) a += partials[(size_t)b * width + c];
  for (int off = 32; off > 0; off >>= 1) a += __shfl_down(a, off, 64);
  if (lane == 0 && c < nout) dst[c] = a;
}

// ---- block subtraction:  w <- w - sum_{c < nc} coef[c] * V[:, c],  coef[c] = (coef_dev[2c], coef_dev[2c + 1]) on the device ----
// Ascending c, one multiply and one subtract (add) per real term:
//   real     x = x - cr * v
//   complex  x.re = (x.re - cr * v.re) + ci * v.im ;  x.im = (x.im - cr * v.im) - ci * v.re
// NORM: the partials of |w_new|^2 -> partials[2 block] (and 0 beside it), for sd_reduce-style summation by k_eigs_reduce.
template <int NC, bool NORM>
__global__ __launch_bounds__(BS) void k_block_axpy(double *__restrict__ w, const double *__restrict__ V, int64_t ld, int nc,
                                                   const double *__restrict__ coef_dev, int64_t N, double *__restrict__ partials) {
  __shared__ double red[32];
  double cr[EIGS_B], ci[EIGS_B];
#pragma unroll
  for (int c = 0; c < EIGS_B; ++c) { cr[c] = c < nc ? coef_dev[2 * c] : 0.0; ci[c] = (c < nc && NC == 2) ? coef_dev[2 * c + 1] : 0.0; }
  double s = 0.0, s1 = 0.0;
  const int64_t stride = (int64_t)gridDim.x * BS;
  const int64_t i0 = (int64_t)blockIdx.x * BS + threadIdx.x;
  if (NC == 2) {
    double2 *w2 = (double2 *)w;
    for (int64_t i = i0; i < N; i += stride) {
      double2 x = w2[i];
#pragma unroll
      for (int c = 0; c < EIGS_B; ++c)
        if (c < nc) {
          const double2 v = ((const double2 *)(V + (int64_t)c * ld))[i];
          x.x = (x.x - cr[c] * v.x) + ci[c] * v.y;
          x.y = (x.y - cr[c] * v.y) - ci[c] * v.x;
        }
      w2[i] = x;
      if (NORM) s += x.x * x.x + x.y * x.y;
    }
  } else {
    const bool vec = (ld % 2 == 0) && !(((uintptr_t)w | (uintptr_t)V) & 15);
    const int64_t n2 = vec ? N / 2 : 0;
    double2 *w2 = (double2 *)w;
    for (int64_t i = i0; i < n2; i += stride) {
      double2 x = w2[i];
#pragma unroll
      for (int c = 0; c < EIGS_B; ++c)
        if (c < nc) { const double2 v = ((const double2 *)(V + (int64_t)c * ld))[i]; x.x = x.x - cr[c] * v.x; x.y = x.y - cr[c] * v.y; }
      w2[i] = x;
      if (NORM) s += x.x * x.x + x.y * x.y;
    }
    for (int64_t i = 2 * n2 + i0; i < N; i += stride) {
      double x = w[i];
#pragma unroll
      for (int c = 0; c < EIGS_B; ++c)
        if (c < nc) x = x - cr[c] * V[(int64_t)c * ld + i];
      w[i] = x;
      if (NORM) s += x * x;
    }
  }
  if (NORM) {
    sd_dev::block_reduce2(s, s1, red);
    if (threadIdx.x == 0) { partials[2 * blockIdx.x] = s; partials[2 * blockIdx.x + 1] = 0.0; }
  }
}

inline int blocks_for(int64_t items) { return (int)std::min<int64_t>(EIGS_BLOCKS, std::max<int64_t>(1, (items + BS - 1) / BS)); }

template <int KB>
void launch_rotate(sd_ctx *ctx, double *V, int64_t ld, int64_t n, int m, int k, const double *Qd) {
  const bool pair = (ld % 2 == 0) && !((uintptr_t)V & 15);
  const size_t lds = sizeof(double) * (size_t)m * KB;
  if (pair) hipLaunchKernelGGL((k_basis_rotate<KB, 2>), dim3(blocks_for((n + 1) / 2)), dim3(BS), lds, ctx->stream, V, ld, n, m, k, Qd);
  else hipLaunchKernelGGL((k_basis_rotate<KB, 1>), dim3(blocks_for(n)), dim3(BS), lds, ctx->stream, V, ld, n, m, k, Qd);
}

}  // namespace

// doubles of ctx->d_partials the three launchers below use (sd_ensure_partials is theirs)
static size_t eigs_partials() { return (size_t)EIGS_BLOCKS * 2 * EIGS_B; }

int sd_k_basis_rotate(sd_ctx *ctx, double *V, int64_t ld, int64_t n, int m, const double *Q_dev, int k) {
  if (m < 1 || k < 1 || k > m || m > SD_EIGS_MAX_BASIS || k > SD_EIGS_MAX_KEEP || n < 0 || ld < n || !V || !Q_dev)
    return sd_set_err(ctx, SD_EARG, "basis rotation: need 1 <= k <= m <= 128, k <= 32 and ld >= n");
  if (n == 0) return SD_OK;
  if (k <= 4) launch_rotate<4>(ctx, V, ld, n, m, k, Q_dev);
  else if (k <= 8) launch_rotate<8>(ctx, V, ld, n, m, k, Q_dev);
  else if (k <= 16) launch_rotate<16>(ctx, V, ld, n, m, k, Q_dev);
  else launch_rotate<32>(ctx, V, ld, n, m, k, Q_dev);
  SD_HIP(ctx, hipGetLastError());
  return SD_OK;
}

int sd_k_block_dots(sd_ctx *ctx, int nc, const double *V, int64_t ld, int ncols, const double *w, int64_t N, double *out_dev) {
  if (ncols < 1 || ncols > EIGS_B || (nc != 1 && nc != 2)) return sd_set_err(ctx, SD_EARG, "block dots: 1 to 8 columns");
  int rc = sd_ensure_partials(ctx, eigs_partials()); if (rc) return rc;
  const int nb = blocks_for(N);
  if (nc == 2) hipLaunchKernelGGL(k_block_dots<2>, dim3(nb), dim3(BS), 0, ctx->stream, V, ld, ncols, w, N, ctx->d_partials);
  else hipLaunchKernelGGL(k_block_dots<1>, dim3(nb), dim3(BS), 0, ctx->stream, V, ld, ncols, w, N, ctx->d_partials);
  hipLaunchKernelGGL(k_eigs_reduce, dim3(1), dim3(64 * 2 * EIGS_B), 0, ctx->stream, ctx->d_partials, nb, 2 * EIGS_B, 2 * ncols, out_dev);
  SD_HIP(ctx, hipGetLastError());
  return SD_OK;
}

int sd_k_block_axpy(sd_ctx *ctx, int nc, double *w, const double *V, int64_t ld, int ncols, const double *coef_dev, int64_t N,
                    double *n2_dev) {
  if (ncols < 1 || ncols > EIGS_B || (nc != 1 && nc != 2)) return sd_set_err(ctx, SD_EARG, "block subtraction: 1 to 8 columns");
  int rc = sd_ensure_partials(ctx, eigs_partials()); if (rc) return rc;
  const int nb = blocks_for(N);
  if (n2_dev) {
    if (nc == 2) hipLaunchKernelGGL((k_block_axpy<2, true>), dim3(nb), dim3(BS), 0, ctx->stream, w, V, ld, ncols, coef_dev, N, ctx->d_partials);
    else hipLaunchKernelGGL((k_block_axpy<1, true>), dim3(nb), dim3(BS), 0, ctx->stream, w, V, ld, ncols, coef_dev, N, ctx->d_partials);
    hipLaunchKernelGGL(k_eigs_reduce, dim3(1), dim3(64 * 2 * EIGS_B), 0, ctx->stream, ctx->d_partials, nb, 2, 1, n2_dev);
  } else {
    if (nc == 2) hipLaunchKernelGGL((k_block_axpy<2, false>), dim3(nb), dim3(BS), 0, ctx->stream, w, V, ld, ncols, coef_dev, N, (double *)nullptr);
    else hipLaunchKernelGGL((k_block_axpy<1, false>), dim3(nb), dim3(BS), 0, ctx->stream, w, V, ld, ncols, coef_dev, N, (double *)nullptr);
  }
  SD_HIP(ctx, hipGetLastError());
  return SD_OK;
}
