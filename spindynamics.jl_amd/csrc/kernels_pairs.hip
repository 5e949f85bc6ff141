// Equal-time pair correlations: for site pairs i <= j (bits bi <= bj) of one state psi, nothing divided by <psi|psi>,
//     PM : G_ij = <psi| S^+_i S^-_j |psi> = sum over rows s with site j up and site i down of conj(psi[s']) psi[s],
//          s' = s with the up spin moved from j to i;   G_ii = sum_s |psi[s]|^2 [site i up];   G_ji = conj(G_ij) (host)
//     ZZ : Z_ij = <psi| S^z_i S^z_j |psi> = (1/4) sum_s (+-|psi[s]|^2), + when the two sites agree (so Z_ii = <psi|psi> / 4).
// One gather kernel.  Workgroup column blockIdx.x owns a chunk of SD_PAIR_CHUNK pairs of the host's list, blockIdx.y a share of the
// rows; a thread reads psi[s] once per row and keeps one complex accumulator per pair of its chunk (16 doubles, as k_site_chunk).
// The chunk is the FAST grid index, so the workgroups in flight together read the same rows for different pairs and psi is
// streamed from memory about once, not once per chunk.
// Row configurations (MODE), as k_current: 1 the tile's prefix and the suffix table of a tiled sector plan, 0 unrank_g of the row
// (sector plans without tiles), 2 the row index (full basis).  Partner row s':
//   MODE 2: idx ^ mask.
//   MODE 1: the plan's own rank, idx0(s') = addr[prefix of s'] + suf_rank[suffix of s'] (sd_internal.hpp), two cached loads.
//   MODE 0: a LOCAL rank difference, O(bj - bi) lookups instead of O(L), the binomials in LDS as in k_current; for neighbours the
//           walk is empty and the two end terms are k_current's closed form by Pascal's rule (pair_partner, device_common.hpp).
// Sums: per thread, block_reduce2 per pair, block partials in ctx->d_partials, k_pairs_reduce adds them in a fixed order.  No
// atomics, and the grid depends on the plan alone: the same call gives the same bits.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "device_common.hpp"

using namespace sd_dev;

namespace {

#define SD_PAIR_CHUNK 8          // pairs per workgroup column
#define SD_PAIR_ROW (2 * SD_PAIR_CHUNK)   // doubles of a block's partial row
#define SD_PAIR_MAX_BLOCKS 2048  // row blocks (grid.y): tiles of a tiled plan, else blocks of 256 rows, capped here

// NC: components of psi.  pairs[k] = bi | bj << 8 (0-based bits, bi <= bj).  PM false: the ZZ form (sums before the factor 1/4).
template <int NC, bool PM, int MODE>
__global__ __launch_bounds__(256) void k_pairs(sd_dev_model dm, const double *__restrict__ psi, const int *__restrict__ pairs,
                                               int npairs, double *__restrict__ partials) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  double *red = reinterpret_cast<double *>(smem);            // 32 doubles
  int64_t *lbin = reinterpret_cast<int64_t *>(red + 32);     // lbin[n * K + k] = C(n, k), n < L, k <= nup (the rank walk only)
  const int K = (dm.nup > 0 ? dm.nup : 0) + 1;
  if (PM && MODE == 0) {
    for (int k = threadIdx.x; k < dm.L * K; k += 256) lbin[k] = dm.binom[(k / K) * (SD_MAX_L + 1) + (k % K)];
    __syncthreads();
  }
  const int c0 = blockIdx.x * SD_PAIR_CHUNK, cn = min(SD_PAIR_CHUNK, npairs - c0);
  int pb[SD_PAIR_CHUNK];
  double ar[SD_PAIR_CHUNK], ai[SD_PAIR_CHUNK];
#pragma unroll
  for (int k = 0; k < SD_PAIR_CHUNK; ++k) { pb[k] = k < cn ? pairs[c0 + k] : 0; ar[k] = 0.0; ai[k] = 0.0; }
  auto row = [&](uint64_t s, int64_t idx) {
    double vr, vi = 0.0;
    if (NC == 2) { const double2 v = ((const double2 *)psi)[idx]; vr = v.x; vi = v.y; }
    else vr = psi[idx];
    const double w = NC == 2 ? vr * vr + vi * vi : vr * vr;
#pragma unroll
    for (int k = 0; k < SD_PAIR_CHUNK; ++k) {
      const int bi = pb[k] & 255, bj = pb[k] >> 8;
      const bool ui = (s >> bi) & 1, uj = (s >> bj) & 1;
      if (k >= cn) continue;
      if (!PM) { ar[k] += ui == uj ? w : -w; continue; }
      double dr = w, di = 0.0;                               // bi == bj: |psi[s]|^2 when the site is up
      bool hit = uj;
      if (bi != bj) {
        hit = uj && !ui;
        if (hit) {
          const int64_t partner = pair_partner<MODE>(dm, lbin, K, s, idx, bi, bj);
          if (NC == 2) {
            const double2 u = ((const double2 *)psi)[partner];
            dr = u.x * vr + u.y * vi;                        // conj(psi[s']) * psi[s]
            di = u.x * vi - u.y * vr;
          } else {
            dr = psi[partner] * vr;
          }
        }
      }
      if (hit) { ar[k] += dr; ai[k] += di; }
    }
  };
  if (MODE == 1) {
    for (int t = blockIdx.y; t < dm.n_tiles; t += gridDim.y) {
      const uint32_t P = dm.tile_prefix[t];
      const int64_t base = dm.tile_base[t];
      const int t2 = dm.nup - __popc(P);
      const int len = (int)binom_g(dm, dm.LS, t2);
      const uint16_t *__restrict__ sufS = dm.suf_states + dm.suf_off[t2];
      for (int i = threadIdx.x; i < len; i += 256) row((uint64_t)P | ((uint64_t)sufS[i] << dm.p), base + i);
    }
  } else {
    const int64_t stride = (int64_t)gridDim.y * 256;
    for (int64_t idx = (int64_t)blockIdx.y * 256 + threadIdx.x; idx < dm.n_local; idx += stride)
      row(MODE == 2 ? (uint64_t)idx : unrank_g(dm, idx), idx);
  }
  double *__restrict__ prow = partials + ((size_t)blockIdx.x * gridDim.y + blockIdx.y) * SD_PAIR_ROW;
#pragma unroll
  for (int k = 0; k < SD_PAIR_CHUNK; ++k) {
    double a = ar[k], b = ai[k];
    block_reduce2(a, b, red);
    if (threadIdx.x == 0) { prow[2 * k] = a; prow[2 * k + 1] = b; }
    __syncthreads();
  }
}

// Block c sums the partial rows of chunk c in a fixed order (16 strided sums per column, then their sum) and files
// out[2 pair .. +1] = scale * sum for the pairs of the chunk.
__global__ __launch_bounds__(256) void k_pairs_reduce(const double *__restrict__ partials, int nblocks, int npairs, double scale,
                                                      double *__restrict__ out) {
  __shared__ double sm[16][SD_PAIR_ROW];
  const int c = threadIdx.x & (SD_PAIR_ROW - 1), j = threadIdx.x >> 4;
  const double *__restrict__ p = partials + (size_t)blockIdx.x * nblocks * SD_PAIR_ROW;
  double a = 0.0;
  for (int b = j; b < nblocks; b += 16) a += p[(size_t)b * SD_PAIR_ROW + c];
  sm[j][c] = a;
  __syncthreads();
  if (threadIdx.x < SD_PAIR_ROW) {
    double t = 0.0;
    for (int jj = 0; jj < 16; ++jj) t += sm[jj][c];
    const int pair = blockIdx.x * SD_PAIR_CHUNK + (c >> 1);
    if (pair < npairs) out[2 * (size_t)pair + (c & 1)] = scale * t;
  }
}

template <int NC, bool PM>
void launch_mode(int mode, dim3 grid, size_t shmem, hipStream_t st, const sd_dev_model &dm, const double *psi, const int *pairs,
                 int npairs, double *partials) {
  if (mode == 1) hipLaunchKernelGGL((k_pairs<NC, PM, 1>), grid, dim3(256), shmem, st, dm, psi, pairs, npairs, partials);
  else if (mode == 2) hipLaunchKernelGGL((k_pairs<NC, PM, 2>), grid, dim3(256), shmem, st, dm, psi, pairs, npairs, partials);
  else hipLaunchKernelGGL((k_pairs<NC, PM, 0>), grid, dim3(256), shmem, st, dm, psi, pairs, npairs, partials);
}

}  // namespace

// dst[2k .. +1] (device) = (re, im) of the correlation of pair k of pairs_dev (npairs entries bi | bj << 8, 0-based bits,
// bi <= bj < L): SD_PAIR_PM G_ij, SD_PAIR_ZZ (Z_ij, 0).  psi of `dtype` on the device.  Queued on the context's stream.
int sd_launch_pair_correlations(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi, int component, const int *pairs_dev,
                                int npairs, double *dst) {
  if (!m->dev_ready) return sd_set_err(ctx, SD_EARG, "model has no device tables (created without a context)");
  if (dtype != SD_F64 && dtype != SD_C128) return sd_set_err(ctx, SD_EARG, "dtype must be SD_F64 or SD_C128");
  if (component != SD_PAIR_ZZ && component != SD_PAIR_PM) return sd_set_err(ctx, SD_EARG, "component must be SD_PAIR_ZZ or SD_PAIR_PM");
  if (m->nranks != 1) return sd_set_err(ctx, SD_EARG, "pair correlations need an unsharded model");
  if (npairs < 1 || npairs > SD_MAX_L * (SD_MAX_L + 1) / 2) return sd_set_err(ctx, SD_EINTERNAL, "pair correlations: bad pair count");
  const sd_dev_model &dm = m->dm;
  if (dm.n_local == 0) {      // no rows: every sum is empty
    SD_HIP(ctx, hipMemsetAsync(dst, 0, 2 * (size_t)npairs * sizeof(double), ctx->stream));
    return SD_OK;
  }
  const int mode = dm.nup < 0 ? 2 : (m->p >= 0 && dm.n_tiles > 0) ? 1 : 0;
  const int64_t nb64 = mode == 1 ? (int64_t)dm.n_tiles : (dm.n_local + 255) / 256;
  const unsigned nb = (unsigned)std::min<int64_t>(nb64, SD_PAIR_MAX_BLOCKS);
  const unsigned nchunks = (unsigned)((npairs + SD_PAIR_CHUNK - 1) / SD_PAIR_CHUNK);
  const bool pm = component == SD_PAIR_PM;
  const size_t shmem = 32 * sizeof(double) + (pm && mode == 0 ? (size_t)dm.L * (size_t)(dm.nup + 1) * sizeof(int64_t) : 0);
  int rc = sd_ensure_partials(ctx, (size_t)nchunks * nb * SD_PAIR_ROW);
  if (rc) return rc;
  const dim3 grid(nchunks, nb);
  const double *v = (const double *)psi;
  if (dtype == SD_C128) {
    if (pm) launch_mode<2, true>(mode, grid, shmem, ctx->stream, dm, v, pairs_dev, npairs, ctx->d_partials);
    else launch_mode<2, false>(mode, grid, shmem, ctx->stream, dm, v, pairs_dev, npairs, ctx->d_partials);
  } else {
    if (pm) launch_mode<1, true>(mode, grid, shmem, ctx->stream, dm, v, pairs_dev, npairs, ctx->d_partials);
    else launch_mode<1, false>(mode, grid, shmem, ctx->stream, dm, v, pairs_dev, npairs, ctx->d_partials);
  }
  hipLaunchKernelGGL(k_pairs_reduce, dim3(nchunks), dim3(256), 0, ctx->stream, ctx->d_partials, (int)nb, npairs, pm ? 1.0 : 0.25, dst);
  SD_HIP(ctx, hipGetLastError());
  return SD_OK;
}
