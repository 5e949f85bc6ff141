// Equal-time pair correlations: for site pairs i <= j (bits bi <= bj) of one state psi, nothing divided by <psi|psi>,
//     PM : G_ij = <psi| S^+_i S^-_j |psi> = sum over rows s with site j up and site i down of conj(psi[s']) psi[s],
//          s' = s with the up spin moved from j to i;   G_ii = sum_s |psi[s]|^2 [site i up];   G_ji = conj(G_ij) (host)
//     ZZ : Z_ij = <psi| S^z_i S^z_j |psi> = (1/4) sum_s (+-|psi[s]|^2), + when the two sites agree (so Z_ii = <psi|psi> / 4).
// One gather kernel.  Workgroup column blockIdx.x owns a chunk of SD_PAIR_CHUNK pairs of the host's list, blockIdx.y a share of the
// rows; a thread reads psi[s] once per row and keeps one complex accumulator per pair of its chunk (16 doubles, as k_site_chunk).
// The chunk is the FAST grid index, so the workgroups in flight together read the same rows for different pairs and psi is
// streamed from memory about once, not once per chunk.
// Rows and their configurations (MODE) by for_rows (gather_common.hpp): 1 the tile's prefix and the suffix table of a tiled sector
// plan, 0 unrank_g of the row (sector plans without tiles), 2 the row index (full basis).  Partner row s':
//   MODE 2: idx ^ mask.
//   MODE 1: the plan's own rank, idx0(s') = addr[prefix of s'] + suf_rank[suffix of s'] (sd_internal.hpp), two cached loads.
//   MODE 0: a LOCAL rank difference, O(bj - bi) lookups instead of O(L), the binomials in LDS as in k_current; for neighbours the
//           walk is empty and the two end terms are k_current's closed form by Pascal's rule (pair_partner, gather_common.hpp).
// Sums: per thread, block_reduce2 per pair, block partials in ctx->d_partials, k_chunk_reduce adds them in a fixed order.  No
// atomics, and the grid depends on the plan alone: the same call gives the same bits.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "gather_common.hpp"

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
  if (PM) fill_lbin<MODE>(dm, lbin, K);
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
  for_rows<MODE>(dm, blockIdx.y, gridDim.y, row);
  double *__restrict__ prow = partials + ((size_t)blockIdx.x * gridDim.y + blockIdx.y) * SD_PAIR_ROW;
#pragma unroll
  for (int k = 0; k < SD_PAIR_CHUNK; ++k) {
    double a = ar[k], b = ai[k];
    block_reduce2(a, b, red);
    if (threadIdx.x == 0) { prow[2 * k] = a; prow[2 * k + 1] = b; }
    __syncthreads();
  }
}

template <int NC, bool PM>
void launch_mode(int mode, dim3 grid, size_t shmem, hipStream_t st, const sd_dev_model &dm, const double *psi, const int *pairs,
                 int npairs, double *partials) {
  sd_with_mode(mode, [&](auto M) {
    hipLaunchKernelGGL((k_pairs<NC, PM, decltype(M)::value>), grid, dim3(256), shmem, st, dm, psi, pairs, npairs, partials);
  });
}

}  // namespace

// dst[2k .. +1] (device) = (re, im) of the correlation of pair k of pairs_dev (npairs entries bi | bj << 8, 0-based bits,
// bi <= bj < L): SD_PAIR_PM G_ij, SD_PAIR_ZZ (Z_ij, 0).  psi of `dtype` on the device.  Queued on the context's stream.
int sd_launch_pair_correlations(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi, int component, const int *pairs_dev,
                                int npairs, double *dst) {
  if (int rc = sd_gather_check(ctx, m, dtype, "pair correlations need")) return rc;
  if (component != SD_PAIR_ZZ && component != SD_PAIR_PM) return sd_set_err(ctx, SD_EARG, "component must be SD_PAIR_ZZ or SD_PAIR_PM");
  if (npairs < 1 || npairs > SD_MAX_L * (SD_MAX_L + 1) / 2) return sd_set_err(ctx, SD_EINTERNAL, "pair correlations: bad pair count");
  const sd_dev_model &dm = m->dm;
  if (dm.n_local == 0) {      // no rows: every sum is empty
    SD_HIP(ctx, hipMemsetAsync(dst, 0, 2 * (size_t)npairs * sizeof(double), ctx->stream));
    return SD_OK;
  }
  const sd_gather_grid g = sd_gather_grid_of(m, SD_PAIR_MAX_BLOCKS, SD_PAIR_MAX_BLOCKS);
  const int mode = g.mode;
  const unsigned nb = g.nb;
  const unsigned nchunks = (unsigned)((npairs + SD_PAIR_CHUNK - 1) / SD_PAIR_CHUNK);
  const bool pm = component == SD_PAIR_PM;
  const size_t shmem = 32 * sizeof(double) + (pm ? g.lbin_bytes : 0);
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
  hipLaunchKernelGGL(k_chunk_reduce<SD_PAIR_CHUNK>, dim3(nchunks), dim3(256), 0, ctx->stream, ctx->d_partials, (int)nb, npairs, pm ? 1.0 : 0.25, dst);
  SD_HIP(ctx, hipGetLastError());
  return SD_OK;
}
