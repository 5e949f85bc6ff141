// Bond operators and dimer correlations.  For a bond b = (i, j), i != j, and two real weights,
//     D_b = xy/2 (S^+_i S^-_j + S^-_i S^+_j) + zz S^z_i S^z_j        (xy = zz = 1: S_i . S_j),
// on a row with configuration s:  (D_b psi)(s) = +-(zz/4) psi(s), + when the two sites agree, and, when they differ,
// + (xy/2) psi(s'), s' = s with the two sites exchanged.  One multiply, and one multiply and add, per component (bond_value).
//   k_bond_apply : out = D_b psi, every row written.
//   k_dimer_gram : for a list of B bonds, D_ab = <psi|D_a D_b|psi> = sum_s conj((D_a psi)(s)) (D_b psi)(s) and
//                  e_b = <psi|D_b|psi> = Re sum_s conj(psi(s)) (D_b psi)(s); no vector D_b psi is stored, nothing divided by <psi|psi>.
// The bonds are cut into chunks of SD_DIMER_CHUNK = 4.  Workgroup column blockIdx.x owns one tile (chunk ca <= chunk cb) of 4 x 4
// entries, blockIdx.y a share of the rows.  A thread reads psi(s) once per row, gathers the at most 8 partners of its two chunks
// (4 on a diagonal tile, whose two chunks are one), and adds the 16 products into register accumulators: 16 complex, 16 real
// for a Float64 psi.  The e_b come from the diagonal tiles, from the same values.  The tile is the FAST grid index, so the
// workgroups in flight together read the same rows and psi is streamed from memory about once, not once per tile.
// Only the tiles ca <= cb are summed; the host fills the other triangle with the conjugate (and inside a diagonal tile uses
// a <= b only), so the matrix is Hermitian to the bit.
// Rows and their configurations (MODE) by for_rows, the partner of either orientation by bond_partner (gather_common.hpp).
// Sums: per thread, block_reduce2, block partials in ctx->d_partials, k_dimer_reduce adds them in a fixed order.  No atomics, and
// the grid depends on the plan and B alone: the same call gives the same bits.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "gather_common.hpp"

using namespace sd_dev;

namespace {

#define SD_DIMER_CHUNK 4                                   // bonds per chunk; a tile is CHUNK x CHUNK entries
#define SD_DIMER_ROW (2 * SD_DIMER_CHUNK * SD_DIMER_CHUNK + SD_DIMER_CHUNK)   // doubles of a block's partial row: 16 (re, im), then 4 e
#define SD_DIMER_RED_GROUPS 7                              // k_dimer_reduce: 7 strided sums per column (7 * 36 = 252 threads)
#define SD_DIMER_MAX_BLOCKS 2048  // row blocks (grid.y): tiles of a tiled plan, else blocks of 256 rows, capped here (as SD_PAIR_MAX_BLOCKS)

// psi[idx] = (vr, vi) on the row with configuration s -> (D_b psi)(s) for the bond pb = bi | bj << 8 (0-based bits, bi < bj),
// cz = zz / 4, cx = xy / 2
template <int NC, int MODE>
__device__ __forceinline__ void bond_value(const sd_dev_model &dm, const int64_t *lbin, int K, const double *__restrict__ psi,
                                           uint64_t s, int64_t idx, double vr, double vi, int pb, double cz, double cx, double &dr,
                                           double &di) {
  const int bi = pb & 255, bj = pb >> 8;
  const bool ui = (s >> bi) & 1, uj = (s >> bj) & 1;
  const double c = ui == uj ? cz : -cz;
  dr = c * vr;
  di = NC == 2 ? c * vi : 0.0;
  if (ui != uj) {
    const int64_t partner = bond_partner<MODE>(dm, lbin, K, s, idx, bi, bj);
    if (NC == 2) {
      const double2 u = ((const double2 *)psi)[partner];
      dr = dr + cx * u.x;
      di = di + cx * u.y;
    } else {
      dr = dr + cx * psi[partner];
    }
  }
}

template <int NC, int MODE>
__global__ __launch_bounds__(256) void k_bond_apply(sd_dev_model dm, const double *__restrict__ psi, int pb, double cz, double cx,
                                                    double *__restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  int64_t *lbin = reinterpret_cast<int64_t *>(smem);
  const int K = (dm.nup > 0 ? dm.nup : 0) + 1;
  fill_lbin<MODE>(dm, lbin, K);
  for_rows<MODE>(dm, blockIdx.y, gridDim.y, [&](uint64_t s, int64_t idx) {
    double vr, vi = 0.0, dr, di;
    if (NC == 2) { const double2 v = ((const double2 *)psi)[idx]; vr = v.x; vi = v.y; }
    else vr = psi[idx];
    bond_value<NC, MODE>(dm, lbin, K, psi, s, idx, vr, vi, pb, cz, cx, dr, di);
    if (NC == 2) ((double2 *)out)[idx] = make_double2(dr, di);
    else out[idx] = dr;
  });
}

// bonds[k] = bi | bj << 8, k < B.  Tile blockIdx.x = (ca, cb), ca <= cb, counted row by row of the upper triangle of chunks.
template <int NC, int MODE>
__global__ __launch_bounds__(256) void k_dimer_gram(sd_dev_model dm, const double *__restrict__ psi, const int *__restrict__ bonds,
                                                    int B, double cz, double cx, double *__restrict__ partials) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  double *red = reinterpret_cast<double *>(smem);            // 32 doubles
  int64_t *lbin = reinterpret_cast<int64_t *>(red + 32);
  const int K = (dm.nup > 0 ? dm.nup : 0) + 1;
  fill_lbin<MODE>(dm, lbin, K);
  const int nc = (B + SD_DIMER_CHUNK - 1) / SD_DIMER_CHUNK;
  int ca = 0, cb = (int)blockIdx.x;
  while (cb >= nc - ca) { cb -= nc - ca; ++ca; }
  cb += ca;
  const bool diag = ca == cb;
  const int na = min(SD_DIMER_CHUNK, B - ca * SD_DIMER_CHUNK), nb = min(SD_DIMER_CHUNK, B - cb * SD_DIMER_CHUNK);
  int pa[SD_DIMER_CHUNK], pbb[SD_DIMER_CHUNK];
  double ar[SD_DIMER_CHUNK][SD_DIMER_CHUNK], ai[SD_DIMER_CHUNK][SD_DIMER_CHUNK], er[SD_DIMER_CHUNK];
#pragma unroll
  for (int k = 0; k < SD_DIMER_CHUNK; ++k) {
    pa[k] = k < na ? bonds[ca * SD_DIMER_CHUNK + k] : 0;
    pbb[k] = k < nb ? bonds[cb * SD_DIMER_CHUNK + k] : 0;
    er[k] = 0.0;
#pragma unroll
    for (int l = 0; l < SD_DIMER_CHUNK; ++l) { ar[k][l] = 0.0; ai[k][l] = 0.0; }
  }
  for_rows<MODE>(dm, blockIdx.y, gridDim.y, [&](uint64_t s, int64_t idx) {
    double vr, vi = 0.0;
    if (NC == 2) { const double2 v = ((const double2 *)psi)[idx]; vr = v.x; vi = v.y; }
    else vr = psi[idx];
    double xr[SD_DIMER_CHUNK], xi[SD_DIMER_CHUNK];           // (D_a psi)(s), a in chunk ca; a bond past the list: 0
#pragma unroll
    for (int a = 0; a < SD_DIMER_CHUNK; ++a) {
      xr[a] = 0.0; xi[a] = 0.0;
      if (a < na) bond_value<NC, MODE>(dm, lbin, K, psi, s, idx, vr, vi, pa[a], cz, cx, xr[a], xi[a]);
    }
#pragma unroll
    for (int b = 0; b < SD_DIMER_CHUNK; ++b) {
      double yr = xr[b], yi = xi[b];                         // (D_b psi)(s), b in chunk cb
      if (!diag) {
        yr = 0.0; yi = 0.0;
        if (b < nb) bond_value<NC, MODE>(dm, lbin, K, psi, s, idx, vr, vi, pbb[b], cz, cx, yr, yi);
      }
#pragma unroll
      for (int a = 0; a < SD_DIMER_CHUNK; ++a) {             // conj(x_a) y_b
        if (NC == 2) {
          ar[a][b] += xr[a] * yr + xi[a] * yi;
          ai[a][b] += xr[a] * yi - xi[a] * yr;
        } else {
          ar[a][b] += xr[a] * yr;
        }
      }
    }
    if (diag) {
#pragma unroll
      for (int a = 0; a < SD_DIMER_CHUNK; ++a) er[a] += NC == 2 ? vr * xr[a] + vi * xi[a] : vr * xr[a];
    }
  });
  double *__restrict__ prow = partials + ((size_t)blockIdx.x * gridDim.y + blockIdx.y) * SD_DIMER_ROW;
#pragma unroll
  for (int a = 0; a < SD_DIMER_CHUNK; ++a) {
#pragma unroll
    for (int b = 0; b < SD_DIMER_CHUNK; ++b) {
      double x = ar[a][b], y = ai[a][b];
      block_reduce2(x, y, red);
      if (threadIdx.x == 0) { prow[2 * (a * SD_DIMER_CHUNK + b)] = x; prow[2 * (a * SD_DIMER_CHUNK + b) + 1] = y; }
      __syncthreads();
    }
  }
#pragma unroll
  for (int a = 0; a < SD_DIMER_CHUNK; a += 2) {
    double x = er[a], y = er[a + 1];
    block_reduce2(x, y, red);
    if (threadIdx.x == 0) { prow[2 * SD_DIMER_CHUNK * SD_DIMER_CHUNK + a] = x; prow[2 * SD_DIMER_CHUNK * SD_DIMER_CHUNK + a + 1] = y; }
    __syncthreads();
  }
}

// Block t sums the partial rows of tile t in a fixed order (7 strided sums per column, then their sum): out[t * SD_DIMER_ROW + c].
__global__ __launch_bounds__(256) void k_dimer_reduce(const double *__restrict__ partials, int nblocks, double *__restrict__ out) {
  __shared__ double sm[SD_DIMER_RED_GROUPS][SD_DIMER_ROW];
  const int c = threadIdx.x % SD_DIMER_ROW, j = threadIdx.x / SD_DIMER_ROW;
  const double *__restrict__ p = partials + (size_t)blockIdx.x * nblocks * SD_DIMER_ROW;
  if (j < SD_DIMER_RED_GROUPS) {
    double a = 0.0;
    for (int b = j; b < nblocks; b += SD_DIMER_RED_GROUPS) a += p[(size_t)b * SD_DIMER_ROW + c];
    sm[j][c] = a;
  }
  __syncthreads();
  if (threadIdx.x < SD_DIMER_ROW) {
    double t = 0.0;
    for (int jj = 0; jj < SD_DIMER_RED_GROUPS; ++jj) t += sm[jj][c];
    out[(size_t)blockIdx.x * SD_DIMER_ROW + c] = t;
  }
}

int check_model(sd_ctx *ctx, const sd_model *m, int dtype) {
  return sd_gather_check(ctx, m, dtype, "bond operators and dimer correlations need");
}

}  // namespace

// out (device, psi's dtype, must not alias psi) = D_b psi for the bond of the 0-based bits bi < bj < L.  Queued on the context's stream.
int sd_launch_bond_apply(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi, int bi, int bj, double xy, double zz, void *out) {
  int rc = check_model(ctx, m, dtype);
  if (rc) return rc;
  if (bi < 0 || bi >= bj || bj >= m->L) return sd_set_err(ctx, SD_EINTERNAL, "bond apply: bad bond");
  const sd_dev_model &dm = m->dm;
  if (dm.n_local == 0) return SD_OK;
  const sd_gather_grid g = sd_gather_grid_of(m, SD_DIMER_MAX_BLOCKS, SD_DIMER_MAX_BLOCKS);
  const dim3 grid(1, g.nb);
  const int pb = bi | (bj << 8);
  const double cz = zz * 0.25, cx = xy * 0.5;
  const double *v = (const double *)psi;
  double *o = (double *)out;
  sd_with_mode(g.mode, [&](auto M) {
    constexpr int MODE = decltype(M)::value;
    if (dtype == SD_C128) hipLaunchKernelGGL((k_bond_apply<2, MODE>), grid, dim3(256), g.lbin_bytes, ctx->stream, dm, v, pb, cz, cx, o);
    else hipLaunchKernelGGL((k_bond_apply<1, MODE>), grid, dim3(256), g.lbin_bytes, ctx->stream, dm, v, pb, cz, cx, o);
  });
  SD_HIP(ctx, hipGetLastError());
  return SD_OK;
}

int sd_dimer_tiles(int B) {
  const int nc = (B + SD_DIMER_CHUNK - 1) / SD_DIMER_CHUNK;
  return nc * (nc + 1) / 2;
}

// dst (device, sd_dimer_tiles(B) * SD_DIMER_TILE_ROW doubles): per tile (ca <= cb, the upper triangle of chunks of 4 bonds row by
// row) (re, im) of D_ab at [2 (4 a + b)], a in chunk ca and b in chunk cb, then on the diagonal tiles e_a at [32 + a].  bonds_dev: B
// device ints bi | bj << 8, 0-based bits, bi < bj < L.  Queued on the context's stream.
int sd_launch_dimer_gram(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi, const int *bonds_dev, int B, double xy, double zz,
                         double *dst) {
  static_assert(SD_DIMER_ROW == SD_DIMER_TILE_ROW, "partial row layout");
  int rc = check_model(ctx, m, dtype);
  if (rc) return rc;
  if (B < 1 || B > SD_DIMER_MAX_BONDS) return sd_set_err(ctx, SD_EINTERNAL, "dimer correlations: bad bond count");
  const sd_dev_model &dm = m->dm;
  const unsigned ntiles = (unsigned)sd_dimer_tiles(B);
  if (dm.n_local == 0) {      // no rows: every sum is empty
    SD_HIP(ctx, hipMemsetAsync(dst, 0, (size_t)ntiles * SD_DIMER_ROW * sizeof(double), ctx->stream));
    return SD_OK;
  }
  const sd_gather_grid g = sd_gather_grid_of(m, SD_DIMER_MAX_BLOCKS, SD_DIMER_MAX_BLOCKS);
  const unsigned nb = g.nb;
  const size_t shmem = 32 * sizeof(double) + g.lbin_bytes;
  rc = sd_ensure_partials(ctx, (size_t)ntiles * nb * SD_DIMER_ROW);
  if (rc) return rc;
  const dim3 grid(ntiles, nb);
  const double cz = zz * 0.25, cx = xy * 0.5;
  const double *v = (const double *)psi;
  sd_with_mode(g.mode, [&](auto M) {
    constexpr int MODE = decltype(M)::value;
    if (dtype == SD_C128)
      hipLaunchKernelGGL((k_dimer_gram<2, MODE>), grid, dim3(256), shmem, ctx->stream, dm, v, bonds_dev, B, cz, cx, ctx->d_partials);
    else
      hipLaunchKernelGGL((k_dimer_gram<1, MODE>), grid, dim3(256), shmem, ctx->stream, dm, v, bonds_dev, B, cz, cx, ctx->d_partials);
  });
  hipLaunchKernelGGL(k_dimer_reduce, dim3(ntiles), dim3(256), 0, ctx->stream, ctx->d_partials, (int)nb, dst);
  SD_HIP(ctx, hipGetLastError());
  return SD_OK;
}
