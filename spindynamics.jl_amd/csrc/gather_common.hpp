// The shared scaffold of the gather kernels: a thread visits a basis row, reconstructs its configuration s, looks up
// one or more partner rows and writes or sums.  Header-only, included by the gather *.hip files; the apply path keeps
// device_common.hpp to itself.
// Where the row's configuration comes from is a template MODE, chosen per model by sd_gather_mode:
//   1  a tiled sector plan: the tile's prefix and the suffix table, one tile per workgroup at a time, strided by the grid;
//   0  a sector plan without tiles: unrank_g of the row, a grid-stride loop over the rows;
//   2  the full basis: the row index is the configuration, the same grid-stride loop.
// A new gather kernel takes its rows from for_rows (or for_tiles, when it has work per tile), its binomials from fill_lbin, its
// grid from sd_gather_grid_of and its MODE from sd_with_mode; it does not copy them.
#pragma once
#include <algorithm>
#include <string>
#include <type_traits>

#include "device_common.hpp"

// ---- host side ----

// The one copy of the mode rule.  Not sd_model_path (capi.cpp), which names the APPLY path: that one says 2 only for a full basis
// with its own suffix tiles (full_ls > 0) and 0 for a full basis below L = 12; here 2 is the full basis at any L, because the row
// index is the configuration whatever the apply does.  1 needs the tiles to exist (a plan with p >= 0 and no tile stays 0).
inline int sd_gather_mode(const sd_model *m) { return m->dm.nup < 0 ? 2 : (m->p >= 0 && m->dm.n_tiles > 0) ? 1 : 0; }

// nb: workgroups along the row axis, the tiles of a tiled plan capped at cap_tiles, else the blocks of 256 rows capped at cap_rows
// (no lower clamp: a launcher that wants at least one block says so).  lbin_bytes: the LDS copy of the binomials, MODE 0 only.
struct sd_gather_grid { int mode; unsigned nb; size_t lbin_bytes; };
inline sd_gather_grid sd_gather_grid_of(const sd_model *m, int64_t cap_tiles, int64_t cap_rows) {
  const sd_dev_model &dm = m->dm;
  sd_gather_grid g;
  g.mode = sd_gather_mode(m);
  const int64_t nb64 = g.mode == 1 ? (int64_t)dm.n_tiles : (dm.n_local + 255) / 256;
  g.nb = (unsigned)std::min<int64_t>(nb64, g.mode == 1 ? cap_tiles : cap_rows);
  g.lbin_bytes = g.mode == 0 ? (size_t)dm.L * (size_t)(dm.nup + 1) * sizeof(int64_t) : 0;
  return g;
}

// f(std::integral_constant<int, MODE>{}) for the run-time mode: the one place a mode becomes a template argument.
template <class F>
inline void sd_with_mode(int mode, F &&f) {
  if (mode == 1) f(std::integral_constant<int, 1>{});
  else if (mode == 2) f(std::integral_constant<int, 2>{});
  else f(std::integral_constant<int, 0>{});
}

// The argument checks the gather launchers share.  who: the feature with its verb ("symmetry operators need"); need_L adds the
// check of the configuration width for the kernels that shift by L.
inline int sd_gather_check(sd_ctx *ctx, const sd_model *m, int dtype, const char *who, bool need_L = false) {
  if (!m->dev_ready) return sd_set_err(ctx, SD_EARG, "model has no device tables (created without a context)");
  if (dtype != SD_F64 && dtype != SD_C128) return sd_set_err(ctx, SD_EARG, "dtype must be SD_F64 or SD_C128");
  if (m->nranks != 1) return sd_set_err(ctx, SD_EARG, std::string(who) + " an unsharded model");
  if (need_L && (m->L < 1 || m->L > SD_MAX_L)) return sd_set_err(ctx, SD_EARG, std::string(who) + " 1 <= L <= 63");
  return SD_OK;
}

namespace sd_dev {

// ---- the rows of a workgroup ----
// blk of nblk: blockIdx.x of gridDim.x, or .y where the x axis counts chunks.  The row stride is the literal 256 of the launches.

// lbin[n * K + k] = C(n, k), n < L, k < K = nup + 1: the LDS copy of dm.binom for the rank walks of MODE 0, and its barrier
template <int MODE>
__device__ __forceinline__ void fill_lbin(const sd_dev_model &dm, int64_t *lbin, int K) {
  if (MODE == 0) {
    for (int k = threadIdx.x; k < dm.L * K; k += 256) lbin[k] = dm.binom[(k / K) * (SD_MAX_L + 1) + (k % K)];
    __syncthreads();
  }
}

// MODE 1, the outer loop: f(P, base, len, sufS) once per tile of this workgroup's share -- prefix configuration, first row, rows,
// and the suffix configurations of the rows in order
template <class F>
__device__ __forceinline__ void for_tiles(const sd_dev_model &dm, unsigned blk, unsigned nblk, F &&f) {
  for (int t = blk; t < dm.n_tiles; t += nblk) {
    const uint32_t P = dm.tile_prefix[t];
    const int64_t base = dm.tile_base[t];
    const int t2 = dm.nup - __popc(P);
    const int len = (int)binom_g(dm, dm.LS, t2);
    const uint16_t *__restrict__ sufS = dm.suf_states + dm.suf_off[t2];
    f(P, base, len, sufS);
  }
}

// row(s, idx) for every row of this workgroup's share: configuration and row
template <int MODE, class F>
__device__ __forceinline__ void for_rows(const sd_dev_model &dm, unsigned blk, unsigned nblk, F &&row) {
  if (MODE == 1) {
    for_tiles(dm, blk, nblk, [&](uint32_t P, int64_t base, int len, const uint16_t *__restrict__ sufS) {
      for (int i = threadIdx.x; i < len; i += 256) row((uint64_t)P | ((uint64_t)sufS[i] << dm.p), base + i);
    });
  } else {
    const int64_t stride = (int64_t)nblk * 256;
    for (int64_t idx = (int64_t)blk * 256 + threadIdx.x; idx < dm.n_local; idx += stride)
      row(MODE == 2 ? (uint64_t)idx : unrank_g(dm, idx), idx);
  }
}

// ---- partner rows ----
// Rows of one site pair bi < bj (0-based bits) whose two sites differ, and their partner rows s' = s with the two sites exchanged
// (kernels_pairs.hip, kernels_dimer.hip, kernels_ecurrent.hip).
// rank_shift: |idx(s) - idx(s')| in the combinadic order (MODE 0).  Moving one up spin from bj down to bi leaves r_k (the ups still
// to place at site k) as it is below bi and above bj and lowers it by one in between, so only the terms of sites bi..bj of rank_g's
// sum change:
//   d = C(L-1-bi, r-1) + sum_{bi<b<bj, b down} [C(L-1-b, r_b-1) - C(L-1-b, r_b-2)] - C(L-1-bj, r_bj-2),
// C(n, -1) = 0, r = nup - popcount(s below bi) >= 1.  The walk reads the sites below bi and strictly between bi and bj only, which
// s and s' share, so it serves both orientations: the row with bj up lies d rows AFTER the one with bi up.
// lbin: fill_lbin's copy.
__device__ __forceinline__ int64_t rank_shift(const sd_dev_model &dm, const int64_t *lbin, int K, uint64_t s, int bi, int bj) {
  int r = dm.nup - __popcll(s & (((uint64_t)1 << bi) - 1));
  int64_t d = lbin[(dm.L - 1 - bi) * K + r - 1];
  for (int b = bi + 1; b < bj; ++b) {
    if ((s >> b) & 1) { --r; continue; }
    const int64_t *row = lbin + (dm.L - 1 - b) * K;
    d += row[r - 1];
    if (r >= 2) d -= row[r - 2];
  }
  if (r >= 2) d -= lbin[(dm.L - 1 - bj) * K + r - 2];
  return d;
}
// MODES 1 and 2 are symmetric in the orientation: the plan's own rank of s' (two cached loads), or idx ^ mask.
template <int MODE>
__device__ __forceinline__ int64_t partner_sym(const sd_dev_model &dm, uint64_t s, int64_t idx, uint64_t mask) {
  if (MODE == 2) return idx ^ (int64_t)mask;
  const uint64_t t = s ^ mask;
  return dm.addr[(uint32_t)t & (((uint32_t)1 << dm.p) - 1u)] + (int64_t)dm.suf_rank[t >> dm.p];
}
// site bj up and site bi down in s
template <int MODE>
__device__ __forceinline__ int64_t pair_partner(const sd_dev_model &dm, const int64_t *lbin, int K, uint64_t s, int64_t idx, int bi,
                                                int bj) {
  if (MODE != 0) return partner_sym<MODE>(dm, s, idx, ((uint64_t)1 << bi) | ((uint64_t)1 << bj));
  return idx - rank_shift(dm, lbin, K, s, bi, bj);
}
// either orientation: the two sites differ in s
template <int MODE>
__device__ __forceinline__ int64_t bond_partner(const sd_dev_model &dm, const int64_t *lbin, int K, uint64_t s, int64_t idx, int bi,
                                                int bj) {
  if (MODE != 0) return partner_sym<MODE>(dm, s, idx, ((uint64_t)1 << bi) | ((uint64_t)1 << bj));
  const int64_t d = rank_shift(dm, lbin, K, s, bi, bj);
  return ((s >> bj) & 1) ? idx - d : idx + d;
}

// Row of an arbitrary configuration t of the basis (kernels_opstring.hip, kernels_symmetry.hip, kernels_permute.hip): MODE 2 the
// configuration itself; 1 the plan's own rank addr[prefix of t] + suf_rank[suffix of t], two cached loads; 0 the combinadic rank
// walked over fill_lbin's copy of the binomials.  t must have nup bits set below bit L (MODES 0 and 1).
template <int MODE>
__device__ __forceinline__ int64_t config_row(const sd_dev_model &dm, const int64_t *lbin, int K, uint64_t t) {
  if (MODE == 2) return (int64_t)t;
  if (MODE == 1) return dm.addr[(uint32_t)t & (((uint32_t)1 << dm.p) - 1u)] + (int64_t)dm.suf_rank[t >> dm.p];
  int64_t idx = 0;
  int r = dm.nup;
  for (int b = 0; b < dm.L && r > 0; ++b) {
    if ((t >> b) & 1) --r;
    else idx += lbin[(dm.L - 1 - b) * K + r - 1];
  }
  return idx;
}

// ---- the reduction of chunked partial rows ----
// The kernels whose grid is (chunk of CHUNK list entries, row block) leave one partial row of 2 CHUNK doubles per block, (re, im) per
// entry, chunk after chunk.  Block c sums the partial rows of chunk c in a fixed order (256 / (2 CHUNK) strided sums per column,
// then their sum) and files out[2 e .. +1] = scale * sum for the entries e < n of the chunk.  scale == 1.0 changes no bits.
template <int CHUNK>
__global__ __launch_bounds__(256) void k_chunk_reduce(const double *__restrict__ partials, int nblocks, int n, double scale,
                                                      double *__restrict__ out) {
  constexpr int ROW = 2 * CHUNK, GROUPS = 256 / ROW;
  static_assert(GROUPS * ROW == 256, "a block is a whole number of partial rows");
  __shared__ double sm[GROUPS][ROW];
  const int c = threadIdx.x % ROW, j = threadIdx.x / ROW;
  const double *__restrict__ p = partials + (size_t)blockIdx.x * nblocks * ROW;
  double a = 0.0;
  for (int b = j; b < nblocks; b += GROUPS) a += p[(size_t)b * ROW + c];
  sm[j][c] = a;
  __syncthreads();
  if (threadIdx.x < ROW) {
    double t = 0.0;
    for (int jj = 0; jj < GROUPS; ++jj) t += sm[jj][c];
    const int e = blockIdx.x * CHUNK + (c >> 1);
    if (e < n) out[2 * (size_t)e + (c & 1)] = scale * t;
  }
}

}  // namespace sd_dev
