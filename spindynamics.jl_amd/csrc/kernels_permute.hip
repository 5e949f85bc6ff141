// Site permutations.  pi moves the spin of site i + 1 to site perm[i]; U_pi |s> = |pi s>, so
//     (U_pi psi)[idx(s)] = psi[idx(src(s))],   bit i of src(s) = bit (perm[i] - 1) of s            (site_perm.hpp)
// -- a permutation gather that copies bits, like the plain form of k_sym_apply, for a map that is no rotation or reversal: src(s) is
// the OR of one table read per byte of s.  Every workgroup builds its tables in LDS from the permutation, passed by value, with the
// code that builds them on the host (sd_site_perm_fill).
// Row configurations (MODE) of gather_common.hpp: 1 the tile's prefix and the suffix table of a tiled sector plan (for_tiles, with the
// prefix's share of the source formed once per tile), 0 unrank_g of the row, 2 the row index (full basis).  MODE 1 splits the tables
// where the plan splits the configuration: ceil(p / 8) tables over the prefix bits, read once per tile, and ceil(LS / 8) <= 2 over the
// suffix bits, read per row.  MODES 0 and 2: ceil(L / 8) tables over the whole configuration.  At most 8 tables, 16 KiB.  The source
// row is config_row<MODE> (same header): MODE 0 keeps the binomials in LDS behind the tables.
// Stores follow the output order (coalesced, 16 bytes per lane for ComplexF64); the loads are the gather.  When pi leaves the suffix
// sites in place, the source rows of a tile are one contiguous run of another tile and the loads coalesce too.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "gather_common.hpp"
#include "site_perm.hpp"

using namespace sd_dev;

namespace {

#define SD_PERM_TILE_BLOCKS 4096         // tiled plans: workgroups, as SD_SYM_TILE_BLOCKS
#define SD_PERM_ROW_BLOCKS 8192          // blocks of 256 rows (per-row plans, full basis), as SD_SYM_ROW_BLOCKS

template <int NC, int MODE>
__global__ __launch_bounds__(256) void k_site_permute(sd_dev_model dm, sd_site_perm pm, const double *__restrict__ x,
                                                      double *__restrict__ out) {
  using V = typename VT<NC>::type;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  uint64_t *lut = reinterpret_cast<uint64_t *>(smem);
  const int n_lo = MODE == 1 ? (dm.p + 7) >> 3 : (dm.L + 7) >> 3;      // tables from bit 0 up
  const int n_hi = MODE == 1 ? (dm.LS + 7) >> 3 : 0;                   // tables from bit p up (the suffix)
  const uint64_t *lut_hi = lut + 256 * n_lo;
  int64_t *lbin = reinterpret_cast<int64_t *>(lut + 256 * (n_lo + n_hi));
  const int K = (dm.nup > 0 ? dm.nup : 0) + 1;
  sd_site_perm_fill(lut, pm, dm.L, 0, n_lo, threadIdx.x, 256);
  if (MODE == 1) sd_site_perm_fill(lut + 256 * n_lo, pm, dm.L, dm.p, n_hi, threadIdx.x, 256);
  fill_lbin<MODE>(dm, lbin, K);
  if (MODE != 0) __syncthreads();                                      // MODE 0: fill_lbin's barrier covers the tables too
  const V *__restrict__ xv = reinterpret_cast<const V *>(x);
  V *__restrict__ ov = reinterpret_cast<V *>(out);
  if (MODE == 1) {
    for_tiles(dm, blockIdx.x, gridDim.x, [&](uint32_t P, int64_t base, int len, const uint16_t *__restrict__ sufS) {
      const uint64_t srcP = sd_site_perm_source(lut, n_lo, (uint64_t)P);   // once per tile
      for (int i = threadIdx.x; i < len; i += 256) {
        const uint64_t src = srcP | sd_site_perm_source(lut_hi, n_hi, (uint64_t)sufS[i]);
        ov[base + i] = xv[config_row<1>(dm, lbin, K, src)];
      }
    });
  } else {
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < dm.n_local; idx += stride) {
      const uint64_t s = MODE == 2 ? (uint64_t)idx : unrank_g(dm, idx);
      ov[idx] = xv[config_row<MODE>(dm, lbin, K, sd_site_perm_source(lut, n_lo, s))];
    }
  }
}

template <int NC>
void launch_permute(int mode, unsigned nb, size_t shmem, hipStream_t st, const sd_dev_model &dm, const sd_site_perm &pm, const double *x,
                    double *out) {
  const dim3 grid(nb), blk(256);
  sd_with_mode(mode, [&](auto M) { hipLaunchKernelGGL((k_site_permute<NC, decltype(M)::value>), grid, blk, shmem, st, dm, pm, x, out); });
}

}  // namespace

// The caller (capi.cpp) has validated the permutation (a bijection of 1..L), the model (device tables, unsharded) and the dtype.
int sd_launch_site_permute(sd_ctx *ctx, const sd_model *m, int dtype, const sd_site_perm &pm, const void *x, void *out) {
  const sd_dev_model &dm = m->dm;
  if (m->L < 1 || m->L > SD_MAX_L) return sd_set_err(ctx, SD_EARG, "site permutations need 1 <= L <= 63");
  if (dm.n_local == 0) return SD_OK;
  const sd_gather_grid g = sd_gather_grid_of(m, SD_PERM_TILE_BLOCKS, SD_PERM_ROW_BLOCKS);
  const int mode = g.mode;
  const int ntab = mode == 1 ? ((dm.p + 7) >> 3) + ((dm.LS + 7) >> 3) : (dm.L + 7) >> 3;
  if (ntab > SD_PERM_MAX_TABLES) return sd_set_err(ctx, SD_EINTERNAL, "site permutation: more than 8 tables");
  const size_t shmem = (size_t)ntab * 256 * sizeof(uint64_t) + g.lbin_bytes;
  if (dtype == SD_C128) launch_permute<2>(mode, g.nb, shmem, ctx->stream, dm, pm, (const double *)x, (double *)out);
  else launch_permute<1>(mode, g.nb, shmem, ctx->stream, dm, pm, (const double *)x, (double *)out);
  SD_HIP(ctx, hipGetLastError());
  return SD_OK;
}
