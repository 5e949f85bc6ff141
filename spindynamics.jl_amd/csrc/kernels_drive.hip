// Diagonal drives.  D = sum_i W_i S^z_i + sum_b V_b S^z_{i_b} S^z_{j_b} is diagonal in the S^z basis, so the step of a
// recursion on H0 + D is the step on H0 with d(s_r) psi[r] added to (H0 psi)[r] before the recursion's epilogue:
//     acc = h[r] + d(s_r) * psi[r],   epilogue<NC>(epi, ea, r, acc, psi[r], out, sums)
// -- one elementwise pass of three streams (h, psi, out; out may be h), the weights in kernel arguments (uniform: scalar loads), the
// configuration of a row from the plan's tables.
// d(s), -ffp-contract=off, the selection idea of diag_of's list-order form: a sequential sum from 0.0 of the site terms i = 0..L-1, each
// +W_i/2 (site up) or -W_i/2, then of the bond terms in list order, each +V_b/4 (parallel) or -V_b/4.  The table holds the halves and
// quarters, which are exact, so every term is selected, not multiplied.  Without site weights the site loop is skipped.
// Row configurations (MODE) of gather_common.hpp: 1 the tile's prefix and the suffix table of a tiled sector plan (for_tiles), 0
// unrank_g of the row, 2 the row index (full basis).  MODE 1 splits the sum as diag_head / diag_tail do: its leading terms depend on
// the prefix alone -- the site terms of sites 0..p-1, or (no site weights) the leading bonds that lie inside the prefix -- and are
// formed once per tile; every row continues the same sequential sum, so the bits are those of the undivided loop.
// Sums: per thread, block_reduce2, one pair per block in ctx->d_partials, sd_reduce_pairs -- as k_epilogue_only.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "drive_terms.hpp"   // d(s): drive_sites, drive_bonds
#include "gather_common.hpp"

using namespace sd_dev;

namespace {

#define SD_DRIVE_TILE_BLOCKS 4096        // tiled plans: workgroups, one tile at a time each
#define SD_DRIVE_ROW_BLOCKS 8192         // blocks of 256 rows (per-row plans, full basis)

// head_bonds: the leading bonds of the table with both sites below p (MODE 1 without site weights; the launcher counts them)
template <int NC, int MODE>
__global__ __launch_bounds__(256) void k_drive_epilogue(sd_dev_model dm, sd_drive_table tb, int head_bonds, int epi, sd_epi_args ea,
                                                        double *out_, const double *h_, const double *__restrict__ psi_,
                                                        double *__restrict__ partials) {
  using V = typename VT<NC>::type;
  __shared__ double red[32];
  const V *h = reinterpret_cast<const V *>(h_);              // may be out_, or null: h = 0
  const V *__restrict__ psi = reinterpret_cast<const V *>(psi_);
  EpiSums sums{0.0, 0.0};
  auto row = [&](int64_t r, double d) {
    const V own = psi[r];
    V acc;
    if (h) acc = h[r];
    else if constexpr (NC == 2) acc = make_double2(0.0, 0.0);
    else acc = 0.0;
    acc = vadd_mul(acc, d, own);
    epilogue<NC>(epi, ea, r, acc, own, out_, sums);
  };
  if (MODE == 1) {
    for_tiles(dm, blockIdx.x, gridDim.x, [&](uint32_t P, int64_t base, int len, const uint16_t *__restrict__ sufS) {
      const double d0 = tb.has_sites ? drive_sites(tb, (uint64_t)P, 0, dm.p, 0.0) : drive_bonds(tb, (uint64_t)P, 0, head_bonds, 0.0);
      for (int i = threadIdx.x; i < len; i += 256) {
        const uint64_t s = (uint64_t)P | ((uint64_t)sufS[i] << dm.p);
        double d = d0;
        if (tb.has_sites) d = drive_bonds(tb, s, 0, tb.n_bonds, drive_sites(tb, s, dm.p, dm.L, d));
        else d = drive_bonds(tb, s, head_bonds, tb.n_bonds, d);
        row(base + i, d);
      }
    });
  } else {
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < dm.n_local; idx += stride) {
      const uint64_t s = MODE == 2 ? (uint64_t)idx : unrank_g(dm, idx);
      double d = 0.0;
      if (tb.has_sites) d = drive_sites(tb, s, 0, dm.L, d);
      row(idx, drive_bonds(tb, s, 0, tb.n_bonds, d));
    }
  }
  if (epi_has_sums(epi)) {
    double a = sums.s0, b = sums.s1;
    block_reduce2(a, b, red);
    if (threadIdx.x == 0) { partials[2 * (size_t)blockIdx.x] = a; partials[2 * (size_t)blockIdx.x + 1] = b; }
  }
}

template <int NC>
void launch_drive(int mode, unsigned nb, hipStream_t st, const sd_dev_model &dm, const sd_drive_table &tb, int head_bonds, int epi,
                  const sd_epi_args &ea, double *out, const double *h, const double *psi, double *partials) {
  const dim3 grid(nb), blk(256);
  sd_with_mode(mode, [&](auto M) {
    hipLaunchKernelGGL((k_drive_epilogue<NC, decltype(M)::value>), grid, blk, 0, st, dm, tb, head_bonds, epi, ea, out, h, psi, partials);
  });
}

}  // namespace

// The caller has built the table with sd_drive_build (sites below L, at most SD_DRIVE_MAX_BONDS bonds).
int sd_launch_drive_epilogue(sd_ctx *ctx, const sd_model *m, int dtype, void *out, const void *h, const void *psi, int epi,
                             const sd_epi_args &ea_in, const sd_drive_table &table) {
  if (!m || !m->dev_ready) return sd_set_err(ctx, SD_EARG, "model has no device tables");
  if (m->nranks != 1) return sd_set_err(ctx, SD_EARG, "diagonal drives need an unsharded model");
  if (dtype != SD_F64 && dtype != SD_C128) return sd_set_err(ctx, SD_EARG, "dtype must be SD_F64 or SD_C128");
  if (m->L < 1 || m->L > SD_MAX_L || table.n_bonds < 0 || table.n_bonds > SD_DRIVE_MAX_BONDS)
    return sd_set_err(ctx, SD_EINTERNAL, "bad drive table");
  const sd_dev_model &dm = m->dm;
  const bool sums = (epi == SD_EPI_DOT || epi == SD_EPI_KPM || epi == SD_EPI_RESCALE_DOT);
  sd_epi_args ea = ea_in;
  ea.stream_hint = 0;
  if (dm.n_local <= 0) {
    if (sums) SD_HIP(ctx, hipMemsetAsync(ea.sums_dst ? ea.sums_dst : ctx->d_scalars, 0, 2 * sizeof(double), ctx->stream));
    return SD_OK;
  }
  const sd_gather_grid g = sd_gather_grid_of(m, SD_DRIVE_TILE_BLOCKS, SD_DRIVE_ROW_BLOCKS);
  const int mode = g.mode;
  const int64_t nb = g.nb;
  int head_bonds = 0;
  if (mode == 1 && !table.has_sites)
    while (head_bonds < table.n_bonds && (table.bits[head_bonds] & 255) < dm.p && (table.bits[head_bonds] >> 8) < dm.p) ++head_bonds;
  if (sums) { int rc = sd_ensure_partials(ctx, 2 * (size_t)nb + 2 * SD_RED_STAGE_BLOCKS); if (rc) return rc; }
  if (dtype == SD_C128)
    launch_drive<2>(mode, (unsigned)nb, ctx->stream, dm, table, head_bonds, epi, ea, (double *)out, (const double *)h, (const double *)psi,
                    ctx->d_partials);
  else
    launch_drive<1>(mode, (unsigned)nb, ctx->stream, dm, table, head_bonds, epi, ea, (double *)out, (const double *)h, (const double *)psi,
                    ctx->d_partials);
  SD_HIP(ctx, hipGetLastError());
  if (sums) return sd_reduce_pairs(ctx, nb, ea.sums_dst);
  return SD_OK;
}
