// Hopping drives.  B = sum_b (z_b S^+_{i_b} S^-_{j_b} + conj(z_b) S^-_{i_b} S^+_{j_b}), z_b = x_b + i y_b, is Hermitian and
// keeps nup, so the step of a recursion on H0 + D + B is the step on H0 with d(s_r) psi[r] and (B psi)[r] added to (H0 psi)[r] before the
// recursion's epilogue:
//     acc = h[r];  acc += d(s_r) * psi[r]  (a stage with a diagonal table, as kernels_drive.hip);
//     for every bond b in list order whose two sites differ in s_r, v = psi[partner row]:
//       real form    : acc.c += x_b * v.c per component
//       complex form : y' = +y_b when site i_b is up in s_r, -y_b when site j_b is (selected, not multiplied),
//                      t = (x_b v.re - y' v.im, x_b v.im + y' v.re), acc += t
//     epilogue<NC>(epi, ea, r, acc, psi[r], out, sums)
// -- one pass of three streams (h, psi, out; out may be h) plus the gathers of psi, -ffp-contract=off.  psi must alias neither h nor out:
// other rows' gathers read it while this row's out is written.
// The hop table is in device memory (site words lo | hi << 8 | (i is the higher bit) << 16, and the (x, y) pairs), read with the loop
// index: uniform loads.  The diagonal table rides in the kernel arguments as in kernels_drive.hip; no per-tile head here -- the
// undivided sum has the same bits.
// Rows and configurations (MODE) by for_rows, partner rows by bond_partner (gather_common.hpp): 1 the plan's own rank of the flipped
// configuration, 0 the rank walk over the LDS binomials, 2 idx ^ mask.
// Sums: per thread, block_reduce2, one pair per block in ctx->d_partials, sd_reduce_pairs -- as k_drive_epilogue.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "drive_terms.hpp"
#include "gather_common.hpp"

using namespace sd_dev;

namespace {

#define SD_HOP_TILE_BLOCKS 4096          // tiled plans: workgroups, one tile at a time each
#define SD_HOP_ROW_BLOCKS 8192           // blocks of 256 rows (per-row plans, full basis)

struct hop_args {                        // the table of one stage on the device
  int n;
  int has_diag;
  const uint32_t *bits;
  const double2 *xy;
};

// everything the kernel takes by value must fit the 4 KiB of kernel arguments
static_assert(sizeof(sd_dev_model) + sizeof(sd_drive_table) + sizeof(hop_args) + sizeof(sd_epi_args) + 2 * sizeof(int) +
                      4 * sizeof(void *) <= 4096, "kernel arguments of k_hop_drive_epilogue exceed 4 KiB");

template <int NC, int MODE, bool CPLX>
__global__ __launch_bounds__(256) void k_hop_drive_epilogue(sd_dev_model dm, sd_drive_table tb, hop_args hp, int epi, sd_epi_args ea,
                                                            double *out_, const double *h_, const double *__restrict__ psi_,
                                                            double *__restrict__ partials) {
  static_assert(!CPLX || NC == 2, "the complex form needs a ComplexF64 vector");
  using V = typename VT<NC>::type;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  double *red = reinterpret_cast<double *>(smem);            // 32 doubles
  int64_t *lbin = reinterpret_cast<int64_t *>(red + 32);     // MODE 0: lbin[n * K + k] = C(n, k)
  const int K = (dm.nup > 0 ? dm.nup : 0) + 1;
  fill_lbin<MODE>(dm, lbin, K);
  const V *h = reinterpret_cast<const V *>(h_);              // may be out_, or null: h = 0
  const V *__restrict__ psi = reinterpret_cast<const V *>(psi_);
  EpiSums sums{0.0, 0.0};
  for_rows<MODE>(dm, blockIdx.x, gridDim.x, [&](uint64_t s, int64_t r) {
    const V own = psi[r];
    V acc;
    if (h) acc = h[r];
    else if constexpr (NC == 2) acc = make_double2(0.0, 0.0);
    else acc = 0.0;
    if (hp.has_diag) {
      double d = 0.0;
      if (tb.has_sites) d = drive_sites(tb, s, 0, dm.L, d);
      acc = vadd_mul(acc, drive_bonds(tb, s, 0, tb.n_bonds, d), own);
    }
    for (int b = 0; b < hp.n; ++b) {
      const uint32_t w = hp.bits[b];
      const int lo = (int)(w & 255u), hi = (int)((w >> 8) & 255u);
      const uint64_t ulo = (s >> lo) & 1, uhi = (s >> hi) & 1;
      if (ulo == uhi) continue;
      const int64_t partner = bond_partner<MODE>(dm, lbin, K, s, r, lo, hi);
      const double2 xy = hp.xy[b];
      const V v = psi[partner];
      if constexpr (NC == 1) {
        acc = acc + xy.x * v;
      } else if constexpr (!CPLX) {
        acc = make_double2(acc.x + xy.x * v.x, acc.y + xy.x * v.y);
      } else {
        const bool i_up = ((w >> 16) & 1u) ? uhi : ulo;      // site i_b is up in s
        const double yp = i_up ? xy.y : -xy.y;
        const double tr = xy.x * v.x - yp * v.y, ti = xy.x * v.y + yp * v.x;
        acc = make_double2(acc.x + tr, acc.y + ti);
      }
    }
    epilogue<NC>(epi, ea, r, acc, own, out_, sums);
  });
  if (epi_has_sums(epi)) {
    double a = sums.s0, b = sums.s1;
    block_reduce2(a, b, red);
    if (threadIdx.x == 0) { partials[2 * (size_t)blockIdx.x] = a; partials[2 * (size_t)blockIdx.x + 1] = b; }
  }
}

template <int NC, bool CPLX>
void launch_hop(int mode, unsigned nb, size_t shmem, hipStream_t st, const sd_dev_model &dm, const sd_drive_table &tb, const hop_args &hp,
                int epi, const sd_epi_args &ea, double *out, const double *h, const double *psi, double *partials) {
  sd_with_mode(mode, [&](auto M) {
    hipLaunchKernelGGL((k_hop_drive_epilogue<NC, decltype(M)::value, CPLX>), dim3(nb), dim3(256), shmem, st, dm, tb, hp, epi, ea, out, h,
                       psi, partials);
  });
}

}  // namespace

// The caller has built the lists with sd_drive_build / sd_hop_build (sites below L, at most SD_HOP_MAX_BONDS terms).
int sd_launch_hop_drive_epilogue(sd_ctx *ctx, const sd_model *m, int dtype, void *out, const void *h, const void *psi, int epi,
                                 const sd_epi_args &ea_in, const sd_drive_table *diag, int n_hop, int complex_form,
                                 const uint32_t *bits_dev, const double *xy_dev) {
  if (!m) return sd_set_err(ctx, SD_EARG, "model has no device tables");
  if (int rc = sd_gather_check(ctx, m, dtype, "hopping drives need", true)) return rc;
  if (n_hop < 0 || n_hop > SD_HOP_MAX_BONDS || (n_hop > 0 && (!bits_dev || !xy_dev)) ||
      (diag && (diag->n_bonds < 0 || diag->n_bonds > SD_DRIVE_MAX_BONDS)))
    return sd_set_err(ctx, SD_EINTERNAL, "bad hop table");
  if (complex_form && dtype != SD_C128) return sd_set_err(ctx, SD_EARG, "a hopping drive with complex weights needs a ComplexF64 vector");
  const sd_dev_model &dm = m->dm;
  const bool sums = (epi == SD_EPI_DOT || epi == SD_EPI_KPM || epi == SD_EPI_RESCALE_DOT);
  sd_epi_args ea = ea_in;
  ea.stream_hint = 0;
  if (dm.n_local <= 0) {
    if (sums) SD_HIP(ctx, hipMemsetAsync(ea.sums_dst ? ea.sums_dst : ctx->d_scalars, 0, 2 * sizeof(double), ctx->stream));
    return SD_OK;
  }
  const sd_gather_grid g = sd_gather_grid_of(m, SD_HOP_TILE_BLOCKS, SD_HOP_ROW_BLOCKS);
  const unsigned nb = std::max(g.nb, 1u);
  const size_t shmem = 32 * sizeof(double) + g.lbin_bytes;
  if (sums) { int rc = sd_ensure_partials(ctx, 2 * (size_t)nb + 2 * SD_RED_STAGE_BLOCKS); if (rc) return rc; }
  static const sd_drive_table no_diag{};
  hop_args hp;
  hp.n = n_hop;
  hp.has_diag = diag ? 1 : 0;
  hp.bits = bits_dev;
  hp.xy = reinterpret_cast<const double2 *>(xy_dev);
  const sd_drive_table &tb = diag ? *diag : no_diag;
  double *o = (double *)out;
  const double *hh = (const double *)h, *p = (const double *)psi;
  if (dtype == SD_F64) launch_hop<1, false>(g.mode, nb, shmem, ctx->stream, dm, tb, hp, epi, ea, o, hh, p, ctx->d_partials);
  else if (!complex_form) launch_hop<2, false>(g.mode, nb, shmem, ctx->stream, dm, tb, hp, epi, ea, o, hh, p, ctx->d_partials);
  else launch_hop<2, true>(g.mode, nb, shmem, ctx->stream, dm, tb, hp, epi, ea, o, hh, p, ctx->d_partials);
  SD_HIP(ctx, hipGetLastError());
  if (sums) return sd_reduce_pairs(ctx, (int64_t)nb, ea.sums_dst);
  return SD_OK;
}
