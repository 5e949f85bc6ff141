// Spin current of the hop list.  With hops (i_b, j_b, t_b) the bond current is
//     j_b = i t_b (S^+_{i_b} S^-_{j_b} - S^-_{i_b} S^+_{j_b}),        J_w = sum_b w_b j_b   (real weights w),
// Hermitian, carrying S^z from site i_b to site j_b.  Row form, one owner thread per row s:
//     (J_w psi)[s] = i * sum_{b : s_{i_b} != s_{j_b}} (w_b t_b sigma_b(s)) * psi[flip_b(s)],
//     sigma_b(s) = +1 when site i_b is up in s, -1 when site j_b is,
// summed in hop-list order from a zero accumulator, each term the product (w_b t_b sigma_b) * psi[partner]; the factor i is
// the exact swap (re, im) -> (-im, re) at the end.  J_w keeps nup; in the full basis the partner is s ^ mask.
//
// One kernel template in two forms:
//   write   : out[s] = (J_w psi)[s]                      (psi Float64 or ComplexF64, out ComplexF64)
//   bracket : sum_s conj(bra[s]) (J_w ket)[s]            (bra Float64 or ComplexF64, ket ComplexF64) WITHOUT writing J_w ket --
//             the per-time-point measurement of the typicality driver: two read streams plus the gathers.  Per-thread sums,
//             a fixed-order block reduction, then sd_reduce_pairs over the blocks: no atomics, the same call gives the same bits.
// Rows and their configurations (MODE) by for_rows (gather_common.hpp): 1 the tile's prefix and the suffix table of a tiled sector
// plan, 0 unrank_g of the row (sector plans without tiles), 2 the row index itself (full basis).  Partner rows in a
// sector: the leading chain bonds (b, b+1) by the closed form of the combinadic order,
//     idx +- C(L - b - 1, u),   u = ups among the sites above b + 1,   + when site b is the up one,
// with the binomials in LDS; every other bond by the rank walk, as k_apply_short / k_apply_generic do.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "gather_common.hpp"

using namespace sd_dev;

namespace {

// sum_b (wt_b sigma_b) * ket[partner_b] for row idx with configuration s; wt_b = w_b t_b.  NCK = 1: .y stays 0.
template <int NCK, int MODE>
__device__ __forceinline__ double2 current_row(const sd_dev_model &dm, const double *__restrict__ ket, const double *__restrict__ wt,
                                               const int64_t *lbin, int K, uint64_t s, int64_t idx) {
  double ar = 0.0, ai = 0.0;
  for (int b = 0; b < dm.n_hop; ++b) {
    const bool chain = b < dm.nn_hops;                       // hop b is the chain bond of sites (b + 1, b + 2): bits b, b + 1
    const int bi = chain ? b : dm.hop_i[b] - 1, bj = chain ? b + 1 : dm.hop_j[b] - 1;
    const bool ui = (s >> bi) & 1, uj = (s >> bj) & 1;
    if (ui == uj) continue;
    int64_t partner;
    if (MODE == 2) {
      partner = idx ^ (int64_t)(((uint64_t)1 << bi) | ((uint64_t)1 << bj));
    } else if (chain) {
      const int64_t c = lbin[(dm.L - b - 2) * K + __popcll(s >> (b + 2))];
      partner = ui ? idx + c : idx - c;
    } else {
      partner = rank_g(dm, s ^ (((uint64_t)1 << bi) | ((uint64_t)1 << bj)));
    }
    const double c = ui ? wt[b] : -wt[b];
    if (NCK == 2) {
      const double2 v = ((const double2 *)ket)[partner];
      ar += c * v.x;
      ai += c * v.y;
    } else {
      ar += c * ket[partner];
    }
  }
  return make_double2(ar, ai);
}

// NC: components of psi (write form) or of bra (bracket form; the ket is ComplexF64)
template <int NC, bool BRACKET, int MODE>
__global__ __launch_bounds__(256) void k_current(sd_dev_model dm, const double *__restrict__ vec, const double *__restrict__ bra,
                                                 const double *__restrict__ wt, double2 *__restrict__ out,
                                                 double *__restrict__ partials) {
  constexpr int NCK = BRACKET ? 2 : NC;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  double *red = reinterpret_cast<double *>(smem);            // 32 doubles
  int64_t *lbin = reinterpret_cast<int64_t *>(red + 32);     // lbin[n * K + k] = C(n, k), n < L, k <= nup (sector plans with chain bonds)
  const int K = (dm.nup > 0 ? dm.nup : 0) + 1;
  if (MODE != 2 && dm.nn_hops > 0) fill_lbin<0>(dm, lbin, K);   // the chain bonds' closed form reads it in MODE 1 too
  double sr = 0.0, si = 0.0;
  auto row = [&](uint64_t s, int64_t idx) {
    const double2 a = current_row<NCK, MODE>(dm, vec, wt, lbin, K, s, idx);
    const double2 j = make_double2(-a.y, a.x);               // i * a
    if (!BRACKET) {
      out[idx] = j;
    } else if (NC == 2) {
      const double2 bv = ((const double2 *)bra)[idx];
      sr += bv.x * j.x + bv.y * j.y;                         // conj(bra) * j
      si += bv.x * j.y - bv.y * j.x;
    } else {
      const double bv = bra[idx];
      sr += bv * j.x;
      si += bv * j.y;
    }
  };
  for_rows<MODE>(dm, blockIdx.x, gridDim.x, row);
  if (BRACKET) {
    block_reduce2(sr, si, red);
    if (threadIdx.x == 0) { partials[2 * (size_t)blockIdx.x] = sr; partials[2 * (size_t)blockIdx.x + 1] = si; }
  }
}

#define SD_CURRENT_TILE_BLOCKS 4096      // tiled plans: workgroups, one tile at a time each
#define SD_CURRENT_ROW_BLOCKS 8192       // blocks of 256 rows (per-row plans, full basis)

template <int NC, bool BRACKET>
void launch_mode(int mode, unsigned nb, size_t shmem, hipStream_t st, const sd_dev_model &dm, const double *vec, const double *bra,
                 const double *wt, double2 *out, double *partials) {
  sd_with_mode(mode, [&](auto M) {
    hipLaunchKernelGGL((k_current<NC, BRACKET, decltype(M)::value>), dim3(nb), dim3(256), shmem, st, dm, vec, bra, wt, out, partials);
  });
}

}  // namespace

// Write form (out != null): out = J_w vec, vec of `dtype`, out ComplexF64, must not alias vec.  Bracket form (out == null):
// dst[0..1] (device) = <bra|J_w|vec>, bra of `dtype`, vec ComplexF64.  wt_dev: the n_hop products w_b t_b on the device.
// Queued on the context's stream.
int sd_launch_current(sd_ctx *ctx, const sd_model *m, int dtype, const void *vec, const void *bra, const double *wt_dev, void *out,
                      double *dst) {
  if (int rc = sd_gather_check(ctx, m, dtype, "the spin current needs")) return rc;
  const sd_dev_model &dm = m->dm;
  const bool bracket = out == nullptr;
  if (dm.n_local == 0) {      // no rows: the bracket is zero
    if (bracket) SD_HIP(ctx, hipMemsetAsync(dst, 0, 2 * sizeof(double), ctx->stream));
    return SD_OK;
  }
  const sd_gather_grid g = sd_gather_grid_of(m, SD_CURRENT_TILE_BLOCKS, SD_CURRENT_ROW_BLOCKS);
  const int mode = g.mode;
  const unsigned nb = std::max(g.nb, 1u);
  // not g.lbin_bytes: the chain bonds read the binomials in MODE 1 as well, and the region is sized in every mode
  const size_t shmem = 32 * sizeof(double) + (size_t)dm.L * (size_t)((dm.nup > 0 ? dm.nup : 0) + 1) * sizeof(int64_t);
  if (bracket) { int rc = sd_ensure_partials(ctx, 2 * (size_t)nb + 2 * SD_RED_STAGE_BLOCKS); if (rc) return rc; }
  const double *v = (const double *)vec, *b = (const double *)bra;
  double2 *o = (double2 *)out;
  const bool c = dtype == SD_C128;
  if (bracket) {
    if (c) launch_mode<2, true>(mode, nb, shmem, ctx->stream, dm, v, b, wt_dev, o, ctx->d_partials);
    else launch_mode<1, true>(mode, nb, shmem, ctx->stream, dm, v, b, wt_dev, o, ctx->d_partials);
  } else {
    if (c) launch_mode<2, false>(mode, nb, shmem, ctx->stream, dm, v, b, wt_dev, o, ctx->d_partials);
    else launch_mode<1, false>(mode, nb, shmem, ctx->stream, dm, v, b, wt_dev, o, ctx->d_partials);
  }
  SD_HIP(ctx, hipGetLastError());
  if (bracket) return sd_reduce_pairs(ctx, (int64_t)nb, dst);
  return SD_OK;
}
