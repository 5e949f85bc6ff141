// Lists of dressed bond currents, the form of the energy current.  With j'_ij = i (S^+_i S^-_j - S^-_i S^+_j) a
// term (i, j, k, c) stands for c S^z_k j'_ij (k = 0: no S^z factor), consecutive terms of one ordered (i, j) form a group, and
//     (J psi)[s] = i * sum_groups [s_i != s_j] (sigma co) * psi[s with the sites i, j exchanged],
//     co = sum over the group's terms, in list order from 0.0, of (k == 0 ? c : site k up in s ? 0.5 c : -0.5 c),
//     sigma = +1 when site i is up in s, -1 when site j is,
// real and imaginary parts summed separately in group order from zero, the factor i the exact swap (re, im) -> (-im, re) at the
// end.  One gather per group, however many terms it has.  The host hands over 0.5 c (exact) for the dressed terms.
//
// One kernel template in two forms, as k_current:
//   write   : out[s] = (J psi)[s]                  (psi Float64 or ComplexF64, out ComplexF64)
//   bracket : sum_s conj(bra[s]) (J ket)[s]        (bra Float64 or ComplexF64, ket ComplexF64) without writing J ket.  Per-thread sums,
//             block_reduce2, then sd_reduce_pairs over the blocks: no atomics, the grid depends on the plan alone.
// Rows and their configurations (MODE) by for_rows (gather_common.hpp): 1 tile prefix and suffix table, 0 unrank_g of the row, 2 the
// row index.  Partner rows by bond_partner (same header): the plan's tables, the local rank walk with the binomials in LDS, or
// idx ^ mask.
// The group and term tables are read from global memory with wave-uniform indices (scalar loads), as k_current reads its hop list.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "gather_common.hpp"

using namespace sd_dev;

namespace {

// sum_groups (sigma co) * ket[partner] for row idx with configuration s.  NCK = 1: .y stays 0.
template <int NCK, int MODE>
__device__ __forceinline__ double2 dcurrent_row(const sd_dev_model &dm, const double *__restrict__ ket,
                                                const sd_dgroup *__restrict__ groups, int n_groups,
                                                const sd_dterm_dev *__restrict__ terms, const int64_t *lbin, int K, uint64_t s,
                                                int64_t idx) {
  double ar = 0.0, ai = 0.0;
  for (int g = 0; g < n_groups; ++g) {
    const sd_dgroup G = groups[g];
    const int lo = G.bits & 255, hi = (G.bits >> 8) & 255;      // 0-based bits, lo < hi
    const bool ulo = (s >> lo) & 1, uhi = (s >> hi) & 1;
    if (ulo == uhi) continue;
    double co = 0.0;
    for (int t = G.first; t < G.first + G.count; ++t) {
      const sd_dterm_dev T = terms[t];
      co += T.kb < 0 ? T.ch : (((s >> T.kb) & 1) ? T.ch : -T.ch);
    }
    const bool ui = (G.bits >> 16) & 1 ? uhi : ulo;             // bit 16: site i is the higher one
    const double f = ui ? co : -co;
    const int64_t partner = bond_partner<MODE>(dm, lbin, K, s, idx, lo, hi);
    if (NCK == 2) {
      const double2 v = ((const double2 *)ket)[partner];
      ar += f * v.x;
      ai += f * v.y;
    } else {
      ar += f * ket[partner];
    }
  }
  return make_double2(ar, ai);
}

// NC: components of psi (write form) or of bra (bracket form; the ket is ComplexF64)
template <int NC, bool BRACKET, int MODE>
__global__ __launch_bounds__(256) void k_dcurrent(sd_dev_model dm, const double *__restrict__ vec, const double *__restrict__ bra,
                                                  const sd_dgroup *__restrict__ groups, int n_groups,
                                                  const sd_dterm_dev *__restrict__ terms, double2 *__restrict__ out,
                                                  double *__restrict__ partials) {
  constexpr int NCK = BRACKET ? 2 : NC;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  double *red = reinterpret_cast<double *>(smem);            // 32 doubles
  int64_t *lbin = reinterpret_cast<int64_t *>(red + 32);     // lbin[n * K + k] = C(n, k), n < L, k <= nup (MODE 0: the rank walk)
  const int K = (dm.nup > 0 ? dm.nup : 0) + 1;
  fill_lbin<MODE>(dm, lbin, K);
  double sr = 0.0, si = 0.0;
  auto row = [&](uint64_t s, int64_t idx) {
    const double2 a = dcurrent_row<NCK, MODE>(dm, vec, groups, n_groups, terms, lbin, K, s, idx);
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

#define SD_DCURRENT_TILE_BLOCKS 4096     // tiled plans: workgroups, as k_current's
#define SD_DCURRENT_ROW_BLOCKS 8192      // blocks of 256 rows (per-row plans, full basis), as k_current's

template <int NC, bool BRACKET>
void launch_mode(int mode, unsigned nb, size_t shmem, hipStream_t st, const sd_dev_model &dm, const double *vec, const double *bra,
                 const sd_dgroup *groups, int n_groups, const sd_dterm_dev *terms, double2 *out, double *partials) {
  sd_with_mode(mode, [&](auto M) {
    hipLaunchKernelGGL((k_dcurrent<NC, BRACKET, decltype(M)::value>), dim3(nb), dim3(256), shmem, st, dm, vec, bra, groups, n_groups, terms,
                       out, partials);
  });
}

}  // namespace

// Write form (out != null): out = J vec, vec of `dtype`, out ComplexF64, must not alias vec.  Bracket form (out == null):
// dst[0..1] (device) = <bra|J|vec>, bra of `dtype`, vec ComplexF64.  groups_dev / terms_dev: the device tables of the list
// (n_groups == 0: the empty list, J = 0).  Launch caps as sd_launch_current.  Queued on the context's stream.
int sd_launch_dcurrent(sd_ctx *ctx, const sd_model *m, int dtype, const void *vec, const void *bra, const sd_dgroup *groups_dev,
                       int n_groups, const sd_dterm_dev *terms_dev, void *out, double *dst) {
  if (int rc = sd_gather_check(ctx, m, dtype, "the energy current needs")) return rc;
  const sd_dev_model &dm = m->dm;
  const bool bracket = out == nullptr;
  if (dm.n_local == 0 || n_groups == 0) {      // no rows, or no terms: a zero bracket, a zero vector
    if (bracket) SD_HIP(ctx, hipMemsetAsync(dst, 0, 2 * sizeof(double), ctx->stream));
    else if (dm.n_local > 0) SD_HIP(ctx, hipMemsetAsync(out, 0, 2 * sizeof(double) * (size_t)dm.n_local, ctx->stream));
    return SD_OK;
  }
  const sd_gather_grid g = sd_gather_grid_of(m, SD_DCURRENT_TILE_BLOCKS, SD_DCURRENT_ROW_BLOCKS);
  const int mode = g.mode;
  const unsigned nb = std::max(g.nb, 1u);
  const size_t shmem = 32 * sizeof(double) + g.lbin_bytes;
  if (bracket) { int rc = sd_ensure_partials(ctx, 2 * (size_t)nb + 2 * SD_RED_STAGE_BLOCKS); if (rc) return rc; }
  const double *v = (const double *)vec, *b = (const double *)bra;
  double2 *o = (double2 *)out;
  const bool c = dtype == SD_C128;
  if (bracket) {
    if (c) launch_mode<2, true>(mode, nb, shmem, ctx->stream, dm, v, b, groups_dev, n_groups, terms_dev, o, ctx->d_partials);
    else launch_mode<1, true>(mode, nb, shmem, ctx->stream, dm, v, b, groups_dev, n_groups, terms_dev, o, ctx->d_partials);
  } else {
    if (c) launch_mode<2, false>(mode, nb, shmem, ctx->stream, dm, v, b, groups_dev, n_groups, terms_dev, o, ctx->d_partials);
    else launch_mode<1, false>(mode, nb, shmem, ctx->stream, dm, v, b, groups_dev, n_groups, terms_dev, o, ctx->d_partials);
  }
  SD_HIP(ctx, hipGetLastError());
  if (bracket) return sd_reduce_pairs(ctx, (int64_t)nb, dst);
  return SD_OK;
}
