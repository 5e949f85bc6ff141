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
// Where the row's configuration comes from (MODE): 1 the tile's prefix and the suffix table of a tiled sector plan (as
// k_site_project), 0 unrank_g of the row (sector plans without tiles), 2 the row index itself (full basis).  Partner rows in a
// sector: the leading chain bonds (b, b+1) by the closed form of the combinadic order,
//     idx +- C(L - b - 1, u),   u = ups among the sites above b + 1,   + when site b is the up one,
// with the binomials in LDS; every other bond by the rank walk, as k_apply_short / k_apply_generic do.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "device_common.hpp"

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
  if (MODE != 2 && dm.nn_hops > 0) {
    for (int k = threadIdx.x; k < dm.L * K; k += 256) lbin[k] = dm.binom[(k / K) * (SD_MAX_L + 1) + (k % K)];
    __syncthreads();
  }
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
  if (MODE == 1) {
    for (int t = blockIdx.x; t < dm.n_tiles; t += gridDim.x) {
      const uint32_t P = dm.tile_prefix[t];
      const int64_t base = dm.tile_base[t];
      const int t2 = dm.nup - __popc(P);
      const int len = (int)binom_g(dm, dm.LS, t2);
      const uint16_t *__restrict__ sufS = dm.suf_states + dm.suf_off[t2];
      for (int i = threadIdx.x; i < len; i += 256) row((uint64_t)P | ((uint64_t)sufS[i] << dm.p), base + i);
    }
  } else {
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < dm.n_local; idx += stride)
      row(MODE == 2 ? (uint64_t)idx : unrank_g(dm, idx), idx);
  }
  if (BRACKET) {
    block_reduce2(sr, si, red);
    if (threadIdx.x == 0) { partials[2 * (size_t)blockIdx.x] = sr; partials[2 * (size_t)blockIdx.x + 1] = si; }
  }
}

template <int NC, bool BRACKET>
void launch_mode(int mode, unsigned nb, size_t shmem, hipStream_t st, const sd_dev_model &dm, const double *vec, const double *bra,
                 const double *wt, double2 *out, double *partials) {
  if (mode == 1) hipLaunchKernelGGL((k_current<NC, BRACKET, 1>), dim3(nb), dim3(256), shmem, st, dm, vec, bra, wt, out, partials);
  else if (mode == 2) hipLaunchKernelGGL((k_current<NC, BRACKET, 2>), dim3(nb), dim3(256), shmem, st, dm, vec, bra, wt, out, partials);
  else hipLaunchKernelGGL((k_current<NC, BRACKET, 0>), dim3(nb), dim3(256), shmem, st, dm, vec, bra, wt, out, partials);
}

}  // namespace

// Write form (out != null): out = J_w vec, vec of `dtype`, out ComplexF64, must not alias vec.  Bracket form (out == null):
// dst[0..1] (device) = <bra|J_w|vec>, bra of `dtype`, vec ComplexF64.  wt_dev: the n_hop products w_b t_b on the device.
// Queued on the context's stream.
int sd_launch_current(sd_ctx *ctx, const sd_model *m, int dtype, const void *vec, const void *bra, const double *wt_dev, void *out,
                      double *dst) {
  if (!m->dev_ready) return sd_set_err(ctx, SD_EARG, "model has no device tables (created without a context)");
  if (dtype != SD_F64 && dtype != SD_C128) return sd_set_err(ctx, SD_EARG, "dtype must be SD_F64 or SD_C128");
  if (m->nranks != 1) return sd_set_err(ctx, SD_EARG, "the spin current needs an unsharded model");
  const sd_dev_model &dm = m->dm;
  const bool bracket = out == nullptr;
  if (dm.n_local == 0) {      // no rows: the bracket is zero
    if (bracket) SD_HIP(ctx, hipMemsetAsync(dst, 0, 2 * sizeof(double), ctx->stream));
    return SD_OK;
  }
  const int mode = dm.nup < 0 ? 2 : (m->p >= 0 && dm.n_tiles > 0) ? 1 : 0;
  int64_t nb64 = mode == 1 ? std::min<int64_t>(dm.n_tiles, 4096) : std::min<int64_t>((dm.n_local + 255) / 256, 8192);
  const unsigned nb = (unsigned)std::max<int64_t>(nb64, 1);
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
