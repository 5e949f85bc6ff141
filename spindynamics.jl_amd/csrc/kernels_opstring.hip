// Operator strings: any product of S^+, S^-, S^z on distinct sites, and sums of such products, from one gather kernel
// family.  Site i is bit i - 1 of a configuration s.  A term (plus P, minus M, z Z, c, op) stands for
//     c prod_{i in P} S^+_i prod_{j in M} S^-_j prod_{l in Z} S^z_l          (P, M, Z pairwise disjoint site masks),
// consecutive terms with equal (P, M, op) form a GROUP and share one gather, and
//     (O psi)[s] = sum_groups [(s & P) == P and (s & M) == 0] co_g(s) psi[row(s ^ (P | M))],
//     co_g(s)    = sum over the group's terms, in list order from (0, 0), of sigma_t(s) ch_t,
//                  sigma_t(s) = +1 when popcount(~s & Z_t) is even, else -1;  ch_t = c_t 2^-|Z_t| (scaled on the host, exact),
//     product      t_re = co_re v_re - co_im v_im, t_im = co_re v_im + co_im v_re, both products first, then the add / subtract
//                  (a Float64 psi: t_re = co_re v, t_im = co_im v),
// (re, im) accumulated from (0, 0) in group order.  Nothing is fused (-ffp-contract=off).  A group with P = M = 0 is diagonal: its
// source is the row itself and it needs no rank.  tests/opstring_ref.py restates exactly this.
//   k_opstring        out = O psi, or the fused out = O psi + b y (one complex multiply, then one add, per entry).  Every row is written.
//   k_opstring_expect sum_s conj(bra[s]) (O_k ket)[s] for K operators in one pass, no vector O_k ket stored.  Layout of k_sym_overlaps:
//                     workgroup column blockIdx.x owns a chunk of SD_OPS_CHUNK operators, blockIdx.y a share of the rows, the chunk is
//                     the FAST grid index; per-thread accumulators, block_reduce2, block partials in ctx->d_partials (one list of
//                     pairs per operator), sd_reduce_pairs_batched adds them in a fixed order.  No atomics; the grid depends on the
//                     plan and K alone: the same call gives the same bits.
// Rows and their configurations (MODE) by for_rows (gather_common.hpp): 1 the tile's prefix and the suffix table of a tiled sector
// plan, 0 unrank_g of the row, 2 the row index (full basis).  Source rows by config_row (same header).  The group and term tables are
// read from global memory with wave-uniform indices (scalar loads).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "gather_common.hpp"

using namespace sd_dev;

namespace {

#define SD_OPS_CHUNK 8                  // operators per workgroup column (expectations)
#define SD_OPS_RED_BLOCKS 2048          // expectations: row blocks (grid.y), tiles or blocks of 256 rows, as k_pairs
#define SD_OPS_TILE_BLOCKS 4096         // write form, tiled plans: workgroups, as k_dcurrent
#define SD_OPS_ROW_BLOCKS 8192          // write form, blocks of 256 rows (per-row plans, full basis), as k_dcurrent

// (O psi)[s] over groups[g0 .. g1) for row idx with configuration s.  NCI = 1: psi is real; WANT_IM = false: the imaginary part is
// not formed (a Float64 output: every ch_im is 0).
template <int NCI, bool WANT_IM, int MODE>
__device__ __forceinline__ double2 opstring_row(const sd_dev_model &dm, const double *__restrict__ psi,
                                                const sd_opgroup *__restrict__ groups, int g0, int g1,
                                                const sd_opterm_dev *__restrict__ terms, const int64_t *lbin, int K, uint64_t s,
                                                int64_t idx) {
  double re = 0.0, im = 0.0;
  for (int g = g0; g < g1; ++g) {
    const sd_opgroup G = groups[g];
    if ((s & G.plus) != G.plus || (s & G.minus) != 0) continue;
    double cr = 0.0, ci = 0.0;
    for (int t = G.first; t < G.first + G.count; ++t) {
      const sd_opterm_dev T = terms[t];
      const bool neg = __popcll(~s & T.z) & 1;
      cr += neg ? -T.ch_re : T.ch_re;
      if (WANT_IM) ci += neg ? -T.ch_im : T.ch_im;
    }
    const uint64_t flip = G.plus | G.minus;
    const int64_t src = flip ? config_row<MODE>(dm, lbin, K, s ^ flip) : idx;
    if (NCI == 2) {
      const double2 v = ((const double2 *)psi)[src];
      const double tr = cr * v.x - ci * v.y, ti = cr * v.y + ci * v.x;
      re += tr; im += ti;
    } else {
      const double v = psi[src];
      re += cr * v;
      if (WANT_IM) im += ci * v;
    }
  }
  return make_double2(re, im);
}

// NCI / NCO: components of psi / out (NCO >= NCI; NCO == 1 only with every coefficient real and b_im == 0)
template <int NCI, int NCO, int MODE, bool FUSED>
__global__ __launch_bounds__(256) void k_opstring(sd_dev_model dm, const double *__restrict__ psi,
                                                  const sd_opgroup *__restrict__ groups, int n_groups,
                                                  const sd_opterm_dev *__restrict__ terms, const double *y, double br, double bi,
                                                  double *out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  int64_t *lbin = reinterpret_cast<int64_t *>(smem);
  const int K = (dm.nup > 0 ? dm.nup : 0) + 1;
  fill_lbin<MODE>(dm, lbin, K);
  for_rows<MODE>(dm, blockIdx.x, gridDim.x, [&](uint64_t s, int64_t idx) {
    double2 a = opstring_row<NCI, NCO == 2, MODE>(dm, psi, groups, 0, n_groups, terms, lbin, K, s, idx);
    if (NCO == 2) {
      if (FUSED) {
        const double2 w = ((const double2 *)y)[idx];
        const double tr = br * w.x - bi * w.y, ti = br * w.y + bi * w.x;
        a.x = a.x + tr;
        a.y = a.y + ti;
      }
      ((double2 *)out)[idx] = a;
    } else {
      double v = a.x;
      if (FUSED) v = v + br * y[idx];
      out[idx] = v;
    }
  });
}

// partials: one list of gridDim.y pairs per operator, list k at partials + 2 * k * gridDim.y
template <int NC, int MODE>
__global__ __launch_bounds__(256) void k_opstring_expect(sd_dev_model dm, const double *__restrict__ bra, const double *__restrict__ ket,
                                                         const sd_opgroup *__restrict__ groups, const int32_t *__restrict__ op_first,
                                                         const sd_opterm_dev *__restrict__ terms, int n_ops,
                                                         double *__restrict__ partials) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  double *red = reinterpret_cast<double *>(smem);            // 32 doubles
  int64_t *lbin = reinterpret_cast<int64_t *>(red + 32);
  const int K = (dm.nup > 0 ? dm.nup : 0) + 1;
  fill_lbin<MODE>(dm, lbin, K);
  const int c0 = blockIdx.x * SD_OPS_CHUNK, cn = min(SD_OPS_CHUNK, n_ops - c0);
  int g0[SD_OPS_CHUNK], g1[SD_OPS_CHUNK];
  double ar[SD_OPS_CHUNK], ai[SD_OPS_CHUNK];
#pragma unroll
  for (int k = 0; k < SD_OPS_CHUNK; ++k) {
    g0[k] = k < cn ? op_first[c0 + k] : 0;
    g1[k] = k < cn ? op_first[c0 + k + 1] : 0;
    ar[k] = 0.0; ai[k] = 0.0;
  }
  for_rows<MODE>(dm, blockIdx.y, gridDim.y, [&](uint64_t s, int64_t idx) {
    double br, bi = 0.0;
    if (NC == 2) { const double2 b = ((const double2 *)bra)[idx]; br = b.x; bi = b.y; }
    else br = bra[idx];
#pragma unroll
    for (int k = 0; k < SD_OPS_CHUNK; ++k) {
      if (k >= cn) continue;
      const double2 u = opstring_row<NC, true, MODE>(dm, ket, groups, g0[k], g1[k], terms, lbin, K, s, idx);
      ar[k] += br * u.x + bi * u.y;                          // conj(bra[s]) * (O_k ket)[s]
      ai[k] += br * u.y - bi * u.x;
    }
  });
#pragma unroll
  for (int k = 0; k < SD_OPS_CHUNK; ++k) {
    double a = ar[k], b = ai[k];
    block_reduce2(a, b, red);
    if (threadIdx.x == 0 && k < cn) {
      double *__restrict__ p = partials + 2 * ((size_t)(c0 + k) * gridDim.y + blockIdx.y);
      p[0] = a; p[1] = b;
    }
    __syncthreads();
  }
}

template <int NCI, int NCO, bool FUSED>
void launch_write(const sd_gather_grid &g, hipStream_t st, const sd_dev_model &dm, const double *psi, const sd_opgroup *groups, int n_groups,
                  const sd_opterm_dev *terms, const double *y, double br, double bi, double *out) {
  const dim3 grid(g.nb), blk(256);
  sd_with_mode(g.mode, [&](auto M) {
    hipLaunchKernelGGL((k_opstring<NCI, NCO, decltype(M)::value, FUSED>), grid, blk, g.lbin_bytes, st, dm, psi, groups, n_groups, terms, y,
                       br, bi, out);
  });
}

template <int NC>
void launch_expect(const sd_gather_grid &g, unsigned nchunks, hipStream_t st, const sd_dev_model &dm, const double *bra, const double *ket,
                   const sd_opgroup *groups, const int32_t *op_first, const sd_opterm_dev *terms, int n_ops, double *partials) {
  const dim3 grid(nchunks, g.nb), blk(256);
  const size_t shmem = 32 * sizeof(double) + g.lbin_bytes;
  sd_with_mode(g.mode, [&](auto M) {
    hipLaunchKernelGGL((k_opstring_expect<NC, decltype(M)::value>), grid, blk, shmem, st, dm, bra, ket, groups, op_first, terms, n_ops,
                       partials);
  });
}

int ops_common(sd_ctx *ctx, const sd_model *m, int dtype) { return sd_gather_check(ctx, m, dtype, "operator strings need", true); }

// every launcher here takes at least one block
sd_gather_grid ops_grid(const sd_model *m, bool reduction) {
  sd_gather_grid g = reduction ? sd_gather_grid_of(m, SD_OPS_RED_BLOCKS, SD_OPS_RED_BLOCKS)
                               : sd_gather_grid_of(m, SD_OPS_TILE_BLOCKS, SD_OPS_ROW_BLOCKS);
  g.nb = std::max(g.nb, 1u);
  return g;
}

}  // namespace

// The callers (recur.cpp) have validated the list against the model (sd_opstring_build): masks inside L bits and disjoint,
// |plus| == |minus| in a sector, so every source configuration lies in the basis.
int sd_launch_opstring(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi, const sd_opgroup *groups_dev, int n_groups,
                       const sd_opterm_dev *terms_dev, const void *y, double b_re, double b_im, int dtype_out, void *out) {
  int rc = ops_common(ctx, m, dtype);
  if (rc) return rc;
  if (dtype_out != SD_C128 && !(dtype_out == SD_F64 && dtype == SD_F64))
    return sd_set_err(ctx, SD_EARG, "the output is SD_C128, or SD_F64 for an SD_F64 psi with real coefficients");
  if (dtype_out == SD_F64 && y && b_im != 0.0) return sd_set_err(ctx, SD_EARG, "a Float64 output takes a real b (b_im = 0)");
  const sd_dev_model &dm = m->dm;
  if (dm.n_local == 0) return SD_OK;
  const sd_gather_grid g = ops_grid(m, false);
  const double *p = (const double *)psi, *yv = (const double *)y;
  double *o = (double *)out;
  hipStream_t st = ctx->stream;
  if (dtype == SD_C128) {
    if (y) launch_write<2, 2, true>(g, st, dm, p, groups_dev, n_groups, terms_dev, yv, b_re, b_im, o);
    else launch_write<2, 2, false>(g, st, dm, p, groups_dev, n_groups, terms_dev, yv, b_re, b_im, o);
  } else if (dtype_out == SD_C128) {
    if (y) launch_write<1, 2, true>(g, st, dm, p, groups_dev, n_groups, terms_dev, yv, b_re, b_im, o);
    else launch_write<1, 2, false>(g, st, dm, p, groups_dev, n_groups, terms_dev, yv, b_re, b_im, o);
  } else {
    if (y) launch_write<1, 1, true>(g, st, dm, p, groups_dev, n_groups, terms_dev, yv, b_re, b_im, o);
    else launch_write<1, 1, false>(g, st, dm, p, groups_dev, n_groups, terms_dev, yv, b_re, b_im, o);
  }
  SD_HIP(ctx, hipGetLastError());
  return SD_OK;
}

int sd_launch_opstring_expect(sd_ctx *ctx, const sd_model *m, int dtype, const void *bra, const void *ket, const sd_opgroup *groups_dev,
                              const int32_t *op_first_dev, const sd_opterm_dev *terms_dev, int n_ops, double *dst) {
  int rc = ops_common(ctx, m, dtype);
  if (rc) return rc;
  if (n_ops < 1 || n_ops > SD_OPSTRING_MAX_OPS) return sd_set_err(ctx, SD_EINTERNAL, "operator strings: bad operator count");
  const sd_dev_model &dm = m->dm;
  if (dm.n_local == 0) {      // no rows: every sum is empty
    SD_HIP(ctx, hipMemsetAsync(dst, 0, 2 * (size_t)n_ops * sizeof(double), ctx->stream));
    return SD_OK;
  }
  const sd_gather_grid g = ops_grid(m, true);
  const unsigned nchunks = (unsigned)((n_ops + SD_OPS_CHUNK - 1) / SD_OPS_CHUNK);
  rc = sd_ensure_partials(ctx, 2 * (size_t)n_ops * g.nb);
  if (rc) return rc;
  if (dtype == SD_C128)
    launch_expect<2>(g, nchunks, ctx->stream, dm, (const double *)bra, (const double *)ket, groups_dev, op_first_dev, terms_dev, n_ops, ctx->d_partials);
  else
    launch_expect<1>(g, nchunks, ctx->stream, dm, (const double *)bra, (const double *)ket, groups_dev, op_first_dev, terms_dev, n_ops, ctx->d_partials);
  SD_HIP(ctx, hipGetLastError());
  return sd_reduce_pairs_batched(ctx, (int64_t)g.nb, n_ops, dst, 2);
}
