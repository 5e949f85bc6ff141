// Lattice symmetry operators.  Site i is bit i - 1 of a configuration, L-bit masks implied:
//     T s = rotate left by one (the spin of site i moves to site i + 1 mod L),  R s = bit reversal over L bits (site i <-> L + 1 - i),
//     Z s = ~s (every spin flipped; the full basis and half-filled sectors only).
// A group element g = (r, refl, flip), code r | refl << 8 | flip << 9, is U_g = T^r R^refl Z^flip with U_g |s> = |T^r R^refl Z^flip s>, so
//     (U_g psi)[idx(s)] = psi[idx(src_g(s))],   src_g(s) = Z^flip R^refl T^-r s            (sym_source)
// -- a permutation gather.  Three kernels:
//   k_sym_apply    out = U_g x, or the fused out = U_g x + c y (one row of y per row of out; a chain of shifts).  The plain form
//                  copies bits.
//   k_sym_overlaps <bra|U_g|ket> = sum_s conj(bra[s]) ket[src_g(s)] for a list of elements in one pass.  Layout of k_pairs: workgroup
//                  column blockIdx.x owns a chunk of SD_SYM_CHUNK elements, blockIdx.y a share of the rows, the chunk is the FAST grid
//                  index so that the workgroups in flight read the same rows of bra; per-thread accumulators, block_reduce2, block
//                  partials in ctx->d_partials, k_chunk_reduce adds them in a fixed order.  No atomics, and the grid depends on the plan
//                  alone: the same call gives the same bits.
//   k_sym_project  out = sum_g c_g U_g psi for a list with complex coefficients in one pass: every row gathers once per element.
//                  ORDER (the restatement tests/symmetry_ref.py follows it): (re, im) start at (0, 0); elements in list order; the
//                  term of element g is t = c_g psi[src_g(s)] with t_re = c_re v_re - c_im v_im and t_im = c_re v_im + c_im v_re formed
//                  first (for a Float64 psi t_re = c_re v, t_im = c_im v), then re += t_re, im += t_im.  Nothing is fused.
// Rows and their configurations (MODE) by for_rows (gather_common.hpp): 1 the tile's prefix and the suffix table of a tiled sector
// plan, 0 unrank_g of the row, 2 the row index (full basis).  Source row of a configuration t by config_row (same header): MODE 1 the
// plan's own rank addr[prefix of t] + suf_rank[suffix of t], two cached loads; MODE 0 rank_g with the binomials in LDS; MODE 2 t itself.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "gather_common.hpp"

using namespace sd_dev;

namespace {

#define SD_SYM_CHUNK 8                   // elements per workgroup column (overlaps)
#define SD_SYM_ROW (2 * SD_SYM_CHUNK)    // doubles of a block's partial row
#define SD_SYM_RED_BLOCKS 2048           // overlaps: row blocks (grid.y), tiles or blocks of 256 rows, as k_pairs
#define SD_SYM_TILE_BLOCKS 4096          // write form and projector, tiled plans: workgroups, as k_current
#define SD_SYM_ROW_BLOCKS 8192           // write form and projector, blocks of 256 rows (per-row plans, full basis), as k_current

__device__ __forceinline__ uint64_t sym_source(uint64_t s, int code, int L, uint64_t mask) {
  const int r = code & 255;
  if (r) s = ((s >> r) | (s << (L - r))) & mask;           // T^-r: rotate right
  if (code & 256) s = __brevll(s) >> (64 - L);
  if (code & 512) s = ~s & mask;
  return s;
}

// out = U_g x (+ (cr + i ci) y, FUSED; a Float64 launch has ci == 0)
template <int NC, int MODE, bool FUSED>
__global__ __launch_bounds__(256) void k_sym_apply(sd_dev_model dm, int code, const double *__restrict__ x, const double *y,
                                                   double cr, double ci, double *out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  int64_t *lbin = reinterpret_cast<int64_t *>(smem);
  const int K = (dm.nup > 0 ? dm.nup : 0) + 1;
  fill_lbin<MODE>(dm, lbin, K);
  const uint64_t mask = ~(uint64_t)0 >> (64 - dm.L);
  for_rows<MODE>(dm, blockIdx.x, gridDim.x, [&](uint64_t s, int64_t idx) {
    const int64_t src = config_row<MODE>(dm, lbin, K, sym_source(s, code, dm.L, mask));
    if (NC == 2) {
      double2 v = ((const double2 *)x)[src];
      if (FUSED) {
        const double2 w = ((const double2 *)y)[idx];
        v.x = v.x + (cr * w.x - ci * w.y);
        v.y = v.y + (cr * w.y + ci * w.x);
      }
      ((double2 *)out)[idx] = v;
    } else {
      double v = x[src];
      if (FUSED) v = v + cr * y[idx];
      out[idx] = v;
    }
  });
}

template <int NC, int MODE>
__global__ __launch_bounds__(256) void k_sym_overlaps(sd_dev_model dm, const double *__restrict__ bra, const double *__restrict__ ket,
                                                      const int *__restrict__ codes, int ncodes, double *__restrict__ partials) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  double *red = reinterpret_cast<double *>(smem);            // 32 doubles
  int64_t *lbin = reinterpret_cast<int64_t *>(red + 32);
  const int K = (dm.nup > 0 ? dm.nup : 0) + 1;
  fill_lbin<MODE>(dm, lbin, K);
  const uint64_t mask = ~(uint64_t)0 >> (64 - dm.L);
  const int c0 = blockIdx.x * SD_SYM_CHUNK, cn = min(SD_SYM_CHUNK, ncodes - c0);
  int cd[SD_SYM_CHUNK];
  double ar[SD_SYM_CHUNK], ai[SD_SYM_CHUNK];
#pragma unroll
  for (int k = 0; k < SD_SYM_CHUNK; ++k) { cd[k] = k < cn ? codes[c0 + k] : 0; ar[k] = 0.0; ai[k] = 0.0; }
  for_rows<MODE>(dm, blockIdx.y, gridDim.y, [&](uint64_t s, int64_t idx) {
    double br, bi = 0.0;
    if (NC == 2) { const double2 b = ((const double2 *)bra)[idx]; br = b.x; bi = b.y; }
    else br = bra[idx];
#pragma unroll
    for (int k = 0; k < SD_SYM_CHUNK; ++k) {
      if (k >= cn) continue;
      const int64_t src = config_row<MODE>(dm, lbin, K, sym_source(s, cd[k], dm.L, mask));
      if (NC == 2) {
        const double2 u = ((const double2 *)ket)[src];
        ar[k] += br * u.x + bi * u.y;                        // conj(bra[s]) * ket[src]
        ai[k] += br * u.y - bi * u.x;
      } else {
        ar[k] += br * ket[src];
      }
    }
  });
  double *__restrict__ prow = partials + ((size_t)blockIdx.x * gridDim.y + blockIdx.y) * SD_SYM_ROW;
#pragma unroll
  for (int k = 0; k < SD_SYM_CHUNK; ++k) {
    double a = ar[k], b = ai[k];
    block_reduce2(a, b, red);
    if (threadIdx.x == 0) { prow[2 * k] = a; prow[2 * k + 1] = b; }
    __syncthreads();
  }
}

// NCI / NCO: components of psi / out (NCO >= NCI; NCO == 1 only with every coefficient real).  coef[2g .. +1] = c_g.
template <int NCI, int NCO, int MODE>
__global__ __launch_bounds__(256) void k_sym_project(sd_dev_model dm, const double *__restrict__ psi, const int *__restrict__ codes,
                                                     const double *__restrict__ coef, int ncodes, double *__restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  int64_t *lbin = reinterpret_cast<int64_t *>(smem);
  const int K = (dm.nup > 0 ? dm.nup : 0) + 1;
  fill_lbin<MODE>(dm, lbin, K);
  const uint64_t mask = ~(uint64_t)0 >> (64 - dm.L);
  for_rows<MODE>(dm, blockIdx.x, gridDim.x, [&](uint64_t s, int64_t idx) {
    double re = 0.0, im = 0.0;
    for (int g = 0; g < ncodes; ++g) {                       // list order: see ORDER at the top
      const double cr = coef[2 * g], ci = coef[2 * g + 1];
      const int64_t src = config_row<MODE>(dm, lbin, K, sym_source(s, codes[g], dm.L, mask));
      if (NCI == 2) {
        const double2 v = ((const double2 *)psi)[src];
        const double tr = cr * v.x - ci * v.y, ti = cr * v.y + ci * v.x;
        re += tr; im += ti;
      } else {
        const double v = psi[src];
        re += cr * v;
        if (NCO == 2) im += ci * v;
      }
    }
    if (NCO == 2) ((double2 *)out)[idx] = make_double2(re, im);
    else out[idx] = re;
  });
}

template <int NC, bool FUSED>
void launch_apply(const sd_gather_grid &g, hipStream_t st, const sd_dev_model &dm, int code, const double *x, const double *y, double cr,
                  double ci, double *out) {
  const dim3 grid(g.nb), blk(256);
  sd_with_mode(g.mode, [&](auto M) {
    hipLaunchKernelGGL((k_sym_apply<NC, decltype(M)::value, FUSED>), grid, blk, g.lbin_bytes, st, dm, code, x, y, cr, ci, out);
  });
}

template <int NC>
void launch_overlaps(const sd_gather_grid &g, unsigned nchunks, hipStream_t st, const sd_dev_model &dm, const double *bra, const double *ket,
                     const int *codes, int ncodes, double *partials) {
  const dim3 grid(nchunks, g.nb), blk(256);
  const size_t shmem = 32 * sizeof(double) + g.lbin_bytes;
  sd_with_mode(g.mode, [&](auto M) {
    hipLaunchKernelGGL((k_sym_overlaps<NC, decltype(M)::value>), grid, blk, shmem, st, dm, bra, ket, codes, ncodes, partials);
  });
}

template <int NCI, int NCO>
void launch_project(const sd_gather_grid &g, hipStream_t st, const sd_dev_model &dm, const double *psi, const int *codes, const double *coef,
                    int ncodes, double *out) {
  const dim3 grid(g.nb), blk(256);
  sd_with_mode(g.mode, [&](auto M) {
    hipLaunchKernelGGL((k_sym_project<NCI, NCO, decltype(M)::value>), grid, blk, g.lbin_bytes, st, dm, psi, codes, coef, ncodes, out);
  });
}

int sym_common(sd_ctx *ctx, const sd_model *m, int dtype) { return sd_gather_check(ctx, m, dtype, "symmetry operators need", true); }

sd_gather_grid sym_grid(const sd_model *m, bool reduction) {
  return reduction ? sd_gather_grid_of(m, SD_SYM_RED_BLOCKS, SD_SYM_RED_BLOCKS) : sd_gather_grid_of(m, SD_SYM_TILE_BLOCKS, SD_SYM_ROW_BLOCKS);
}

}  // namespace

// The callers (recur.cpp) have validated the element codes against the model: 0 <= r < L, no other bits, Z only where it is defined.
int sd_launch_symmetry_apply(sd_ctx *ctx, const sd_model *m, int dtype, int code, const void *x, const void *y, double cr, double ci,
                             void *out) {
  int rc = sym_common(ctx, m, dtype);
  if (rc) return rc;
  if (dtype == SD_F64 && y && ci != 0.0) return sd_set_err(ctx, SD_EARG, "a Float64 vector takes a real coefficient");
  const sd_dev_model &dm = m->dm;
  if (dm.n_local == 0) return SD_OK;
  const sd_gather_grid g = sym_grid(m, false);
  const double *xv = (const double *)x, *yv = (const double *)y;
  double *o = (double *)out;
  if (dtype == SD_C128) {
    if (y) launch_apply<2, true>(g, ctx->stream, dm, code, xv, yv, cr, ci, o);
    else launch_apply<2, false>(g, ctx->stream, dm, code, xv, yv, cr, ci, o);
  } else {
    if (y) launch_apply<1, true>(g, ctx->stream, dm, code, xv, yv, cr, ci, o);
    else launch_apply<1, false>(g, ctx->stream, dm, code, xv, yv, cr, ci, o);
  }
  SD_HIP(ctx, hipGetLastError());
  return SD_OK;
}

int sd_launch_symmetry_overlaps(sd_ctx *ctx, const sd_model *m, int dtype, const void *bra, const void *ket, const int *codes_dev,
                                int ncodes, double *dst) {
  int rc = sym_common(ctx, m, dtype);
  if (rc) return rc;
  if (ncodes < 1 || ncodes > SD_SYM_MAX_ELEMENTS) return sd_set_err(ctx, SD_EINTERNAL, "symmetry overlaps: bad element count");
  const sd_dev_model &dm = m->dm;
  if (dm.n_local == 0) {      // no rows: every sum is empty
    SD_HIP(ctx, hipMemsetAsync(dst, 0, 2 * (size_t)ncodes * sizeof(double), ctx->stream));
    return SD_OK;
  }
  const sd_gather_grid g = sym_grid(m, true);
  const unsigned nchunks = (unsigned)((ncodes + SD_SYM_CHUNK - 1) / SD_SYM_CHUNK);
  rc = sd_ensure_partials(ctx, (size_t)nchunks * g.nb * SD_SYM_ROW);
  if (rc) return rc;
  if (dtype == SD_C128) launch_overlaps<2>(g, nchunks, ctx->stream, dm, (const double *)bra, (const double *)ket, codes_dev, ncodes, ctx->d_partials);
  else launch_overlaps<1>(g, nchunks, ctx->stream, dm, (const double *)bra, (const double *)ket, codes_dev, ncodes, ctx->d_partials);
  hipLaunchKernelGGL(k_chunk_reduce<SD_SYM_CHUNK>, dim3(nchunks), dim3(256), 0, ctx->stream, ctx->d_partials, (int)g.nb, ncodes, 1.0, dst);
  SD_HIP(ctx, hipGetLastError());
  return SD_OK;
}

int sd_launch_symmetry_project(sd_ctx *ctx, const sd_model *m, int dtype_in, const void *psi, const int *codes_dev,
                               const double *coef_dev, int ncodes, int dtype_out, void *out) {
  int rc = sym_common(ctx, m, dtype_in);
  if (rc) return rc;
  if (dtype_out != SD_C128 && !(dtype_out == SD_F64 && dtype_in == SD_F64))
    return sd_set_err(ctx, SD_EARG, "the projector's output is SD_C128, or SD_F64 for an SD_F64 psi with real coefficients");
  if (ncodes < 1 || ncodes > SD_SYM_MAX_ELEMENTS) return sd_set_err(ctx, SD_EINTERNAL, "symmetry projector: bad element count");
  const sd_dev_model &dm = m->dm;
  if (dm.n_local == 0) return SD_OK;
  const sd_gather_grid g = sym_grid(m, false);
  const double *p = (const double *)psi;
  double *o = (double *)out;
  if (dtype_in == SD_C128) launch_project<2, 2>(g, ctx->stream, dm, p, codes_dev, coef_dev, ncodes, o);
  else if (dtype_out == SD_C128) launch_project<1, 2>(g, ctx->stream, dm, p, codes_dev, coef_dev, ncodes, o);
  else launch_project<1, 1>(g, ctx->stream, dm, p, codes_dev, coef_dev, ncodes, o);
  SD_HIP(ctx, hipGetLastError());
  return SD_OK;
}
