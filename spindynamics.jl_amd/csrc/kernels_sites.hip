// Site projections for the site-resolved KPM correlations:
//     out[i] = sum_rows conj(bra[row]) * s_i(row) * ket[row],   i = 1..L,   s_i = +-1/2 the S^z value of site i,
// plus sum |ket|^2, from ONE pass over the two vectors.  bra is psi0 in its own element type (Float64: an 8 B/row stream),
// ket a ComplexF64 Chebyshev vector v_n = T_n(H~) S^z_j psi0; the L sums are the moments mu_n^{ij} against every site i.
//
// Decomposition of k_obs2 MODE 0 (kernels_aux.hip) with complex sums.  A tile's rows differ in the "variable" sites (the
// suffix sites of a sector plan, the low 10 index bits of the full basis) and share the "uniform" ones:
//   variable sites: one signed add of w = conj(bra) ket per row and site, in per-thread accumulators (2 x 16 doubles);
//   uniform sites : a wave sums its rows' w of the tile (butterfly: every lane ends with the same bits) and lane k adds that
//                   total, signed by bit k of the tile's uniform configuration, to ITS accumulator -- one complex
//                   accumulator per lane instead of 32 per thread, so the complex sums cost no more registers than k_obs2.
// Every sum runs in an order fixed by the plan and the launch geometry (grid.x does not depend on the batch): no atomics, the
// same call gives the same bits, and a vector of a batch gets the bits of a launch of its own.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "device_common.hpp"

using namespace sd_dev;

namespace {

#define SD_SITE_COLS 64    // complex columns of a block's partial row: [0, 16) variable sites, [16, 48) uniform sites, 63: (sum |ket|^2, 0)
#define SD_SITE_CHUNK 8    // sites per pass of the chunked form

// w = conj(bra[row]) * ket[row]; n2 += |ket[row]|^2
template <int NCB>
__device__ __forceinline__ double2 bra_ket(const double *__restrict__ bra, const double2 *__restrict__ ket, int64_t row, double &n2) {
  const double2 v = ket[row];
  n2 += v.x * v.x + v.y * v.y;
  if (NCB == 2) {
    const double2 b = ((const double2 *)bra)[row];
    return make_double2(b.x * v.x + b.y * v.y, b.x * v.y - b.y * v.x);
  }
  const double b = bra[row];
  return make_double2(b * v.x, b * v.y);
}

template <int NCB, bool FULL>
__global__ __launch_bounds__(256) void k_site_project(sd_dev_model dm, const double *__restrict__ bra, int64_t bra_bstride,
                                                      const double2 *__restrict__ ket, int64_t bstride,
                                                      double *__restrict__ partials) {
  constexpr int NV = 16, NU = 32;
  __shared__ double red[4][2 * SD_SITE_COLS];
  bra += (int64_t)blockIdx.y * bra_bstride * NCB;
  ket += (int64_t)blockIdx.y * bstride;
  double vr[NV], vi[NV];
#pragma unroll
  for (int k = 0; k < NV; ++k) { vr[k] = 0.0; vi[k] = 0.0; }
  double ur = 0.0, ui = 0.0, n2 = 0.0;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int nv = FULL ? 10 : dm.LS;                        // variable sites (the uniform ones: L - nv <= 32, checked by the host)
  const int64_t ntiles = FULL ? (dm.n_local >> 10) : (int64_t)dm.n_tiles;
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    uint64_t ubits;                                        // the uniform sites' bits, site order, from bit 0
    int64_t base;
    int len;
    const uint16_t *__restrict__ sufS = nullptr;
    if (FULL) {
      base = t << 10; len = 1024;
      ubits = (uint64_t)((dm.row_lo + base) >> 10);
    } else {
      const uint32_t P = dm.tile_prefix[t];
      base = dm.tile_base[t];
      const int t2 = dm.nup - __popc(P);
      len = (int)binom_g(dm, dm.LS, t2);
      sufS = dm.suf_states + dm.suf_off[t2];
      ubits = P;
    }
    if (wv * 64 >= len) continue;                          // wave-uniform: this wave holds no row of the tile
    double tr = 0.0, ti = 0.0;
    for (int i = threadIdx.x; i < len; i += 256) {
      const double2 w = bra_ket<NCB>(bra, ket, base + i, n2);
      const uint32_t var = FULL ? (uint32_t)i : (uint32_t)sufS[i];
      tr += w.x; ti += w.y;
#pragma unroll
      for (int k = 0; k < NV; ++k)
        if (k < nv) {
          const bool up = (var >> k) & 1u;
          vr[k] += up ? w.x : -w.x;
          vi[k] += up ? w.y : -w.y;
        }
    }
    for (int off = 32; off > 0; off >>= 1) { tr += __shfl_xor(tr, off, 64); ti += __shfl_xor(ti, off, 64); }
    const bool up = (ubits >> lane) & 1;                   // lane k < NU: uniform site k
    ur += up ? tr : -tr;
    ui += up ? ti : -ti;
  }
  auto put = [&](int col, double a, double b) {
    for (int off = 32; off > 0; off >>= 1) { a += __shfl_down(a, off, 64); b += __shfl_down(b, off, 64); }
    if (lane == 0) { red[wv][2 * col] = a; red[wv][2 * col + 1] = b; }
  };
  for (int k = threadIdx.x; k < 4 * 2 * SD_SITE_COLS; k += 256) (&red[0][0])[k] = 0.0;
  __syncthreads();
#pragma unroll
  for (int k = 0; k < NV; ++k) put(k, vr[k], vi[k]);
  if (lane < NU) { red[wv][2 * (NV + lane)] = ur; red[wv][2 * (NV + lane) + 1] = ui; }
  put(SD_SITE_COLS - 1, n2, 0.0);
  __syncthreads();
  if (threadIdx.x < 2 * SD_SITE_COLS)
    partials[((size_t)blockIdx.y * gridDim.x + blockIdx.x) * (2 * SD_SITE_COLS) + threadIdx.x] =
        ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
}

// Block k reduces the partial rows of vector k in a fixed order (8 strided sums per column, then their sum) and files
// out[2 (site-1) .. +1] = (1/2) sum (the +-w sums carry s_i = +-1/2), out[2L] = sum |ket|^2, out[2L+1] = 0.
__global__ __launch_bounds__(1024) void k_site_reduce(const double *__restrict__ partials, int nblocks, int L, int nv, int voff,
                                                      int uoff, double *__restrict__ out, int64_t dstride) {
  __shared__ double sm[8][2 * SD_SITE_COLS];
  const int c = threadIdx.x & (2 * SD_SITE_COLS - 1), j = threadIdx.x >> 7;
  const double *__restrict__ p = partials + (size_t)blockIdx.x * nblocks * (2 * SD_SITE_COLS);
  double a = 0.0;
  for (int b = j; b < nblocks; b += 8) a += p[(size_t)b * (2 * SD_SITE_COLS) + c];
  sm[j][c] = a;
  __syncthreads();
  if (threadIdx.x < 2 * SD_SITE_COLS) {
    double t = 0.0;
    for (int jj = 0; jj < 8; ++jj) t += sm[jj][c];
    const int col = c >> 1, part = c & 1, nu = L - nv;
    double *__restrict__ o = out + (size_t)blockIdx.x * dstride;
    if (col < nv) o[2 * (voff + col) + part] = 0.5 * t;
    else if (col >= 16 && col < 16 + nu) o[2 * (uoff + col - 16) + part] = 0.5 * t;
    else if (col == SD_SITE_COLS - 1) o[2 * L + part] = t;
  }
}

// Chunked form for plans without tiles (per-row rank / unrank, sd_model_path == 0) and for whatever the one-pass form does
// not take: SD_SITE_CHUNK sites per pass over the two vectors, like k_obs.  Partial row of a block: 16 site doubles, |ket|^2, 0.
// Not the shared row walk (for_rows, gather_common.hpp): dm.p at run time, a blockDim.x stride, dm.row_lo for sharded full bases.
#define SD_SITE_CROW 32
template <int NCB>
__global__ __launch_bounds__(256) void k_site_chunk(sd_dev_model dm, const double *__restrict__ bra, int64_t bra_bstride,
                                                    const double2 *__restrict__ ket, int64_t bstride, int c0, int cn,
                                                    double *__restrict__ partials) {
  __shared__ double red[32];
  bra += (int64_t)blockIdx.y * bra_bstride * NCB;
  ket += (int64_t)blockIdx.y * bstride;
  double ar[SD_SITE_CHUNK], ai[SD_SITE_CHUNK], n2 = 0.0;
#pragma unroll
  for (int k = 0; k < SD_SITE_CHUNK; ++k) { ar[k] = 0.0; ai[k] = 0.0; }
  auto row_add = [&](uint64_t s, int64_t row) {
    const double2 w = bra_ket<NCB>(bra, ket, row, n2);
#pragma unroll
    for (int k = 0; k < SD_SITE_CHUNK; ++k)
      if (k < cn) {
        const bool up = (s >> (c0 + k)) & 1;
        ar[k] += up ? w.x : -w.x;
        ai[k] += up ? w.y : -w.y;
      }
  };
  if (dm.p >= 0) {
    for (int t = blockIdx.x; t < dm.n_tiles; t += gridDim.x) {
      const uint32_t P = dm.tile_prefix[t];
      const int64_t base = dm.tile_base[t];
      const int t2 = dm.nup - __popc(P);
      const int len = (int)binom_g(dm, dm.LS, t2);
      const uint16_t *__restrict__ sufS = dm.suf_states + dm.suf_off[t2];
      for (int i = threadIdx.x; i < len; i += blockDim.x) row_add((uint64_t)P | ((uint64_t)sufS[i] << dm.p), base + i);
    }
  } else {
    const bool full = dm.nup < 0;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < dm.n_local; idx += stride)
      row_add(full ? (uint64_t)(dm.row_lo + idx) : unrank_g(dm, idx), idx);
  }
  double *__restrict__ prow = partials + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * SD_SITE_CROW;
#pragma unroll
  for (int k = 0; k < SD_SITE_CHUNK; ++k) {
    double a = ar[k], b = ai[k];
    block_reduce2(a, b, red);
    if (threadIdx.x == 0) { prow[2 * k] = a; prow[2 * k + 1] = b; }
    __syncthreads();
  }
  double a = n2, b = 0.0;
  block_reduce2(a, b, red);
  if (threadIdx.x == 0) { prow[2 * SD_SITE_CHUNK] = a; prow[2 * SD_SITE_CHUNK + 1] = b; }
}

__global__ __launch_bounds__(256) void k_site_chunk_reduce(const double *__restrict__ partials, int nblocks, int L, int c0, int cn,
                                                           double *__restrict__ out, int64_t dstride) {
  __shared__ double sm[8][SD_SITE_CROW];
  const int k = threadIdx.x & (SD_SITE_CROW - 1), j = threadIdx.x >> 5;
  const double *__restrict__ p = partials + (size_t)blockIdx.x * nblocks * SD_SITE_CROW;
  double a = 0.0;
  if (k < 2 * SD_SITE_CHUNK + 2)
    for (int b = j; b < nblocks; b += 8) a += p[(size_t)b * SD_SITE_CROW + k];
  sm[j][k] = a;
  __syncthreads();
  if (threadIdx.x < SD_SITE_CROW) {
    double t = 0.0;
    for (int jj = 0; jj < 8; ++jj) t += sm[jj][k];
    double *__restrict__ o = out + (size_t)blockIdx.x * dstride;
    if (k < 2 * cn) o[2 * c0 + k] = 0.5 * t;
    else if (c0 == 0 && (k == 2 * SD_SITE_CHUNK || k == 2 * SD_SITE_CHUNK + 1)) o[2 * L + (k - 2 * SD_SITE_CHUNK)] = t;
  }
}

}  // namespace

// dst + k * dstride, k < batch: 2L + 2 doubles -- (re, im) of <bra| S^z_i |ket_k> for i = 1..L, then (sum |ket_k|^2, 0).  ket_k =
// ket + k * bstride elements (ComplexF64), bra_k = bra + k * bra_bstride elements of dtype_bra (0: one bra for all).  Device
// pointers; queued on the context's stream, nothing is read back.
int sd_launch_site_project(sd_ctx *ctx, const sd_model *m, int dtype_bra, const void *bra, int64_t bra_bstride, const void *ket,
                           int64_t bstride, int batch, double *dst, int64_t dstride) {
  if (!m->dev_ready) return sd_set_err(ctx, SD_EARG, "model has no device tables (created without a context)");
  if (dtype_bra != SD_F64 && dtype_bra != SD_C128) return sd_set_err(ctx, SD_EARG, "dtype must be SD_F64 or SD_C128");
  if (m->nranks != 1) return sd_set_err(ctx, SD_EARG, "site projections need an unsharded model");
  if (batch < 1 || batch > 65535) return sd_set_err(ctx, SD_EINTERNAL, "site projection: bad batch");
  const sd_dev_model &dm = m->dm;
  const int L = dm.L;
  const bool c = dtype_bra == SD_C128;
  const double *b = (const double *)bra;
  const double2 *kt = (const double2 *)ket;
  const bool tiled = m->p >= 0 && dm.n_tiles > 0 && dm.LS <= 15 && dm.p <= 32;
  const bool fullt = m->p < 0 && m->full_ls > 0 && L >= 12 && L <= 40 && (dm.n_local >> 10) > 0;
  if (tiled || fullt) {
    const int64_t ntiles = fullt ? (dm.n_local >> 10) : (int64_t)dm.n_tiles;
    const int nb = (int)std::min<int64_t>(ntiles, 2048);
    int rc = sd_ensure_partials(ctx, (size_t)nb * 2 * SD_SITE_COLS * (size_t)batch);
    if (rc) return rc;
    const dim3 grid((unsigned)nb, (unsigned)batch);
    if (fullt) {
      if (c) hipLaunchKernelGGL((k_site_project<2, true>), grid, dim3(256), 0, ctx->stream, dm, b, bra_bstride, kt, bstride, ctx->d_partials);
      else hipLaunchKernelGGL((k_site_project<1, true>), grid, dim3(256), 0, ctx->stream, dm, b, bra_bstride, kt, bstride, ctx->d_partials);
    } else {
      if (c) hipLaunchKernelGGL((k_site_project<2, false>), grid, dim3(256), 0, ctx->stream, dm, b, bra_bstride, kt, bstride, ctx->d_partials);
      else hipLaunchKernelGGL((k_site_project<1, false>), grid, dim3(256), 0, ctx->stream, dm, b, bra_bstride, kt, bstride, ctx->d_partials);
    }
    const int nv = fullt ? 10 : dm.LS;
    hipLaunchKernelGGL(k_site_reduce, dim3((unsigned)batch), dim3(1024), 0, ctx->stream, ctx->d_partials, nb, L, nv, fullt ? 0 : dm.p,
                       fullt ? 10 : 0, dst, dstride);
    SD_HIP(ctx, hipGetLastError());
    return SD_OK;
  }
  int nb = m->p >= 0 ? std::min(dm.n_tiles, 2048) : (int)std::min<int64_t>(2048, (dm.n_local + 255) / 256);
  if (nb < 1) nb = 1;
  int rc = sd_ensure_partials(ctx, (size_t)nb * SD_SITE_CROW * (size_t)batch);
  if (rc) return rc;
  const dim3 grid((unsigned)nb, (unsigned)batch);
  for (int c0 = 0; c0 < L; c0 += SD_SITE_CHUNK) {
    const int cn = std::min(SD_SITE_CHUNK, L - c0);
    if (c) hipLaunchKernelGGL(k_site_chunk<2>, grid, dim3(256), 0, ctx->stream, dm, b, bra_bstride, kt, bstride, c0, cn, ctx->d_partials);
    else hipLaunchKernelGGL(k_site_chunk<1>, grid, dim3(256), 0, ctx->stream, dm, b, bra_bstride, kt, bstride, c0, cn, ctx->d_partials);
    hipLaunchKernelGGL(k_site_chunk_reduce, dim3((unsigned)batch), dim3(256), 0, ctx->stream, ctx->d_partials, nb, L, c0, cn, dst, dstride);
  }
  SD_HIP(ctx, hipGetLastError());
  return SD_OK;
}
