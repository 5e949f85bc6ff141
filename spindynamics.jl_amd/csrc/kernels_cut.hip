// Entanglement across a chain cut: the blocks of the reduced density matrix as Gram matrices of the matrices Psi_m
// that psi already is (cut_plan.cpp has the layout, the two forms and the work list).
//   k_cut_gram<NC, FORM, TILE> : one workgroup of 256 threads per work item (block, tile row ti, tile column tj >= ti, [k0, k1)).
//       E(g, kappa) = psi[seg[g] + kappa] (ACROSS) or psi[seg[kappa] + g] (INSIDE) is the element of Gram index g and summation index
//       kappa.  Per chunk of KC = 16 summation indices the two operand panels (TILE x KC elements each; one when ti == tj) are staged
//       in LDS as sX[component][kappa][g], the row padded to TILE + 1 doubles, while the chunk after it is already on its way from
//       memory in registers.  Global loads run along the contiguous index of the form (kappa for ACROSS, g for INSIDE), 16-byte
//       double2 for ComplexF64, 8-byte for Float64 (a segment start has no parity).  Thread (tx, ty) = (tid % 16, tid / 16) owns the
//       outputs (ty + 16 i, tx + 16 j), i, j < TILE / 16: the sixteen lanes of a read group take sixteen consecutive doubles of the
//       column panel and one or two adjacent doubles of the row panel -- no bank conflict; the ACROSS fill writes sixteen kappa rows
//       of one g, which the odd row length spreads over sixteen banks (the INSIDE fill writes consecutive g).
//       Accumulation: a conj(b) as four real products, each an explicit fma into its accumulator in the order re: ar br, ai bi;
//       im: ai br, -ar bi -- plain FP64 VALU, one rounding per product.  A load past the block's edge or past k1 is predicated and
//       contributes an exact zero; no address is formed from an index outside the block.  The tile's partial sums go to the item's
//       slot of the workspace.
//   k_cut_reduce<NC> : one workgroup per tile pair; adds the ns partials of every element in ascending kappa order and writes both
//       triangles, G[b][a] = conj(G[a][b]) from the one summed triangle, the diagonal's imaginary parts exactly 0.
// No atomics: the same call gives the same bits.  Every row and kappa index is 64-bit.
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>
#include <vector>

#include "device_common.hpp"

namespace {

constexpr int KC = SD_CUT_KC;

template <int NC>
__device__ __forceinline__ void load_el(const double *__restrict__ psi, int64_t idx, bool ok, double &re, double &im) {
  re = 0.0; im = 0.0;
  if (ok) {
    if (NC == 2) { const double2 v = ((const double2 *)psi)[idx]; re = v.x; im = v.y; }
    else re = psi[idx];
  }
}

// The elements thread `tid` fetches of the panel of tile `T` for the chunk at kc0: E = TILE * KC / 256 of them.
//   ACROSS: element e = tid + 256 q -> kappa = kc0 + e % KC, g = T TILE + e / KC (sixteen lanes read one segment's 16 kappa);
//           the segment starts of the thread's rows do not change with the chunk: `start` holds them (0 where g >= d, never used).
//   INSIDE: element e = tid + 256 q -> g = T TILE + e % TILE, kappa = kc0 + e / TILE (TILE lanes read consecutive g of one segment).
template <int NC, int FORM, int TILE>
__device__ __forceinline__ void fetch_panel(const double *__restrict__ psi, const int64_t *__restrict__ seg, const int64_t *start, int T,
                                            int64_t d, int64_t kc0, int64_t k1, double *re, double *im) {
  constexpr int E = TILE * KC / 256;
#pragma unroll
  for (int q = 0; q < E; ++q) {
    const int e = (int)threadIdx.x + 256 * q;
    if (FORM == SD_CUT_ACROSS) {
      const int64_t kap = kc0 + (e % KC), g = (int64_t)T * TILE + (e / KC);
      const bool ok = g < d && kap < k1;
      load_el<NC>(psi, ok ? start[q] + kap : 0, ok, re[q], im[q]);
    } else {
      const int64_t g = (int64_t)T * TILE + (e % TILE), kap = kc0 + (e / TILE);
      const bool ok = g < d && kap < k1;
      const int64_t s0 = ok ? seg[kap] : 0;
      load_el<NC>(psi, ok ? s0 + g : 0, ok, re[q], im[q]);
    }
  }
}

template <int NC, int FORM, int TILE>
__device__ __forceinline__ void store_panel(double (*s)[KC][TILE + 1], const double *re, const double *im) {
  constexpr int E = TILE * KC / 256;
#pragma unroll
  for (int q = 0; q < E; ++q) {
    const int e = (int)threadIdx.x + 256 * q;
    const int kl = FORM == SD_CUT_ACROSS ? e % KC : e / TILE, gl = FORM == SD_CUT_ACROSS ? e / KC : e % TILE;
    s[0][kl][gl] = re[q];
    if (NC == 2) s[1][kl][gl] = im[q];
  }
}

template <int NC, int FORM, int TILE>
__global__ __launch_bounds__(256) void k_cut_gram(const double *__restrict__ psi, const sd_cut_blk *__restrict__ blks,
                                                  const int64_t *__restrict__ segs, const sd_cut_item *__restrict__ items,
                                                  double *__restrict__ ws) {
  constexpr int R = TILE / 16;             // outputs per thread and direction
  constexpr int E = TILE * KC / 256;       // panel elements per thread and chunk
  __shared__ double sA[NC][KC][TILE + 1];
  __shared__ double sB[NC][KC][TILE + 1];
  const sd_cut_item it = items[blockIdx.x];
  const sd_cut_blk b = blks[it.block];
  const int64_t *__restrict__ seg = segs + b.seg_off;
  const int64_t d = b.d, k1 = it.k1;
  const bool diag = it.ti == it.tj;
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;

  int64_t startA[E], startB[E];
#pragma unroll
  for (int q = 0; q < E; ++q) {
    startA[q] = 0; startB[q] = 0;
    if (FORM == SD_CUT_ACROSS) {
      const int gl = ((int)threadIdx.x + 256 * q) / KC;
      const int64_t ga = (int64_t)it.ti * TILE + gl, gb = (int64_t)it.tj * TILE + gl;
      if (ga < d) startA[q] = seg[ga];
      if (gb < d) startB[q] = seg[gb];
    }
  }

  double accr[R][R], acci[R][R];
#pragma unroll
  for (int i = 0; i < R; ++i)
#pragma unroll
    for (int j = 0; j < R; ++j) { accr[i][j] = 0.0; acci[i][j] = 0.0; }

  double are[E], aim[E], bre[E], bim[E];
  fetch_panel<NC, FORM, TILE>(psi, seg, startA, it.ti, d, it.k0, k1, are, aim);
  if (!diag) fetch_panel<NC, FORM, TILE>(psi, seg, startB, it.tj, d, it.k0, k1, bre, bim);
  for (int64_t kc0 = it.k0; kc0 < k1; kc0 += KC) {
    __syncthreads();                       // the chunk before has been read
    store_panel<NC, FORM, TILE>(sA, are, aim);
    if (!diag) store_panel<NC, FORM, TILE>(sB, bre, bim);
    __syncthreads();
    if (kc0 + KC < k1) {                   // the next chunk travels while this one is multiplied
      fetch_panel<NC, FORM, TILE>(psi, seg, startA, it.ti, d, kc0 + KC, k1, are, aim);
      if (!diag) fetch_panel<NC, FORM, TILE>(psi, seg, startB, it.tj, d, kc0 + KC, k1, bre, bim);
    }
    double (*sBB)[KC][TILE + 1] = diag ? sA : sB;
#pragma unroll 4
    for (int kl = 0; kl < KC; ++kl) {
      double ar[R], ai[R], br[R], bi[R];
#pragma unroll
      for (int i = 0; i < R; ++i) {
        ar[i] = sA[0][kl][ty + 16 * i];
        br[i] = sBB[0][kl][tx + 16 * i];
        if (NC == 2) { ai[i] = sA[1][kl][ty + 16 * i]; bi[i] = sBB[1][kl][tx + 16 * i]; }
      }
#pragma unroll
      for (int i = 0; i < R; ++i)
#pragma unroll
        for (int j = 0; j < R; ++j) {
          accr[i][j] = fma(ar[i], br[j], accr[i][j]);
          if (NC == 2) {
            accr[i][j] = fma(ai[i], bi[j], accr[i][j]);
            acci[i][j] = fma(ai[i], br[j], acci[i][j]);
            acci[i][j] = fma(-ar[i], bi[j], acci[i][j]);
          }
        }
    }
  }
  double *__restrict__ out = ws + (size_t)it.slot * NC;
#pragma unroll
  for (int i = 0; i < R; ++i)
#pragma unroll
    for (int j = 0; j < R; ++j) {
      const int e = (ty + 16 * i) * TILE + (tx + 16 * j);
      if (NC == 2) ((double2 *)out)[e] = make_double2(accr[i][j], acci[i][j]);
      else out[e] = accr[i][j];
    }
}

template <int NC>
__global__ __launch_bounds__(256) void k_cut_reduce(const sd_cut_blk *__restrict__ blks, const sd_cut_pair *__restrict__ pairs,
                                                    const double *__restrict__ ws, double *__restrict__ G) {
  const sd_cut_pair p = pairs[blockIdx.x];
  const sd_cut_blk b = blks[p.block];
  const int tile = b.tile, tt = tile * tile;
  const int64_t d = b.d;
  double *__restrict__ Gb = G + (size_t)b.out_off * NC;
  const double *__restrict__ w0 = ws + (size_t)p.slot * NC;
  for (int e = threadIdx.x; e < tt; e += 256) {
    const int r = e / tile, c = e % tile;
    const int64_t gr = (int64_t)p.ti * tile + r, gc = (int64_t)p.tj * tile + c;
    if (gr >= d || gc >= d || (p.ti == p.tj && r > c)) continue;
    double sr = 0.0, si = 0.0;
    for (int s = 0; s < p.ns; ++s) {
      const double *__restrict__ w = w0 + ((size_t)s * tt + e) * NC;
      sr += w[0];
      if (NC == 2) si += w[1];
    }
    if (gr == gc) si = 0.0;
    if (NC == 2) {
      ((double2 *)Gb)[gr * d + gc] = make_double2(sr, si);
      if (gr != gc) ((double2 *)Gb)[gc * d + gr] = make_double2(sr, -si);
    } else {
      Gb[gr * d + gc] = sr;
      Gb[gc * d + gr] = sr;
    }
  }
}

struct PoolBlock {   // a block of the context's pool, given back when the launcher returns
  sd_ctx *ctx = nullptr;
  void *p = nullptr;
  size_t bytes = 0;
  ~PoolBlock() { if (p) sd_pool_give(ctx, p, bytes); }
  int take(sd_ctx *c, size_t want) { ctx = c; return sd_pool_take(c, want, &p, &bytes); }
};

template <int NC>
void gram_launch(int cls, unsigned n, hipStream_t st, const double *psi, const sd_cut_blk *blks, const int64_t *segs,
                 const sd_cut_item *items, double *ws) {
  const dim3 grid(n), block(256);
  if (cls == 0) hipLaunchKernelGGL((k_cut_gram<NC, SD_CUT_ACROSS, SD_CUT_SMALL_TILE>), grid, block, 0, st, psi, blks, segs, items, ws);
  else if (cls == 1) hipLaunchKernelGGL((k_cut_gram<NC, SD_CUT_ACROSS, SD_CUT_TILE>), grid, block, 0, st, psi, blks, segs, items, ws);
  else if (cls == 2) hipLaunchKernelGGL((k_cut_gram<NC, SD_CUT_INSIDE, SD_CUT_SMALL_TILE>), grid, block, 0, st, psi, blks, segs, items, ws);
  else hipLaunchKernelGGL((k_cut_gram<NC, SD_CUT_INSIDE, SD_CUT_TILE>), grid, block, 0, st, psi, blks, segs, items, ws);
}

size_t round16(size_t x) { return (x + 15) & ~(size_t)15; }

}  // namespace

int sd_launch_cut_gram(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi, const sd_cut_plan &plan, double *G_dev, float *kernel_ms) {
  if (kernel_ms) *kernel_ms = 0.0f;
  if (!m->dev_ready) return sd_set_err(ctx, SD_EARG, "model has no device tables (created without a context)");
  if (dtype != SD_F64 && dtype != SD_C128) return sd_set_err(ctx, SD_EARG, "dtype must be SD_F64 or SD_C128");
  if (m->nranks != 1) return sd_set_err(ctx, SD_EARG, "entanglement needs an unsharded model");
  const int nc = dtype == SD_C128 ? 2 : 1;
  if (plan.items.empty() || plan.n_out == 0) return SD_OK;
  if (plan.items.size() > 0x7fffffffu || plan.pairs.size() > 0x7fffffffu) return sd_set_err(ctx, SD_EARG, "entanglement: the work list is too long for one grid");
  // one upload: [blocks | segment starts | items | pairs], each part 16-byte aligned
  const size_t b_bytes = round16(plan.blks.size() * sizeof(sd_cut_blk)), s_bytes = round16(plan.segs.size() * sizeof(int64_t));
  const size_t i_bytes = round16(plan.items.size() * sizeof(sd_cut_item)), p_bytes = round16(plan.pairs.size() * sizeof(sd_cut_pair));
  std::vector<unsigned char> host(b_bytes + s_bytes + i_bytes + p_bytes);
  memcpy(host.data(), plan.blks.data(), plan.blks.size() * sizeof(sd_cut_blk));
  memcpy(host.data() + b_bytes, plan.segs.data(), plan.segs.size() * sizeof(int64_t));
  memcpy(host.data() + b_bytes + s_bytes, plan.items.data(), plan.items.size() * sizeof(sd_cut_item));
  memcpy(host.data() + b_bytes + s_bytes + i_bytes, plan.pairs.data(), plan.pairs.size() * sizeof(sd_cut_pair));
  PoolBlock tab, wsb;
  int rc = tab.take(ctx, host.size());
  if (rc) return rc;
  rc = wsb.take(ctx, (size_t)plan.ws_elems * nc * sizeof(double));
  if (rc) return rc;
  rc = sd_xfer_h2d(ctx, tab.p, host.data(), host.size());
  if (rc) return rc;
  const unsigned char *base = (const unsigned char *)tab.p;
  const sd_cut_blk *blks_dev = (const sd_cut_blk *)base;
  const int64_t *segs_dev = (const int64_t *)(base + b_bytes);
  const sd_cut_item *items_dev = (const sd_cut_item *)(base + b_bytes + s_bytes);
  const sd_cut_pair *pairs_dev = (const sd_cut_pair *)(base + b_bytes + s_bytes + i_bytes);
  double *ws = (double *)wsb.p;
  const double *v = (const double *)psi;
  if (kernel_ms) SD_HIP(ctx, hipEventRecord(ctx->ev0, ctx->stream));
  for (int cls = 0; cls < 4; ++cls) {
    const int64_t i0 = plan.class_first[cls], n = plan.class_first[cls + 1] - i0;
    if (n == 0) continue;
    if (nc == 2) gram_launch<2>(cls, (unsigned)n, ctx->stream, v, blks_dev, segs_dev, items_dev + i0, ws);
    else gram_launch<1>(cls, (unsigned)n, ctx->stream, v, blks_dev, segs_dev, items_dev + i0, ws);
  }
  const dim3 rgrid((unsigned)plan.pairs.size());
  if (nc == 2) hipLaunchKernelGGL(k_cut_reduce<2>, rgrid, dim3(256), 0, ctx->stream, blks_dev, pairs_dev, ws, G_dev);
  else hipLaunchKernelGGL(k_cut_reduce<1>, rgrid, dim3(256), 0, ctx->stream, blks_dev, pairs_dev, ws, G_dev);
  SD_HIP(ctx, hipGetLastError());
  if (kernel_ms) SD_HIP(ctx, hipEventRecord(ctx->ev1, ctx->stream));
  SD_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (kernel_ms) SD_HIP(ctx, hipEventElapsedTime(kernel_ms, ctx->ev0, ctx->ev1));
  return SD_OK;
}
