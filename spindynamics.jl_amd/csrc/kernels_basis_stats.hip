// S^z-basis statistics of one state: everything here reads the weights w_s = |psi_s|^2 of the rows in one streaming
// pass, no partner rows, nothing divided by <psi|psi>.
//   moments   : sum w, sum w ln w, max w with the lowest row that attains it, sum w^q for up to SD_MOMENT_MAX_Q exponents.  A plain
//               row stream (no configuration, hence no MODE), 16-byte loads for ComplexF64.
//   counting  : P[k][m] = sum_s w_s [popcount(s & mask_k) = m] for K masks.  Grid (mask chunk, row block), the chunk the FAST index as
//               in k_pairs, so the workgroups in flight together read the same rows.  A chunk holds consecutive masks whose reachable
//               bins fit SD_COUNT_LDS_BINS; every thread owns a private histogram in LDS, bins[bin * 256 + tid]: the bank is a function
//               of tid alone and the read-modify-write needs no atomic.  Rows and their configurations (MODE) by for_rows
//               (gather_common.hpp): 1 tile prefix + suffix table, 0 unrank_g, 2 the row.
//   snapshots : rows drawn from w / sum w.  Fixed chunks of SD_SAMPLE_CHUNK consecutive rows: chunk weights (one wave per chunk, fixed
//               order), a two-level sequential scan of them that is monotone non-decreasing, then per shot a binary search of the scan
//               and a walk of one chunk in row order.  Nothing depends on the tile plan.
// Sums: per thread, then per block in a fixed order, block partials in ctx->d_partials, a reduce kernel adds them in a fixed order.
// No atomics; grids capped and grid-strided; every row index is 64-bit.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "gather_common.hpp"
#include "randn.hpp"

using namespace sd_dev;

namespace {

#define SD_MOMENT_MAX_BLOCKS 1024   // row blocks of k_moments (256 rows per trip)
#define SD_MOMENT_ROW 12            // doubles of a block's partial row: sum w, sum w ln w, max w, its row, 8 x sum w^q
#define SD_COUNT_MAX_BLOCKS 1024    // row blocks of k_count (grid.y): tiles of a tiled plan, else blocks of 256 rows, capped here
#define SD_COUNT_LDS_BINS 36        // bins of a mask chunk: 36 x 256 threads x 8 B = 72 KiB per workgroup, two workgroups per CU
#define SD_SAMPLE_CHUNK 1024        // consecutive rows of a sampling chunk
#define SD_SAMPLE_MAX_BLOCKS 512    // workgroups of k_sample_chunk_sums: four waves each, one chunk per wave and trip
#define SD_SAMPLE_SEG 1024          // chunk weights of a scan segment
#define SD_SAMPLE_SHOT_BLOCKS 32    // workgroups (one wave each) of k_sample_shots: one shot per lane and trip

template <int NC>
__device__ __forceinline__ double weight_at(const double *__restrict__ psi, int64_t idx) {
  if (NC == 2) { const double2 v = ((const double2 *)psi)[idx]; return v.x * v.x + v.y * v.y; }
  const double v = psi[idx];
  return v * v;
}

// ---- moments ----
struct sd_qlist {
  int nq;
  int kind[SD_MOMENT_MAX_Q];     // 2, 3, 4: by multiplication; 0: pow
  double q[SD_MOMENT_MAX_Q];
};

// the larger of two (w, -row) pairs: a total order, so the result does not depend on the order of the comparisons
__device__ __forceinline__ void take_max(double &w, int64_t &row, double ow, int64_t orow) {
  if (ow > w || (ow == w && orow < row)) { w = ow; row = orow; }
}
// max over the block, valid in thread 0; redw / redr: 4 entries of LDS each
__device__ __forceinline__ void block_argmax(double &w, int64_t &row, double *redw, int64_t *redr) {
  for (int off = 32; off > 0; off >>= 1) {
    const double ow = __shfl_down(w, off, 64);
    const int64_t orow = (int64_t)__shfl_down((long long)row, off, 64);
    take_max(w, row, ow, orow);
  }
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (lane == 0) { redw[wv] = w; redr[wv] = row; }
  __syncthreads();
  if (threadIdx.x == 0)
    for (int k = 1; k < 4; ++k) take_max(w, row, redw[k], redr[k]);
}

template <int NC>
__global__ __launch_bounds__(256) void k_moments(const double *__restrict__ psi, int64_t n, sd_qlist ql, double *__restrict__ partials) {
  __shared__ double red[32];
  __shared__ double redw[4];
  __shared__ int64_t redr[4];
  double sw = 0.0, swl = 0.0, mw = -1.0, sq[SD_MOMENT_MAX_Q];
  int64_t mrow = INT64_MAX;
#pragma unroll
  for (int k = 0; k < SD_MOMENT_MAX_Q; ++k) sq[k] = 0.0;
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < n; idx += stride) {
    const double w = weight_at<NC>(psi, idx);
    sw += w;
    if (w > 0.0) swl += w * log(w);
    take_max(mw, mrow, w, idx);
    const double w2 = w * w;
#pragma unroll
    for (int k = 0; k < SD_MOMENT_MAX_Q; ++k) {
      if (k >= ql.nq) continue;
      const int kind = ql.kind[k];
      sq[k] += kind == 2 ? w2 : kind == 3 ? w2 * w : kind == 4 ? w2 * w2 : w > 0.0 ? pow(w, ql.q[k]) : 0.0;
    }
  }
  double *__restrict__ prow = partials + (size_t)blockIdx.x * SD_MOMENT_ROW;
  block_reduce2(sw, swl, red);
  if (threadIdx.x == 0) { prow[0] = sw; prow[1] = swl; }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < SD_MOMENT_MAX_Q; k += 2) {
    double a = sq[k], b = sq[k + 1];
    block_reduce2(a, b, red);
    if (threadIdx.x == 0) { prow[4 + k] = a; prow[5 + k] = b; }
    __syncthreads();
  }
  block_argmax(mw, mrow, redw, redr);
  if (threadIdx.x == 0) { prow[2] = mw; prow[3] = (double)mrow; }
}

// One block: the partial rows summed in a fixed order (256 strided sums per column, then block_reduce2), the maxima compared as
// (w, -row) pairs.  out: sum w, sum w ln w, max w, its row, 0, sum w^q for q of the list.
__global__ __launch_bounds__(256) void k_moments_reduce(const double *__restrict__ partials, int nblocks, int nq, double *__restrict__ out) {
  __shared__ double red[32];
  __shared__ double redw[4];
  __shared__ int64_t redr[4];
  double s[SD_MOMENT_ROW];
#pragma unroll
  for (int c = 0; c < SD_MOMENT_ROW; ++c) s[c] = 0.0;
  double mw = -1.0;
  int64_t mrow = INT64_MAX;
  for (int b = threadIdx.x; b < nblocks; b += 256) {
    const double *__restrict__ p = partials + (size_t)b * SD_MOMENT_ROW;
#pragma unroll
    for (int c = 0; c < SD_MOMENT_ROW; ++c)
      if (c != 2 && c != 3) s[c] += p[c];
    take_max(mw, mrow, p[2], (int64_t)p[3]);
  }
  block_reduce2(s[0], s[1], red);
  if (threadIdx.x == 0) { out[0] = s[0]; out[1] = s[1]; out[4] = 0.0; }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < SD_MOMENT_MAX_Q; k += 2) {
    block_reduce2(s[4 + k], s[5 + k], red);
    if (threadIdx.x == 0) {
      if (k < nq) out[5 + k] = s[4 + k];
      if (k + 1 < nq) out[6 + k] = s[5 + k];
    }
    __syncthreads();
  }
  block_argmax(mw, mrow, redw, redr);
  if (threadIdx.x == 0) { out[2] = mw; out[3] = (double)mrow; }
}

// ---- counting statistics ----
struct sd_cmask {
  uint64_t mask;
  int32_t mmin;      // lowest reachable popcount
  int32_t off;       // the mask's first bin among the bins of the whole list
};

// chunk_first[c] .. chunk_first[c + 1]: the masks of chunk c.  partials[(bin of the list) * gridDim.y + blockIdx.y].
template <int NC, int MODE>
__global__ __launch_bounds__(256) void k_count(sd_dev_model dm, const double *__restrict__ psi, const sd_cmask *__restrict__ cm,
                                               const int32_t *__restrict__ chunk_first, double *__restrict__ partials) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  double *bins = reinterpret_cast<double *>(smem);           // bins[bin * 256 + tid], bin < the chunk's bins
  const int m0 = chunk_first[blockIdx.x], m1 = chunk_first[blockIdx.x + 1];
  const int g0 = cm[m0].off;                                 // the chunk's first bin among the bins of the list
  const int cbins = chunk_first[gridDim.x + 1 + blockIdx.x]; // bins of this chunk (the host's second table, behind the first)
  double *mine = bins + threadIdx.x;
  for (int b = 0; b < cbins; ++b) mine[b * 256] = 0.0;
  auto row = [&](uint64_t s, int64_t idx) {
    const double w = weight_at<NC>(psi, idx);
    for (int k = m0; k < m1; ++k) {
      const sd_cmask c = cm[k];
      const int b = c.off - g0 + (__popcll(s & c.mask) - c.mmin);
      mine[b * 256] += w;
    }
  };
  for_rows<MODE>(dm, blockIdx.y, gridDim.y, row);
  __syncthreads();
  // wave v sums bins v, v + 4, ...: four columns per lane in thread order, then the lanes
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (int b = wv; b < cbins; b += 4) {
    const double *col = bins + b * 256 + lane;
    double a = ((col[0] + col[64]) + col[128]) + col[192];
    for (int off = 32; off > 0; off >>= 1) a += __shfl_down(a, off, 64);
    if (lane == 0) partials[(size_t)(g0 + b) * gridDim.y + blockIdx.y] = a;
  }
}

// Block g sums the row blocks of bin g of the list in a fixed order and files it at P[dst_idx[g]].
__global__ __launch_bounds__(256) void k_count_reduce(const double *__restrict__ partials, int nblocks, const int32_t *__restrict__ dst_idx,
                                                      double *__restrict__ P) {
  __shared__ double red[32];
  const double *__restrict__ p = partials + (size_t)blockIdx.x * nblocks;
  double a = 0.0, z = 0.0;
  for (int b = threadIdx.x; b < nblocks; b += 256) a += p[b];
  block_reduce2(a, z, red);
  if (threadIdx.x == 0) P[dst_idx[blockIdx.x]] = a;
}

template <int NC>
void count_launch(int mode, dim3 grid, size_t shmem, hipStream_t st, const sd_dev_model &dm, const double *psi, const sd_cmask *cm,
                  const int32_t *chunk_first, double *partials) {
  // a workgroup's histogram may exceed the 64 KiB a kernel gets without asking
  const int budget = SD_COUNT_LDS_BINS * 256 * (int)sizeof(double);
  sd_with_mode(mode, [&](auto M) {
    constexpr int MODE = decltype(M)::value;
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&k_count<NC, MODE>), hipFuncAttributeMaxDynamicSharedMemorySize, budget);
    hipLaunchKernelGGL((k_count<NC, MODE>), grid, dim3(256), shmem, st, dm, psi, cm, chunk_first, partials);
  });
}

// ---- snapshots ----
// cw[c] = weight of chunk c: one wave per chunk, lane l adds rows l, l + 64, ... of the chunk in that order, then the lanes
template <int NC>
__global__ __launch_bounds__(256) void k_sample_chunk_sums(const double *__restrict__ psi, int64_t n, int64_t nchunks,
                                                           double *__restrict__ cw) {
  const int lane = threadIdx.x & 63;
  const int64_t nwaves = (int64_t)gridDim.x * 4;
  for (int64_t c = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); c < nchunks; c += nwaves) {
    const int64_t base = c * SD_SAMPLE_CHUNK + lane;
    double a = 0.0;
#pragma unroll
    for (int j = 0; j < SD_SAMPLE_CHUNK / 64; ++j) {
      const int64_t r = base + 64 * j;
      a += r < n ? weight_at<NC>(psi, r) : 0.0;
    }
    for (int off = 32; off > 0; off >>= 1) a += __shfl_down(a, off, 64);
    if (lane == 0) cw[c] = a;
  }
}

// The scan, two levels, every sum sequential.  Segment g holds the chunk weights [g SEG, (g + 1) SEG).
//   tot[g]  = the segment's weights added in order from 0                                   (k_scan_totals, a thread per segment)
//   off[0]  = 0, off[g + 1] = off[g] + tot[g]                                               (k_scan_offsets, one thread)
//   cum[i]  = off[g] + (the segment's weights up to and including i, added in order from 0) (k_scan_write, a thread per segment)
// Monotone: a running sum of non-negative terms does not decrease, x -> fl(off + x) does not decrease either, and the last entry
// of segment g, fl(off[g] + tot[g]), is off[g + 1] itself, which the first entry of segment g + 1 is not below.
__global__ __launch_bounds__(256) void k_scan_totals(const double *__restrict__ cw, int64_t nchunks, int64_t nseg, double *__restrict__ tot) {
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < nseg; g += stride) {
    const int64_t i1 = min((g + 1) * SD_SAMPLE_SEG, nchunks);
    double a = 0.0;
    for (int64_t i = g * SD_SAMPLE_SEG; i < i1; ++i) a += cw[i];
    tot[g] = a;
  }
}
__global__ void k_scan_offsets(const double *__restrict__ tot, int64_t nseg, double *__restrict__ off) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  double a = 0.0;
  for (int64_t g = 0; g < nseg; ++g) { off[g] = a; a += tot[g]; }
  off[nseg] = a;
}
__global__ __launch_bounds__(256) void k_scan_write(double *cw, int64_t nchunks, int64_t nseg, const double *__restrict__ off) {
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < nseg; g += stride) {
    const int64_t i1 = min((g + 1) * SD_SAMPLE_SEG, nchunks);
    const double o = off[g];
    double a = 0.0;
    for (int64_t i = g * SD_SAMPLE_SEG; i < i1; ++i) { a += cw[i]; cw[i] = o + a; }
  }
}

// Shot k: t = u_k W; the first chunk whose cumulative weight exceeds t; then its rows in order, the running sum continued from the
// chunk before.  Rows of weight 0 are never returned: a walk that rounding lets run off the chunk's end returns the chunk's last
// row with w > 0, and a chunk without one (t at or past the last cumulative weight) hands over to the nearest such row before it.
template <int NC>
__global__ __launch_bounds__(64) void k_sample_shots(sd_dev_model dm, const double *__restrict__ psi, int64_t n,
                                                      const double *__restrict__ cum, int64_t nchunks, const double *__restrict__ Wp,
                                                      int64_t shots, uint64_t seed, int64_t *__restrict__ rows,
                                                      uint64_t *__restrict__ configs) {
  const double W = *Wp;
  const int64_t stride = (int64_t)gridDim.x * 64;
  for (int64_t k = (int64_t)blockIdx.x * 64 + threadIdx.x; k < shots; k += stride) {
    const double t = sd_sample_uniform(seed, (uint64_t)k) * W;
    int64_t lo = 0, hi = nchunks;
    while (lo < hi) {
      const int64_t mid = lo + ((hi - lo) >> 1);
      if (cum[mid] > t) hi = mid; else lo = mid + 1;
    }
    const int64_t c = lo < nchunks ? lo : nchunks - 1;
    const int64_t r0 = c * SD_SAMPLE_CHUNK, r1 = min(r0 + SD_SAMPLE_CHUNK, n);
    double run = c > 0 ? cum[c - 1] : 0.0;
    int64_t pick = -1, last = -1;
    for (int64_t r = r0; r < r1; ++r) {
      const double w = weight_at<NC>(psi, r);
      if (!(w > 0.0)) continue;
      last = r;
      run += w;
      if (run > t) { pick = r; break; }
    }
    if (pick < 0) pick = last;
    for (int64_t r = r0 - 1; pick < 0 && r >= 0; --r)
      if (weight_at<NC>(psi, r) > 0.0) pick = r;
    for (int64_t r = r1; pick < 0 && r < n; ++r)
      if (weight_at<NC>(psi, r) > 0.0) pick = r;
    if (pick < 0) pick = 0;                                  // unreachable with W > 0, which the launcher has checked
    rows[k] = pick;
    configs[k] = dm.nup < 0 ? (uint64_t)pick : unrank_g(dm, pick);
  }
}

struct PoolBlock {   // a block of the context's pool, given back when the launcher returns
  sd_ctx *ctx = nullptr;
  void *p = nullptr;
  size_t bytes = 0;
  ~PoolBlock() { if (p) sd_pool_give(ctx, p, bytes); }
  int take(sd_ctx *c, size_t want) { ctx = c; return sd_pool_take(c, want, &p, &bytes); }
};

int common_checks(sd_ctx *ctx, const sd_model *m, int dtype, const char *what) {
  if (!m->dev_ready) return sd_set_err(ctx, SD_EARG, "model has no device tables (created without a context)");
  if (dtype != SD_F64 && dtype != SD_C128) return sd_set_err(ctx, SD_EARG, "dtype must be SD_F64 or SD_C128");
  if (m->nranks != 1) return sd_set_err(ctx, SD_EARG, std::string(what) + " need an unsharded model");
  return SD_OK;
}

}  // namespace

int sd_counting_range_host(const sd_model *m, uint64_t mask, int *m_min, int *n_bins) {
  if (m->L < 64 && (mask >> m->L) != 0) return SD_EARG;
  const int a = __builtin_popcountll(mask);
  int lo = 0, hi = a;
  if (m->nup >= 0) { lo = std::max(0, m->nup - (m->L - a)); hi = std::min(a, m->nup); }
  *m_min = lo; *n_bins = hi - lo + 1;
  return SD_OK;
}

double sd_sample_uniform_host(uint64_t seed, uint64_t k) { return sd_sample_uniform(seed, k); }

// dst (device, 5 + nq doubles) = sum w, sum w ln w, max w, the lowest row that attains it, 0, sum w^q for the nq exponents of q_host
int sd_launch_basis_moments(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi, const double *q_host, int nq, double *dst) {
  int rc = common_checks(ctx, m, dtype, "basis moments");
  if (rc) return rc;
  if (nq < 0 || nq > SD_MOMENT_MAX_Q || (nq > 0 && !q_host)) return sd_set_err(ctx, SD_EARG, "basis moments: between 0 and SD_MOMENT_MAX_Q exponents");
  sd_qlist ql{};
  ql.nq = nq;
  for (int k = 0; k < nq; ++k) {
    const double q = q_host[k];
    if (!std::isfinite(q) || q <= 0.0 || q == 1.0)
      return sd_set_err(ctx, SD_EARG, "basis moments: every exponent must be finite, positive and not 1 (q = 1 is the Shannon term, always returned)");
    ql.q[k] = q;
    ql.kind[k] = q == 2.0 ? 2 : q == 3.0 ? 3 : q == 4.0 ? 4 : 0;
  }
  const int64_t n = m->dm.n_local;
  if (n == 0) {      // no rows: every sum is empty
    SD_HIP(ctx, hipMemsetAsync(dst, 0, (size_t)(5 + nq) * sizeof(double), ctx->stream));
    return SD_OK;
  }
  const unsigned nb = (unsigned)std::min<int64_t>((n + 255) / 256, SD_MOMENT_MAX_BLOCKS);
  rc = sd_ensure_partials(ctx, (size_t)nb * SD_MOMENT_ROW);
  if (rc) return rc;
  const double *v = (const double *)psi;
  if (dtype == SD_C128) hipLaunchKernelGGL(k_moments<2>, dim3(nb), dim3(256), 0, ctx->stream, v, n, ql, ctx->d_partials);
  else hipLaunchKernelGGL(k_moments<1>, dim3(nb), dim3(256), 0, ctx->stream, v, n, ql, ctx->d_partials);
  hipLaunchKernelGGL(k_moments_reduce, dim3(1), dim3(256), 0, ctx->stream, ctx->d_partials, (int)nb, nq, dst);
  SD_HIP(ctx, hipGetLastError());
  return SD_OK;
}

// P_dev (device, K (L + 1) doubles, every entry written) = the counting statistics of the K masks of masks_host.  Returns after the
// stream has drained: the tables go back to the context's pool.
int sd_launch_counting_statistics(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi, const uint64_t *masks_host, int K,
                                  double *P_dev) {
  int rc = common_checks(ctx, m, dtype, "counting statistics");
  if (rc) return rc;
  if (K < 1 || K > SD_COUNT_MAX_MASKS || !masks_host) return sd_set_err(ctx, SD_EARG, "counting statistics: between 1 and SD_COUNT_MAX_MASKS masks");
  const sd_dev_model &dm = m->dm;
  const int L = m->L;
  // the tables: masks with their reachable ranges, the chunks, and where every bin of the list goes in P
  std::vector<sd_cmask> cm((size_t)K);
  std::vector<int32_t> first{0}, cbins, dst_idx;
  int total = 0, in_chunk = 0;
  for (int k = 0; k < K; ++k) {
    int lo = 0, nbk = 0;
    if (sd_counting_range_host(m, masks_host[k], &lo, &nbk)) return sd_set_err(ctx, SD_EARG, "counting statistics: a mask has a bit at or above L");
    if (nbk > SD_COUNT_MAX_BINS) return sd_set_err(ctx, SD_EARG, "counting statistics: a mask reaches more than SD_COUNT_MAX_BINS values");
    if (in_chunk + nbk > SD_COUNT_LDS_BINS) { first.push_back(k); cbins.push_back(in_chunk); in_chunk = 0; }
    cm[(size_t)k] = sd_cmask{masks_host[k], lo, total};
    for (int b = 0; b < nbk; ++b) dst_idx.push_back(k * (L + 1) + lo + b);
    total += nbk; in_chunk += nbk;
  }
  first.push_back(K); cbins.push_back(in_chunk);
  const int nchunks = (int)cbins.size();
  SD_HIP(ctx, hipMemsetAsync(P_dev, 0, (size_t)K * (size_t)(L + 1) * sizeof(double), ctx->stream));   // the bins no configuration reaches
  if (dm.n_local == 0) return SD_OK;
  // one upload: [masks | chunk_first (nchunks + 1) then the chunks' bin counts (nchunks) | dst_idx]
  std::vector<int32_t> itab(first);
  itab.insert(itab.end(), cbins.begin(), cbins.end());
  itab.insert(itab.end(), dst_idx.begin(), dst_idx.end());
  const size_t cm_bytes = cm.size() * sizeof(sd_cmask), it_bytes = itab.size() * sizeof(int32_t);
  std::vector<unsigned char> host(cm_bytes + it_bytes);
  memcpy(host.data(), cm.data(), cm_bytes);
  memcpy(host.data() + cm_bytes, itab.data(), it_bytes);
  PoolBlock tab;
  rc = tab.take(ctx, host.size());
  if (rc) return rc;
  rc = sd_xfer_h2d(ctx, tab.p, host.data(), host.size());
  if (rc) return rc;
  const sd_cmask *cm_dev = (const sd_cmask *)tab.p;
  const int32_t *first_dev = (const int32_t *)((const unsigned char *)tab.p + cm_bytes);
  const int32_t *dst_dev = first_dev + (2 * nchunks + 1);
  const sd_gather_grid g = sd_gather_grid_of(m, SD_COUNT_MAX_BLOCKS, SD_COUNT_MAX_BLOCKS);
  const int mode = g.mode;
  const unsigned nb = g.nb;
  rc = sd_ensure_partials(ctx, (size_t)total * nb);
  if (rc) return rc;
  const size_t shmem = (size_t)*std::max_element(cbins.begin(), cbins.end()) * 256 * sizeof(double);
  const dim3 grid((unsigned)nchunks, nb);
  const double *v = (const double *)psi;
  if (dtype == SD_C128) count_launch<2>(mode, grid, shmem, ctx->stream, dm, v, cm_dev, first_dev, ctx->d_partials);
  else count_launch<1>(mode, grid, shmem, ctx->stream, dm, v, cm_dev, first_dev, ctx->d_partials);
  hipLaunchKernelGGL(k_count_reduce, dim3((unsigned)total), dim3(256), 0, ctx->stream, ctx->d_partials, (int)nb, dst_dev, P_dev);
  SD_HIP(ctx, hipGetLastError());
  SD_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return SD_OK;
}

// rows_dev / configs_dev (device, `shots` entries each) = the rows drawn from |psi|^2 / sum |psi|^2 and their configurations.
// SD_EZERO when the weights sum to zero.  Synchronises the stream (the sum is read on the host; the scan goes back to the pool).
int sd_launch_sample_configurations(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi, int64_t shots, uint64_t seed,
                                    int64_t *rows_dev, uint64_t *configs_dev) {
  int rc = common_checks(ctx, m, dtype, "snapshots");
  if (rc) return rc;
  if (shots < 0) return sd_set_err(ctx, SD_EARG, "snapshots: a negative number of shots");
  const sd_dev_model &dm = m->dm;
  const int64_t n = dm.n_local;
  if (n == 0) return sd_set_err(ctx, SD_EZERO, "snapshots: the state has zero norm");
  const int64_t nchunks = (n + SD_SAMPLE_CHUNK - 1) / SD_SAMPLE_CHUNK, nseg = (nchunks + SD_SAMPLE_SEG - 1) / SD_SAMPLE_SEG;
  PoolBlock scan;   // [cum (nchunks) | tot (nseg) | off (nseg + 1)]
  rc = scan.take(ctx, sizeof(double) * (size_t)(nchunks + 2 * nseg + 1));
  if (rc) return rc;
  double *cum = (double *)scan.p, *tot = cum + nchunks, *off = tot + nseg;
  const double *v = (const double *)psi;
  const unsigned nbc = (unsigned)std::min<int64_t>((nchunks + 3) / 4, SD_SAMPLE_MAX_BLOCKS);
  if (dtype == SD_C128) hipLaunchKernelGGL(k_sample_chunk_sums<2>, dim3(nbc), dim3(256), 0, ctx->stream, v, n, nchunks, cum);
  else hipLaunchKernelGGL(k_sample_chunk_sums<1>, dim3(nbc), dim3(256), 0, ctx->stream, v, n, nchunks, cum);
  const unsigned nbs = (unsigned)std::min<int64_t>((nseg + 255) / 256, 64);
  hipLaunchKernelGGL(k_scan_totals, dim3(nbs), dim3(256), 0, ctx->stream, cum, nchunks, nseg, tot);
  hipLaunchKernelGGL(k_scan_offsets, dim3(1), dim3(64), 0, ctx->stream, tot, nseg, off);
  hipLaunchKernelGGL(k_scan_write, dim3(nbs), dim3(256), 0, ctx->stream, cum, nchunks, nseg, off);
  SD_HIP(ctx, hipGetLastError());
  double W = 0.0;
  SD_HIP(ctx, hipMemcpyAsync(&W, off + nseg, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  SD_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (!(W > 0.0) || !std::isfinite(W)) return sd_set_err(ctx, SD_EZERO, "snapshots: the state has zero (or non-finite) norm");
  if (shots == 0) return SD_OK;
  const unsigned nbk = (unsigned)std::min<int64_t>((shots + 63) / 64, SD_SAMPLE_SHOT_BLOCKS);
  if (dtype == SD_C128)
    hipLaunchKernelGGL(k_sample_shots<2>, dim3(nbk), dim3(64), 0, ctx->stream, dm, v, n, cum, nchunks, off + nseg, shots, seed, rows_dev, configs_dev);
  else
    hipLaunchKernelGGL(k_sample_shots<1>, dim3(nbk), dim3(64), 0, ctx->stream, dm, v, n, cum, nchunks, off + nseg, shots, seed, rows_dev, configs_dev);
  SD_HIP(ctx, hipGetLastError());
  SD_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return SD_OK;
}
