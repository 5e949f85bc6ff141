// S^-_q and S^+_q between adjacent magnetisation sectors (the transverse structure factor, DESIGN.md "Transverse S(q,w)").
//
//   (S^-_q psi)[s'] = L^(-1/2) sum_{r : bit r of s' = 0} e^{iqr} psi[rank_src(s' | 1 << r)]      (source sector nup' + 1)
//   (S^+_q psi)[s'] = L^(-1/2) sum_{r : bit r of s' = 1} e^{iqr} psi[rank_src(s' & ~(1 << r))]   (source sector nup' - 1)
//
// Gather form over the TARGET rows, one fixed order per row: r = 0 .. L-1 ascending, acc.re += c_r x.re - s_r x.im,
// acc.im += c_r x.im + s_r x.re (every product and sum rounded on its own: the library builds with -ffp-contract=off), then
// out = (nf acc.re, nf acc.im) with nf = 1/sqrt(L).  A real psi enters with x.im = 0.  The result is always ComplexF64.
//
// Tiled target (p >= 0).  The combinadic order puts the low sites first, so in BOTH sectors the rows that share their first p
// sites are contiguous and ordered like the (L-p)-site sub-basis.  A target tile (prefix P, suffix filling t') then finds
//   prefix site r < p : its partners at rows base_src(P ^ bit r) + i, the same suffix index i -- one coalesced stream;
//   suffix site r >= p: its partner in the ONE source tile with prefix P and filling t' -+ 1, at suffix rank suf_rank[sigma ^ bit]
//                       (the rank table holds every sigma of 2^LS, whatever its filling), read through L2.
// base_src is the prefix part of the source sector's closed-form rank: it needs the target's split p only, never the
// source model's plan (the two sectors may plan different p).  Prefix sites are the low sites, so "prefix terms, then suffix
// terms" is the ascending site order.
#include <hip/hip_runtime.h>

#include <cmath>

#include "device_common.hpp"

using namespace sd_dev;

namespace {

struct SpmPhases { double c[SD_MAX_L + 1], s[SD_MAX_L + 1]; };

template <int NCIN>
__device__ __forceinline__ void spm_term(const SpmPhases &ph, int r, const double *__restrict__ psi0, int64_t j, double &ar,
                                         double &ai) {
  double xr, xi;
  if (NCIN == 2) { const double2 v = reinterpret_cast<const double2 *>(psi0)[j]; xr = v.x; xi = v.y; }
  else { xr = psi0[j]; xi = 0.0; }
  const double c = ph.c[r], s = ph.s[r];
  ar += c * xr - s * xi;
  ai += c * xi + s * xr;
}

// rank in the sector (L, nup) of the first row whose low p sites are P: sum over the prefix sites k = 1..p that are down,
// while ups remain, of C(L - k, r_k - 1) (sd_internal.hpp, basis layout).  Wave-uniform when P is.
__device__ __forceinline__ int64_t prefix_base(const sd_dev_model &dm, int nup, uint32_t P, int p) {
  int64_t idx = 0;
  int r = nup;
  for (int k = 1; k <= p && r > 0; ++k) {
    if ((P >> (k - 1)) & 1u) --r;
    else idx += binom_g(dm, dm.L - k, r - 1);
  }
  return idx;
}

// the same rank for a whole configuration (per-row plans)
__device__ __forceinline__ int64_t rank_in(const sd_dev_model &dm, int nup, uint64_t s) {
  int64_t idx = 0;
  int r = nup;
  for (int k = 1; k <= dm.L && r > 0; ++k) {
    if ((s >> (k - 1)) & 1) --r;
    else idx += binom_g(dm, dm.L - k, r - 1);
  }
  return idx;
}

// One workgroup per target tile.  WANT: the value of bit r in the TARGET row that gives a term (0 for S^-, 1 for S^+).
// A thread carries RPT rows of the tile (i, i + 256, ...) through the site loop together, so each site issues RPT independent
// partner loads instead of one (each row's own sum still runs r = 0..L-1 in order).
#define SD_SPM_RPT 4
template <int NCIN, int WANT>
__global__ __launch_bounds__(256) void k_spm_tiled(sd_dev_model dd, int nup_src, SpmPhases ph, double nf,
                                                   const double *__restrict__ psi0, double2 *__restrict__ phi) {
  constexpr int RPT = SD_SPM_RPT;
  __shared__ int64_t pbase[32];                                   // p <= SD_MAX_PREFIX_BITS = 26
  const uint32_t P = dd.tile_prefix[blockIdx.x];
  const int64_t base = dd.tile_base[blockIdx.x];
  const int p = dd.p, L = dd.L;
  const int t2 = dd.nup - __popc(P);
  const int len = (int)binom_g(dd, dd.LS, t2);
  const uint16_t *__restrict__ sufS = dd.suf_states + dd.suf_off[t2];
  // partner tile of prefix site r: same suffix filling t' in the source sector, prefix P ^ bit r
  if ((int)threadIdx.x < p && ((P >> threadIdx.x) & 1u) == (uint32_t)WANT)
    pbase[threadIdx.x] = prefix_base(dd, nup_src, P ^ (1u << threadIdx.x), p);
  const int64_t sbase = prefix_base(dd, nup_src, P, p);            // source tile of the suffix terms: prefix P, filling t' -+ 1
  __syncthreads();
  for (int i0 = threadIdx.x; i0 < len; i0 += RPT * blockDim.x) {
    uint32_t sig[RPT];
    double ar[RPT], ai[RPT];
#pragma unroll
    for (int k = 0; k < RPT; ++k) {
      const int i = i0 + k * (int)blockDim.x;
      sig[k] = i < len ? (uint32_t)sufS[i] : 0u;
      ar[k] = 0.0; ai[k] = 0.0;
    }
    for (int r = 0; r < p; ++r)                                    // wave-uniform branch
      if (((P >> r) & 1u) == (uint32_t)WANT) {
#pragma unroll
        for (int k = 0; k < RPT; ++k) {
          const int i = i0 + k * (int)blockDim.x;
          if (i < len) spm_term<NCIN>(ph, r, psi0, pbase[r] + i, ar[k], ai[k]);
        }
      }
    for (int r = p; r < L; ++r) {
      const uint32_t b = 1u << (r - p);
#pragma unroll
      for (int k = 0; k < RPT; ++k) {
        const int i = i0 + k * (int)blockDim.x;
        if (i < len && ((sig[k] >> (r - p)) & 1u) == (uint32_t)WANT)
          spm_term<NCIN>(ph, r, psi0, sbase + dd.suf_rank[sig[k] ^ b], ar[k], ai[k]);
      }
    }
#pragma unroll
    for (int k = 0; k < RPT; ++k) {
      const int i = i0 + k * (int)blockDim.x;
      if (i < len) phi[base + i] = make_double2(nf * ar[k], nf * ai[k]);
    }
  }
}

// Full 2^L basis (idx = state): the partner of row s' is row s' ^ (1 << r); consecutive lanes hold consecutive rows.
template <int NCIN, int WANT>
__global__ __launch_bounds__(256) void k_spm_full(sd_dev_model dd, SpmPhases ph, double nf, const double *__restrict__ psi0,
                                                  double2 *__restrict__ phi) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < dd.N; idx += stride) {
    double ar = 0.0, ai = 0.0;
    for (int r = 0; r < dd.L; ++r)
      if (((idx >> r) & 1) == WANT) spm_term<NCIN>(ph, r, psi0, idx ^ ((int64_t)1 << r), ar, ai);
    phi[idx] = make_double2(nf * ar, nf * ai);
  }
}

// Per-row target plans (very dilute sectors, p < 0): unrank the target row, rank every partner in the source sector.
template <int NCIN, int WANT>
__global__ __launch_bounds__(256) void k_spm_rows(sd_dev_model dd, int nup_src, SpmPhases ph, double nf,
                                                  const double *__restrict__ psi0, double2 *__restrict__ phi) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < dd.N; idx += stride) {
    const uint64_t s = unrank_g(dd, idx);
    double ar = 0.0, ai = 0.0;
    for (int r = 0; r < dd.L; ++r)
      if ((int)((s >> r) & 1) == WANT) spm_term<NCIN>(ph, r, psi0, rank_in(dd, nup_src, s ^ ((uint64_t)1 << r)), ar, ai);
    phi[idx] = make_double2(nf * ar, nf * ai);
  }
}

template <int NCIN, int WANT>
void launch_spm(sd_ctx *ctx, const sd_model *src, const sd_model *dst, const SpmPhases &ph, double nf, const double *psi0,
                double2 *phi) {
  const sd_dev_model &dd = dst->dm;
  if (dst->nup >= 0 && dst->p >= 0) {
    hipLaunchKernelGGL((k_spm_tiled<NCIN, WANT>), dim3((unsigned)dd.n_tiles), dim3(256), 0, ctx->stream, dd, src->nup, ph, nf,
                       psi0, phi);
    return;
  }
  int64_t nb = (dd.N + 255) / 256;
  if (nb > (1 << 20)) nb = 1 << 20;
  if (dst->nup < 0)
    hipLaunchKernelGGL((k_spm_full<NCIN, WANT>), dim3((unsigned)nb), dim3(256), 0, ctx->stream, dd, ph, nf, psi0, phi);
  else
    hipLaunchKernelGGL((k_spm_rows<NCIN, WANT>), dim3((unsigned)nb), dim3(256), 0, ctx->stream, dd, src->nup, ph, nf, psi0, phi);
}

}  // namespace

// phi (dst's rows, ComplexF64) = S^-_q psi0 (op SD_SPIN_MINUS) or S^+_q psi0 (SD_SPIN_PLUS), psi0 on src's rows.  The caller has
// checked that the two models are compatible (recur.cpp, spm_check).
int sd_launch_spm_q(sd_ctx *ctx, const sd_model *src, const sd_model *dst, int op, int dtype_in, const void *psi0, double q,
                    void *phi) {
  if (!src->dev_ready || !dst->dev_ready) return sd_set_err(ctx, SD_EARG, "model has no device tables (created without a context)");
  if (dtype_in != SD_F64 && dtype_in != SD_C128) return sd_set_err(ctx, SD_EARG, "dtype must be SD_F64 or SD_C128");
  if (op != SD_SPIN_MINUS && op != SD_SPIN_PLUS) return sd_set_err(ctx, SD_EARG, "op must be SD_SPIN_MINUS or SD_SPIN_PLUS");
  if (dst->N == 0) return SD_OK;
  if (dst->nup >= 0 && dst->p >= 0 && dst->dm.n_tiles == 0) return SD_OK;
  SpmPhases ph;
  // exp(i q r), r = 0..L-1, in double on the host (as Sz_q_vector: sd_launch_szq)
  for (int r = 0; r < dst->L; ++r) { const double x = q * (double)r; ph.c[r] = cos(x); ph.s[r] = sin(x); }
  const double nf = 1.0 / sqrt((double)dst->L);
  const double *x = (const double *)psi0;
  double2 *y = (double2 *)phi;
  const bool c = dtype_in == SD_C128;
  if (op == SD_SPIN_MINUS) { if (c) launch_spm<2, 0>(ctx, src, dst, ph, nf, x, y); else launch_spm<1, 0>(ctx, src, dst, ph, nf, x, y); }
  else { if (c) launch_spm<2, 1>(ctx, src, dst, ph, nf, x, y); else launch_spm<1, 1>(ctx, src, dst, ph, nf, x, y); }
  SD_HIP(ctx, hipGetLastError());
  return SD_OK;
}
