// On-device recursions: the host logic of the reference's solvers with every
// N-vector living in HBM.  Each iteration is one apply kernel (with a fused
// epilogue where the recursion allows it) plus a few BLAS-1 kernels; only the
// scalars the host-side tridiagonal / Chebyshev algebra needs cross PCIe.
//
// In this file: what runs an operator loop -- Lanczos (extremal values, bounds, ground state, tridiagonal, eigenpairs), Krylov and
// Chebyshev evolution in real and imaginary time, KPM moments, S(q,w) by KPM and by Lanczos with the transverse and site-resolved
// forms, the typicality driver, driven evolution -- and `Op`, the operator they share.  The one-pass observables are in
// observe.cpp; the guard, the pool buffer and the staging of the caller's vectors are in host_calls.hpp.
//
// Reference functions followed (file:line under the reference repository):
//   lanczos_extremal        src/Lanczos.jl:27-84
//   estimate_energy_bounds  src/Lanczos.jl:255-271
//   lanczos_groundstate     src/Lanczos.jl:87-181
//   lanczos_tridiag         src/Lanczos.jl:196-246
//   krylov_time_evolve      src/TimeEvolution/Krylov.jl:136-192
//   chebyshev_time_evolve   src/TimeEvolution/Chebyshev.jl:61-124
//   compute_chebyshev_moments / kpm_sw / kpm_sqw   src/KPM_Sqw.jl:34-128,191-256
//   spectral_from_tridiagonal / lanczos_sqw        src/LanczosSqw.jl:18-80
#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <stdexcept>
#include <string>
#include <vector>

#include "host_calls.hpp"

namespace {

// The caller's operator (sd_ctx_set_apply_callback; the reference's `applyH!` argument): out <- H psi by the callback on the
// context's stream, then the recursion's fused step as one elementwise pass over out.
int user_op(sd_ctx *ctx, int dtype, double *out, const double *psi, int64_t n, int epi, const sd_epi_args &ea) {
  if (ctx->user_apply(ctx->user_apply_data, dtype, out, psi, n, (void *)ctx->stream))
    return sd_set_err(ctx, SD_ECOMM, "the apply callback returned an error");
  if (epi == SD_EPI_PLAIN && !ea.negate) return SD_OK;
  return sd_launch_epilogue_only(ctx, dtype, n, out, out, psi, epi, ea);
}
// out <- H psi for the entry points that run their own loop on an unsharded model
int plain_op(sd_ctx *ctx, const sd_model *m, int dtype, double *out, const double *psi) {
  sd_epi_args ea;
  ++ctx->n_applies;
  if (ctx->user_apply) return user_op(ctx, dtype, out, psi, m->n_local, SD_EPI_PLAIN, ea);
  return sd_launch_apply(ctx, m, dtype, out, psi, SD_EPI_PLAIN, ea);
}

// What a recursion needs from "the operator": the apply on this rank's rows (halo exchange included) and the sum of device
// scalars over the ranks.  Unsharded (comm == nullptr, nranks == 1) both reduce to the plain launch / nothing, so the same
// loops serve the single-GPU and the sharded entry points.
// the effective hopping list of one stage on the device (kernels_hop_drive.hip)
struct HopDev {
  int n = 0, complex_form = 0;
  const uint32_t *bits = nullptr;
  const double *xy = nullptr;
};

struct Op {
  sd_ctx *ctx = nullptr;
  const sd_model *m = nullptr;
  sd_comm *comm = nullptr;
  int64_t n = 0;             // rows of this rank (== N unsharded)
  DBuf halo, send;           // imported partner tiles / tiles packed for the peers (sharded plans; ComplexF64-sized)
  bool overlap = true;       // interior tiles run while the exchange is in flight
  bool use_callback = true;  // false: always the built-in operator (the operator-level entry sd_apply_sharded, which a caller's
                             // operator may itself call on a sharded model: include/spindyn.h, sd_ctx_set_apply_callback)
  const sd_drive_table *drive = nullptr;   // a diagonal drive on top of the operator (driven_evolve_core), or null
  const HopDev *hop = nullptr;             // a hopping drive on top of the operator (driven_hop_evolve_core), or null

  int init(sd_ctx *c, const sd_model *mm, sd_comm *cm) {
    if (!c) return SD_EARG;
    ctx = c; m = mm; comm = cm;
    if (!m || !m->dev_ready) return sd_set_err(ctx, SD_EARG, "model has no device tables");
    if (m->nranks != 1 && !comm) return sd_set_err(ctx, SD_EARG, "a sharded model needs a communicator (the unsharded entry points take an unsharded model)");
    if (comm && sd_comm_nranks(comm) != m->nranks) return sd_set_err(ctx, SD_EARG, "communicator size does not match the model's shard count");
    SD_HIP(ctx, hipSetDevice(ctx->device));
    n = m->n_local;
    if (m->nranks > 1) {
      RC(halo.alloc(ctx, 2 * std::max<int64_t>(m->n_halo, 1)));
      if (m->packed) RC(send.alloc(ctx, 2 * std::max<int64_t>(m->n_send, 1)));
    }
    return SD_OK;
  }
  // out = epilogue(H psi) on the owned rows.  Sharded: pack (cell mode), post the exchange, interior tiles, wait, boundary tiles.
  int apply(int dtype, double *out, const double *psi, int epi, sd_epi_args ea) {
    ++ctx->n_applies;
    if (drive || hop) return apply_driven(dtype, out, psi, epi, ea);
    if (use_callback && ctx->user_apply) return user_op(ctx, dtype, out, psi, n, epi, ea);
    if (m->nranks == 1) return sd_launch_apply(ctx, m, dtype, out, psi, epi, ea, 0);
    ea.halo = halo.p;
    const void *src = psi;
    if (m->packed) { RC(sd_launch_pack(ctx, m, dtype, psi, send.p)); src = send.p; }
    RC(sd_comm_exchange_start(ctx, comm, m, dtype, src, halo.p));
    if (overlap && m->n_interior > 0 && n > 0) {
      RC(sd_launch_apply(ctx, m, dtype, out, psi, epi, ea, 1));
      RC(sd_comm_exchange_wait(ctx, comm, m));
      return sd_launch_apply(ctx, m, dtype, out, psi, epi, ea, 2);
    }
    RC(sd_comm_exchange_wait(ctx, comm, m));
    return sd_launch_apply(ctx, m, dtype, out, psi, epi, ea, 0);
  }
  // out = epilogue((H0 + D) psi): H0 psi into out by the caller's operator or the built-in apply, then the drive pass with the
  // recursion's epilogue over out in place (kernels_drive.hip; with a hop table kernels_hop_drive.hip, which adds B psi in the same
  // pass).  Unsharded models.
  int apply_driven(int dtype, double *out, const double *psi, int epi, const sd_epi_args &ea) {
    if (m->nranks != 1) return sd_set_err(ctx, SD_EARG, hop ? "hopping drives need an unsharded model" : "diagonal drives need an unsharded model");
    if (use_callback && ctx->user_apply) {
      if (ctx->user_apply(ctx->user_apply_data, dtype, out, psi, n, (void *)ctx->stream))
        return sd_set_err(ctx, SD_ECOMM, "the apply callback returned an error");
    } else {
      RC(sd_launch_apply(ctx, m, dtype, out, psi, SD_EPI_PLAIN, sd_epi_args(), 0));
    }
    if (hop) return sd_launch_hop_drive_epilogue(ctx, m, dtype, out, out, psi, epi, ea, drive, hop->n, hop->complex_form, hop->bits, hop->xy);
    return sd_launch_drive_epilogue(ctx, m, dtype, out, out, psi, epi, ea, *drive);
  }
  // device scalars <- their sum over the ranks (in place, ordered on the context's stream)
  int reduce(double *dev, int count) { return sd_comm_allreduce_dev(ctx, comm, dev, count); }
};

double norm_dev(Op &op, const double *x, int64_t n, int *rc) {
  double v = 0.0;
  sd_ctx *ctx = op.ctx;
  *rc = sd_k_nrm2sq(ctx, x, n, 2);
  if (!*rc) *rc = op.reduce(ctx->d_scalars + 2, 1);
  if (!*rc) *rc = sd_read_scalars(ctx, 2, 1, &v);
  return std::sqrt(v);
}

// Every SD_BREAK_PEEK steps the queued recursions read back the betas filed so far (one small copy + one synchronisation)
// and stop queueing when one is below tol or not a number: the reference's break (src/Lanczos.jl:66-70, 228-231) is then
// at most SD_BREAK_PEEK - 1 discarded steps late instead of lanc_m - j.
constexpr int SD_BREAK_PEEK = 32;
int peek_breakdown(sd_ctx *ctx, const double *d_be, int count, double tol, std::vector<double> &buf, bool *broke) {
  buf.resize((size_t)count);
  SD_HIP(ctx, hipMemcpyAsync(buf.data(), d_be, sizeof(double) * (size_t)count, hipMemcpyDeviceToHost, ctx->stream));
  SD_HIP(ctx, hipStreamSynchronize(ctx->stream));
  *broke = false;
  for (int k = 0; k < count; ++k)
    if (!(std::fabs(buf[k]) >= tol)) { *broke = true; break; }
  return SD_OK;
}

// ---- Lanczos at launch-bound sizes: two launches per step, any number of start vectors per launch ----
// The un-reorthogonalised recursion of lanczos_extremal (form 0, src/Lanczos.jl:27-84) and lanczos_tridiag (form 1, :196-246)
// for Qb NORMALISED start vectors stored back to back in u0 (consumed): step j is one batched apply with the <u|Hu> epilogue,
// its per-tile pairs left unreduced, and one batched update pass that sums those pairs and the previous passes' |w|^2 pairs
// itself (k_lanczos_fold_p).  Nothing touches the host until the end.  alpha, beta: Qb rows of mm (beta[., mm-1] unused).
// Same arithmetic per element as the four-launch form; the reductions are summed in another (fixed) order.
// May the vectors of independent recursions on `op` share their launches (sd_epi_args::batch)?  sd_ctx_set_q_batch is on, the
// built-in operator on an unsharded tiled plan of at most 16384 tiles, vectors of at most 2^22 rows (launch-bound sizes).
bool launches_shareable(const Op &op) {
  const sd_model *m = op.m;
  return op.ctx->q_batch && m->nranks == 1 && !op.ctx->user_apply && !op.drive && !op.hop && m->p >= 0 && m->dm.n_singles <= 16384 && op.n <= ((int64_t)1 << 22);
}
bool lanczos_fused_ok(const Op &op, int Qb) {
  const sd_model *m = op.m;
  return m->nranks == 1 && !op.ctx->user_apply && !op.drive && !op.hop && m->p >= 0 && m->dm.n_singles <= 4096 && op.n <= ((int64_t)1 << 22) &&
         (int64_t)Qb * op.n * 16 * 3 <= ((int64_t)4 << 30);
}
int lanczos_fused(Op &op, int Qb, double *u0, int mm, int form, int negate, double tol, std::vector<double> &alpha,
                  std::vector<double> &beta) {
  sd_ctx *ctx = op.ctx;
  const int64_t N = op.n;
  const int nt = op.m->dm.n_singles, nbf = sd_k_lanczos_fold_blocks(N);
  DBuf wb, vp, ab, n2;
  RC(wb.alloc(ctx, 2 * N * Qb)); RC(vp.alloc(ctx, 2 * N * Qb));
  const int64_t srow = 2 * (int64_t)mm;                                  // per vector: alpha[mm] | beta[mm]
  RC(ab.alloc(ctx, srow * Qb)); RC(n2.alloc(ctx, 3 * 2 * (int64_t)nbf * Qb));
  SD_HIP(ctx, hipMemsetAsync(ab.p, 0, sizeof(double) * (size_t)(srow * Qb), ctx->stream));
  double *d_al = ab.p, *d_be = ab.p + mm;
  auto n2buf = [&](int j) { return n2.p + (size_t)(j % 3) * 2 * (size_t)nbf * Qb; };
  sd_epi_args ea; ea.negate = negate; ea.batch = Qb; ea.bstride = N; ea.no_reduce = 1;
  double *ucur = u0, *uprev = vp.p, *t = wb.p;
  std::vector<double> peek;
  for (int j = 1; j <= mm; ++j) {
    ctx->n_applies += Qb - 1;
    RC(op.apply(SD_C128, t, ucur, SD_EPI_DOT, ea));                      // per-tile pairs of <u|Hu> -> ctx->d_partials
    const double *n2c = j > 1 ? n2buf(j - 1) : nullptr, *n2p = j > 2 ? n2buf(j - 2) : nullptr;
    if (j == mm) {                                                       // alpha_m; no vector behind it
      RC(sd_k_lanczos_fold_scalars_p(ctx, Qb, form, ctx->d_partials, nt, n2c, nbf, d_al + (j - 1), j > 1 ? d_be + (j - 2) : nullptr, srow));
      break;
    }
    RC(sd_k_lanczos_fold_p(ctx, t, ucur, j > 1 ? uprev : nullptr, N, Qb, N, form, ctx->d_partials, nt, n2c, n2p, nbf, d_al + (j - 1),
                           j > 1 ? d_be + (j - 2) : nullptr, srow, n2buf(j), nbf));
    { double *old = uprev; uprev = ucur; ucur = t; t = old; }
    if (j % SD_BREAK_PEEK == 0 && j < mm - 1) {                          // stop queueing once EVERY vector has broken down
      peek.resize((size_t)(srow * Qb));
      RC(read_back(ctx, peek.data(), ab.p, sizeof(double) * peek.size()));
      bool all_broke = true;
      for (int q = 0; q < Qb && all_broke; ++q) {
        bool broke = false;
        for (int k = 0; k < j - 1; ++k) if (!(std::fabs(peek[(size_t)(srow * q) + mm + k]) >= tol)) { broke = true; break; }
        all_broke = broke;
      }
      if (all_broke) break;
    }
  }
  std::vector<double> host((size_t)(srow * Qb));
  RC(read_back(ctx, host.data(), ab.p, sizeof(double) * host.size()));
  alpha.assign((size_t)Qb * mm, 0.0); beta.assign((size_t)Qb * mm, 0.0);
  for (int q = 0; q < Qb; ++q)
    for (int k = 0; k < mm; ++k) { alpha[(size_t)q * mm + k] = host[(size_t)(srow * q) + k]; beta[(size_t)q * mm + k] = host[(size_t)(srow * q) + mm + k]; }
  return SD_OK;
}

// The un-reorthogonalised Lanczos coefficients of one NORMALISED start vector u0 (2n doubles, consumed), two live vectors:
// form 0 is lanczos_extremal's recursion (src/Lanczos.jl:27-84), form 1 lanczos_tridiag's (:196-246).  al, be: mm entries
// (be[mm-1] unused).  The caller applies the reference's break on beta_j < tol to them: the steps before it are unaffected by
// what was queued behind them, the rest is discarded.  last_always: the step of alpha_mm is queued even behind a breakdown seen
// on the way (:237-239 stands after lanczos_tridiag's loop), so the betas are not looked at once it is the only step left.
int lanczos_coeffs(Op &op, double *u0, int mm, int form, int negate, double tol, bool last_always, std::vector<double> &al,
                   std::vector<double> &be) {
  if (lanczos_fused_ok(op, 1)) return lanczos_fused(op, 1, u0, mm, form, negate, tol, al, be);   // launch-bound sizes: two launches per step
  // No host round trip inside the loop: alpha_j, beta_j stay on the device (the update pass reads them there and files them
  // into d_al / d_be): the recursion is queued at once and read back once.  The vectors stay un-normalised (u_{j+1} = w_j,
  // |w_j|^2 on the device): the update divides on the fly and the normalising pass of :227/:233 disappears (k_lanczos_fold).
  sd_ctx *ctx = op.ctx;
  const int64_t N = op.n;
  DBuf w, vc, ab;
  RC(w.alloc(ctx, 2 * N)); RC(vc.alloc(ctx, 2 * N)); RC(ab.alloc(ctx, 4 * (int64_t)mm + 2));
  double *d_al = ab.p, *d_be = ab.p + mm, *d_n2 = ab.p + 2 * (int64_t)mm;      // d_n2[2j]: |w_j|^2
  SD_HIP(ctx, hipMemsetAsync(ab.p, 0, sizeof(double) * (4 * (size_t)mm + 2), ctx->stream));
  sd_epi_args ea; ea.negate = negate;
  std::vector<double> peek;
  double *ucur = u0, *uprev = vc.p, *t = w.p;
  const double *n2c = nullptr, *n2p = nullptr;       // |ucur|^2, |uprev|^2 on the device; null: normalised
  for (int j = 1; j <= mm; ++j) {
    RC(op.apply(SD_C128, t, ucur, SD_EPI_DOT, ea));                        // :51 + :55 / :218-219 fused -> d_scalars[0]
    RC(op.reduce(ctx->d_scalars + 0, 2));
    if (j == mm) {                                                         // alpha_m; no vector behind it (:237-239)
      RC(sd_k_lanczos_fold_scalars(ctx, form, ctx->d_scalars + 0, n2c, d_al + (j - 1), j > 1 ? d_be + (j - 2) : nullptr));
      break;
    }
    double *n2o = d_n2 + 2 * (int64_t)j;
    RC(sd_k_lanczos_fold(ctx, t, ucur, j > 1 ? uprev : nullptr, N, form, ctx->d_scalars + 0, n2c, n2p, d_al + (j - 1),
                         j > 1 ? d_be + (j - 2) : nullptr, n2o));          // :58-65 / :222-227 (beta_{j-1} is filed by this pass)
    RC(op.reduce(n2o, 1));
    { double *old = uprev; uprev = ucur; ucur = t; t = old; }
    n2p = n2c; n2c = n2o;
    if (j % SD_BREAK_PEEK == 0 && j < (last_always ? mm - 1 : mm)) {       // bound the work queued behind a breakdown: look at the betas so far
      bool broke = false;
      RC(peek_breakdown(ctx, d_be, j - 1, tol, peek, &broke));
      if (broke && !last_always) break;
      if (broke) j = mm - 1;                                               // on to the step of alpha_mm
    }
  }
  std::vector<double> host(2 * (size_t)mm);
  RC(read_back(ctx, host.data(), ab.p, sizeof(double) * 2 * (size_t)mm));
  al.assign(host.begin(), host.begin() + mm); be.assign(host.begin() + mm, host.end());
  return SD_OK;
}

// the reference's break on beta_j < tol (src/Lanczos.jl:66-70) applied to the read-back coefficients, then the extremal
// eigenvalues of the tridiagonal matrix that is left (:80-83)
int extremal_from_coeffs(sd_ctx *ctx, int mm, double tol, const double *al, const double *be, double *lo, double *hi) {
  int actual = mm;
  for (int j = 1; j < mm; ++j)
    if (!(be[j - 1] >= tol)) { actual = j; break; }                        // :66-70
  std::vector<double> ev(actual);
  if (sd_symtridiag_eig(actual, al, be, ev.data(), nullptr))               // :80-83
    return sd_set_err(ctx, SD_EINTERNAL, "tridiagonal eigen-solver did not converge");
  *lo = ev[0]; *hi = ev[actual - 1];
  return SD_OK;
}

// start vector of this rank's rows: the caller's (host pointer, unsharded calls; device pointer, sharded calls) or the
// counter-based N(0,1) vector keyed by the GLOBAL element index -- the same state for every sharding
int start_vector_op(Op &op, double *d, const void *given, bool given_on_dev, int64_t doubles, uint64_t seed) {
  if (given) return given_on_dev ? d2d(op.ctx, d, (const double *)given, doubles) : h2d(op.ctx, d, given, doubles);
  if (op.m->nranks > 1) return sd_launch_fill_randn_local(op.ctx, op.m, SD_C128, d, seed);
  return sd_k_fill_randn(op.ctx, d, doubles, seed, 0);
}

// lanczos_extremal from the caller's start vector (host or device pointer) or, without one, the seeded random vector
int extremal_dev(Op &op, int lanc_m, double tol, const void *given, bool given_on_dev, uint64_t seed, int negate, double *emin,
                 double *emax) {
  sd_ctx *ctx = op.ctx;
  const int mm = (int)std::min<int64_t>(lanc_m, op.m->N);
  if (mm < 1) return sd_set_err(ctx, SD_EARG, "lanc_m must be >= 1");
  DBuf v; RC(v.alloc(ctx, 2 * op.n));
  RC(start_vector_op(op, v.p, given, given_on_dev, 2 * op.n, seed));
  int rc = 0;
  double nrm = norm_dev(op, v.p, 2 * op.n, &rc); RC(rc);
  RC(sd_k_scale_div(ctx, v.p, v.p, 2 * op.n, nrm));                        // :40
  std::vector<double> al, be;
  RC(lanczos_coeffs(op, v.p, mm, 0, negate, tol, false, al, be));
  return extremal_from_coeffs(ctx, mm, tol, al.data(), be.data(), emin, emax);
}

int moments_dev(Op &op, const double *phi, int M, double a, double b, double *mu) {
  // compute_chebyshev_moments  src/KPM_Sqw.jl:95-128  (phi: device, c128, this rank's rows, normalised by the caller)
  sd_ctx *ctx = op.ctx;
  const int64_t N = op.n;
  if (M < 2) return sd_set_err(ctx, SD_EARG, "kpm_m must be >= 2");
  DBuf b0, b1, b2;
  RC(b0.alloc(ctx, 2 * N)); RC(b1.alloc(ctx, 2 * N)); RC(b2.alloc(ctx, 2 * N));
  double s[2];
  for (int doubling = ctx->kpm_doubling ? 1 : 0; doubling >= 0; --doubling) {
    double *v_prev = b0.p, *v_curr = b1.p, *v_next = b2.p;
    RC(d2d(ctx, v_prev, phi, 2 * N));
    RC(sd_k_dot(ctx, 2, phi, v_prev, N, 4)); RC(op.reduce(ctx->d_scalars + 4, 2));
    RC(sd_read_scalars(ctx, 4, 2, s)); mu[0] = s[0];                                                // :103
    sd_epi_args ea; ea.a = a; ea.b = b;
    if (!doubling) {
      // the reference's recursion: one moment <phi|T_k phi> per apply
      ea.phi = phi;
      RC(op.apply(SD_C128, v_curr, v_prev, SD_EPI_RESCALE_DOT, ea));                                // :106-107
      RC(op.reduce(ctx->d_scalars + 0, 2));
      RC(sd_read_scalars(ctx, 0, 2, s)); mu[1] = s[0];
      for (int k = 2; k <= M - 1; ++k) {
        ea.prev = v_prev;
        RC(op.apply(SD_C128, v_next, v_curr, SD_EPI_KPM, ea));                                      // :111-117 fused
        RC(op.reduce(ctx->d_scalars + 0, 2));
        RC(sd_read_scalars(ctx, 0, 2, s));
        mu[k] = s[0];
        const double nv = std::sqrt(s[1]);
        if (nv > 1e3) RC(sd_k_scale_div(ctx, v_next, v_next, 2 * N, nv));                           // :118-121
        double *t = v_prev; v_prev = v_curr; v_curr = v_next; v_next = t;                           // :124
      }
      return SD_OK;
    }
    // Two moments per apply from the same vectors v_n = T_n(H~) phi (T_m T_n = (T_{m+n} + T_{|m-n|})/2, H~ Hermitian):
    //   mu_{2n}   = 2 <v_n|v_n>       - mu_0,      mu_{2n+1} = 2 Re<v_n|v_{n+1}> - mu_1.
    // Same moments as the reference's loop up to rounding (<= 1e-13 here), in half the applies and without re-reading phi.
    // If the reference's overflow guard (:118-121, |v| > 1e3: the bounds do not contain the spectrum) would fire, the
    // identity no longer mirrors what the reference computes, so the reference recursion is run instead.
    ea.phi = nullptr;                                           // epilogue: s0 = Re<v_curr|v_next>, s1 = |v_next|^2
    // every step is queued without a host round trip: step n files its two sums at d_sum[2n..2n+1]; one read-back at the end
    const int nsteps = M / 2;                                   // applies: v_1 .. v_nsteps
    DBuf sm; RC(sm.alloc(ctx, 2 * (int64_t)nsteps + 2));
    ea.sums_dst = sm.p;
    RC(op.apply(SD_C128, v_curr, v_prev, SD_EPI_RESCALE_DOT, ea));
    RC(op.reduce(sm.p, 2));
    for (int n = 1; n < nsteps; ++n) {
      ea.prev = v_prev; ea.sums_dst = sm.p + 2 * n;
      RC(op.apply(SD_C128, v_next, v_curr, SD_EPI_KPM, ea));                                        // v_{n+1}
      RC(op.reduce(sm.p + 2 * n, 2));
      double *t = v_prev; v_prev = v_curr; v_curr = v_next; v_next = t;
    }
    std::vector<double> hs(2 * (size_t)nsteps);
    RC(read_back(ctx, hs.data(), sm.p, sizeof(double) * 2 * (size_t)nsteps));
    bool guard = false;
    for (int k = 1; k <= nsteps; ++k) {                         // sums of step k: [Re<v_{k-1}|v_k>, |v_k|^2]
      const double s0 = hs[2 * (size_t)(k - 1)], s1 = hs[2 * (size_t)(k - 1) + 1];
      if (k == 1) mu[1] = s0;
      else if (2 * k - 1 <= M - 1) mu[2 * k - 1] = 2.0 * s0 - mu[1];
      if (2 * k <= M - 1) mu[2 * k] = 2.0 * s1 - mu[0];
      if (!(std::sqrt(s1) <= 1e3)) guard = true;
    }
    if (!guard) return SD_OK;
  }
  return SD_OK;
}

// compute_chebyshev_moments (src/KPM_Sqw.jl:95-128) for Qb normalised vectors AT ONCE: phi = Qb vectors of n elements stored
// back to back.  The reference threads over the momenta (src/KPM_Sqw.jl:218); where one vector cannot fill the chip (its own
// documented sizes: L = 16..20) a recursion step per momentum is a launch-bound 5-10 us whatever it computes, so the momenta's
// vectors share the launches instead: one batched apply + one batched reduction per step for all of them (sd_epi_args::batch).
// Every vector sees exactly the arithmetic of moments_dev -- same kernels per tile, same summation order -- so mu is
// bit-identical to the one-momentum-at-a-time loop.  ok[k] = 0: the reference's overflow guard (:118-121) would have fired for
// vector k; the caller reruns it through moments_dev.  Unsharded tiled plans only (the caller checks).
int moments_dev_batched(Op &op, const double *phi, int Qb, int M, double a, double b, double *mu /* Qb x M */, std::vector<char> &ok) {
  sd_ctx *ctx = op.ctx;
  const int64_t N = op.n;
  if (M < 2) return sd_set_err(ctx, SD_EARG, "kpm_m must be >= 2");
  ok.assign((size_t)Qb, 1);
  const bool doubling = ctx->kpm_doubling != 0;
  const int nsteps = doubling ? M / 2 : M - 1;                  // applies: v_1 .. v_nsteps
  DBuf b0, b1, b2, sm;
  RC(b0.alloc(ctx, 2 * N * Qb)); RC(b1.alloc(ctx, 2 * N * Qb)); RC(b2.alloc(ctx, 2 * N * Qb));
  RC(sm.alloc(ctx, (int64_t)Qb * (2 * (int64_t)nsteps + 2)));
  const int64_t srow = 2 * (int64_t)nsteps + 2;                  // per vector: [mu0, 0, (s0, s1) of step 1, 2, ...]
  double *v_prev = b0.p, *v_curr = b1.p, *v_next = b2.p;
  RC(d2d(ctx, v_prev, phi, 2 * N * Qb));
  for (int k = 0; k < Qb; ++k) RC(sd_k_dot_to(ctx, 2, phi + 2 * N * k, v_prev + 2 * N * k, N, sm.p + srow * k));     // :103
  sd_epi_args ea; ea.a = a; ea.b = b;
  ea.batch = Qb; ea.bstride = N; ea.sums_bstride = srow;
  ea.phi = doubling ? nullptr : phi;                            // doubling: s0 = Re<v_curr|v_next>; reference loop: Re<phi|v_next>
  ea.sums_dst = sm.p + 2;
  ctx->n_applies += Qb - 1;                                     // (Op::apply counts one)
  RC(op.apply(SD_C128, v_curr, v_prev, SD_EPI_RESCALE_DOT, ea));                                    // :106-107
  for (int n = 1; n < nsteps; ++n) {
    ea.prev = v_prev; ea.sums_dst = sm.p + 2 + 2 * n;
    ctx->n_applies += Qb - 1;
    RC(op.apply(SD_C128, v_next, v_curr, SD_EPI_KPM, ea));                                          // :111-117 fused
    double *t = v_prev; v_prev = v_curr; v_curr = v_next; v_next = t;                               // :124
  }
  std::vector<double> hs((size_t)Qb * (size_t)srow);
  RC(read_back(ctx, hs.data(), sm.p, sizeof(double) * hs.size()));
  for (int q = 0; q < Qb; ++q) {
    const double *h = hs.data() + (size_t)q * (size_t)srow;
    double *m = mu + (size_t)q * (size_t)M;
    m[0] = h[0];
    for (int k = 1; k <= nsteps; ++k) {                         // sums of step k: [s0, |v_k|^2]
      const double s0 = h[2 * (size_t)k], s1 = h[2 * (size_t)k + 1];
      if (doubling) {
        if (k == 1) m[1] = s0;
        else if (2 * k - 1 <= M - 1) m[2 * k - 1] = 2.0 * s0 - m[1];
        if (2 * k <= M - 1) m[2 * k] = 2.0 * s1 - m[0];
      } else {
        m[k] = s0;
      }
      if (!(std::sqrt(s1) <= 1e3)) ok[q] = 0;                   // the reference would have renormalised v_next here
    }
  }
  return SD_OK;
}

// the reference's break on beta_j < tol (src/Lanczos.jl:228-231; NaN counts as a break) applied to the read-back coefficients
void tridiag_trim(int mm, double tol, const double *al, const double *be, double *alpha, double *beta, int *m_eff_out) {
  int m_eff = mm;
  for (int j = 1; j <= mm - 1; ++j)
    if (!(be[j - 1] >= tol)) { m_eff = j; break; }
  for (int k = 0; k < mm; ++k) alpha[k] = k < m_eff ? al[k] : 0.0;
  for (int k = 0; k + 1 < mm; ++k) beta[k] = (m_eff < mm ? k < m_eff : k < mm - 1) ? be[k] : 0.0;
  *m_eff_out = m_eff;
}

// lanczos_tridiag (src/Lanczos.jl:196-246) on a normalised device vector (consumed)
int tridiag_dev(Op &op, double *vcur, int lanc_m, double tol, double *alpha, double *beta, int *m_eff_out) {
  const int mm = (int)std::min<int64_t>(lanc_m, op.m->N);
  std::vector<double> al, be;
  RC(lanczos_coeffs(op, vcur, mm, 1, 0, tol, true, al, be));
  tridiag_trim(mm, tol, al.data(), be.data(), alpha, beta, m_eff_out);
  return SD_OK;
}

}  // namespace

// --------------------------------------------------------------------------
// host numerics shared with the C ABI
// --------------------------------------------------------------------------

// Implicit-QL symmetric tridiagonal eigen-solver (stands in for LAPACK's
// eigvals/eigen(SymTridiagonal) at src/Lanczos.jl:80-83,164-165,
// src/TimeEvolution/Krylov.jl:175-176, src/LanczosSqw.jl:23-24).
extern "C" int sd_symtridiag_eig(int n, const double *d_in, const double *e_in, double *w, double *z) {
  if (n <= 0 || !d_in || !w) return SD_EARG;
  std::vector<double> d(d_in, d_in + n), e(n, 0.0);
  for (int i = 0; i + 1 < n; ++i) e[i] = e_in[i];
  if (z) { std::fill(z, z + (size_t)n * n, 0.0); for (int i = 0; i < n; ++i) z[i + (size_t)n * i] = 1.0; }
  const double eps = 2.220446049250313e-16;
  for (int l = 0; l < n; ++l) {
    int iter = 0, mm;
    do {
      for (mm = l; mm < n - 1; ++mm)
        if (std::fabs(e[mm]) <= eps * (std::fabs(d[mm]) + std::fabs(d[mm + 1]))) break;
      if (mm != l) {
        if (iter++ == 300) return SD_EINTERNAL;
        double g = (d[l + 1] - d[l]) / (2.0 * e[l]);
        double r = std::hypot(g, 1.0);
        g = d[mm] - d[l] + e[l] / (g + std::copysign(r, g));
        double s = 1.0, c = 1.0, pp = 0.0;
        int i;
        bool underflow = false;
        for (i = mm - 1; i >= l; --i) {
          double f = s * e[i], b = c * e[i];
          r = std::hypot(f, g);
          e[i + 1] = r;
          if (r == 0.0) { d[i + 1] -= pp; e[mm] = 0.0; underflow = true; break; }
          s = f / r; c = g / r;
          g = d[i + 1] - pp;
          r = (d[i] - g) * s + 2.0 * c * b;
          pp = s * r;
          d[i + 1] = g + pp;
          g = c * r - b;
          if (z)
            for (int k = 0; k < n; ++k) {
              double *zi = z + (size_t)n * i, *zi1 = z + (size_t)n * (i + 1);
              const double f2 = zi1[k];
              zi1[k] = s * zi[k] + c * f2;
              zi[k] = c * zi[k] - s * f2;
            }
        }
        if (underflow) continue;
        d[l] -= pp; e[l] = g; e[mm] = 0.0;
      }
    } while (mm != l);
  }
  std::vector<int> order(n);
  for (int i = 0; i < n; ++i) order[i] = i;
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return d[a] < d[b]; });
  std::vector<double> zc;
  if (z) zc.assign(z, z + (size_t)n * n);
  for (int k = 0; k < n; ++k) {
    w[k] = d[order[k]];
    if (z) std::memcpy(z + (size_t)n * k, zc.data() + (size_t)n * order[k], sizeof(double) * n);
  }
  return SD_OK;
}

namespace {

// One real-time Chebyshev step takes |a dt| up to this: a million terms, a million applies.
constexpr double SD_CHEB_ZMAX = 1e6;

// J[k] = J_k(z) for k = 0 .. ktop, 0 <= z <= SD_CHEB_ZMAX, all orders from ONE backward recurrence (Miller):
// f_{k-1} = (2k/z) f_k - f_{k+1} from f_{ktop+1} = 0, f_ktop = 1, normalised by the sum rule J_0 + 2 sum_{k>=1} J_2k = 1.  For
// k > z, J_k is the recurrence's minimal solution and the downward direction damps every error; for k < z it is neutrally
// stable, J and Y of one size, so that roundings add up at most linearly: 1e6 steps of 2^-64 stay below 1e-13 of the amplitude
// sqrt(2/(pi z)) ~ 8e-4 there, far under an ulp of 1.  The start ktop = z + 64 + 24 z^(1/3) is 30 Airy widths (z/2)^(1/3) past the
// turning point k = z, where J_k(z) ~ Ai((2/z)^(1/3) (k - z)) (2/z)^(1/3) < e^-100 J_z (64 orders do the same for z < 1); the
// start's error is that ratio squared.  Orders above ktop are below 1e-100 and are given as zero.  The values grow by that
// ratio on the way down and are rescaled before they can overflow (z << 1, where the ratio per step is 2k/z).  Extended
// precision on the host, as scaled_bessel_i: the rounded values are the Bessel functions to an ulp of 1.
// std::cyl_bessel_j cannot serve: libstdc++ switches to a Hankel form above z = 1000 that is invalid for k ~ z (overflow, NaN),
// loses three digits below, throws for z < 0, and costs O(k) per order.
void bessel_j_all(double z, std::vector<long double> &J) {
  if (z == 0.0) { J.assign(1, 1.0L); return; }
  const int ktop = (int)std::ceil(z) + 64 + (int)std::ceil(24.0 * std::cbrt(z));
  const long double zl = (long double)z;
  J.assign((size_t)ktop + 2, 0.0L);
  J[ktop] = 1.0L;
  for (int k = ktop; k >= 1; --k) {
    const long double f = (long double)(2 * k) / zl * J[k] - J[k + 1];
    J[k - 1] = f;
    if (std::fabs(f) > 0x1p+8000L)
      for (int j = k - 1; j <= ktop; ++j) J[j] *= 0x1p-8000L;
  }
  long double S = 0.0L;
  for (int k = ktop - (ktop & 1); k >= 2; k -= 2) S += J[k];
  S = 2.0L * S + J[0];
  J.resize((size_t)ktop + 1);
  for (long double &x : J) x /= S;
}

// real-time term count: the first k with k > z and |J_k(z)| < 2^-53, z = |a dt| <= SD_CHEB_ZMAX.  Read off the recurrence's own
// values, which reach 14 Airy widths past the point where the rule is met (at z = 1e5 that is k = 100479, at 1e6 1001015),
// so the search needs no cap.
int cheb_auto_terms(double z) {
  std::vector<long double> J;
  bessel_j_all(z, J);
  int k = (int)std::floor(z) + 1;
  while (k < (int)J.size() && !(std::fabs(J[k]) < 0x1p-53L)) ++k;
  return k;
}

}  // namespace

// c_k = (2 - delta_k0) * (-i)^k * J_k(a dt) * exp(-i b dt)   (src/TimeEvolution/Chebyshev.jl:74-79), k = 0 .. cheb_n - 1.
// J_k(a dt) is the Bessel function of the Float64 product a * dt rounded once from extended precision (bessel_j_all), for
// |a dt| <= 1e6 at any cheb_n; a dt < 0 (backward in time) through J_k(-z) = (-1)^k J_k(z), which makes c(-dt) the conjugate of
// c(dt) bit for bit.  cos and sin of the Float64 product b * dt.  SD_EARG: cheb_n < 1, c NULL, a, b or dt not finite, |a dt| > 1e6.
extern "C" int sd_chebyshev_coeffs(int cheb_n, double a, double b, double dt, double *c) {
  if (cheb_n < 1 || !c) return SD_EARG;
  if (!std::isfinite(a) || !std::isfinite(b) || !std::isfinite(dt)) return SD_EARG;
  const double z = a * dt;
  if (!(std::fabs(z) <= SD_CHEB_ZMAX)) return SD_EARG;
  try {
    std::vector<long double> Jz;
    bessel_j_all(std::fabs(z), Jz);
    const double ph = b * dt, pr = std::cos(ph), pi = -std::sin(ph);
    for (int k = 0; k < cheb_n; ++k) {
      const double f = (k == 0) ? 1.0 : 2.0;
      double J = (size_t)k < Jz.size() ? (double)Jz[k] : 0.0;
      if (z < 0.0 && (k & 1)) J = -J;
      double xr, xi;
      switch (k & 3) {
        case 0: xr = f; xi = 0; break;
        case 1: xr = 0; xi = -f; break;
        case 2: xr = -f; xi = 0; break;
        default: xr = 0; xi = f; break;
      }
      xr *= J; xi *= J;
      c[2 * k] = xr * pr - xi * pi;
      c[2 * k + 1] = xr * pi + xi * pr;
    }
  } catch (...) { return SD_ENOMEM; }
  return SD_OK;
}

extern "C" int sd_chebyshev_terms(double z, int *n_terms) {
  if (!n_terms || !(std::fabs(z) <= SD_CHEB_ZMAX)) return SD_EARG;
  try { *n_terms = cheb_auto_terms(std::fabs(z)); } catch (...) { return SD_ENOMEM; }
  return SD_OK;
}

extern "C" int sd_kpm_kernel(int M, int kernel, double *g) {
  if (M < 1 || !g) return SD_EARG;
  const double PI = 3.14159265358979323846;
  for (int n = 0; n < M; ++n) g[n] = 1.0;
  if (kernel == SD_KERNEL_JACKSON) {
    for (int n = 0; n < M; ++n)
      g[n] = ((M - n + 1) * std::cos(PI * n / (M + 1)) + std::sin(PI * n / (M + 1)) * (1.0 / std::tan(PI / (M + 1)))) / (M + 1);
  } else if (kernel == SD_KERNEL_LORENTZ) {
    const double lam = 3.0;
    for (int n = 0; n < M; ++n) g[n] = std::sinh(lam * (1 - (double)n / M)) / std::sinh(lam);
  }
  return SD_OK;
}

extern "C" int sd_kpm_rescaling_from_bounds(double Emin, double Emax, double *a, double *b) {
  if (!a || !b) return SD_EARG;
  *a = (Emax - Emin) / (2 * 0.99);
  *b = (Emax + Emin) / 2;
  return SD_OK;
}

extern "C" int sd_kpm_reconstruct(const double *mu, int kpm_m, const double *omega, int W, double a, double b,
                                  double E0, double *S) {
  if (kpm_m < 1 || W < 0 || !mu || !S) return SD_EARG;
  const double PI = 3.14159265358979323846;
  std::vector<double> T(std::max(kpm_m, 2));
  for (int iw = 0; iw < W; ++iw) {
    const double x = (omega[iw] + E0 - b) / a;                       // src/KPM_Sqw.jl:61
    if (std::fabs(x) >= 1.0) { S[iw] = 0.0; continue; }
    T[0] = 1.0;
    if (kpm_m >= 2) T[1] = x;
    for (int n = 2; n < kpm_m; ++n) T[n] = 2.0 * x * T[n - 1] - T[n - 2];
    double sum_val = mu[0] * T[0];
    for (int n = 1; n < kpm_m; ++n) sum_val += 2.0 * mu[n] * T[n];
    const double denom = PI * std::sqrt(1.0 - x * x);
    const double v = sum_val / (a * denom);
    S[iw] = v > 0.0 ? v : 0.0;
  }
  return SD_OK;
}

extern "C" int sd_spectral_from_tridiagonal(const double *alpha, const double *beta, int mt, double norm_phi, double E0,
                                            const double *omega, int W, double eta, int broaden, double *S) {
  if (mt < 1 || !alpha || !S) return SD_EARG;
  if (broaden != SD_BROADEN_LORENTZ && broaden != SD_BROADEN_GAUSS) return SD_EARG;
  const double PI = 3.14159265358979323846;
  std::vector<double> th(mt), Q((size_t)mt * mt);
  int rc = sd_symtridiag_eig(mt, alpha, beta, th.data(), Q.data());
  if (rc) return rc;
  for (int iw = 0; iw < W; ++iw) {
    double s = 0.0;
    for (int k = 0; k < mt; ++k) {
      const double q1 = Q[(size_t)mt * k];
      const double wgt = q1 * q1 * (norm_phi * norm_phi);
      const double sh = omega[iw] - (th[k] - E0);
      const double f = broaden == SD_BROADEN_LORENTZ ? (1 / PI) * (eta / (sh * sh + eta * eta))
                                                     : (1 / (std::sqrt(2 * PI) * eta)) * std::exp(-(sh * sh) / (2 * eta * eta));
      s += f * wgt;
    }
    S[iw] = s;
  }
  return SD_OK;
}

// --------------------------------------------------------------------------
// recursion-level C ABI
// --------------------------------------------------------------------------

// Every entry point exists in two forms sharing one core: the unsharded form (host vectors in / out, comm == nullptr) and
// the sharded form (this rank's rows as device vectors, a communicator).
static int energy_bounds_core(Op &op, int lanc_m, const void *psi0_a, const void *psi0_b, bool on_dev, uint64_t seed,
                              double *Emin, double *Emax) {
  sd_ctx *ctx = op.ctx;
  double lo, hi;
  if (lanczos_fused_ok(op, 2)) {
    // launch-bound sizes: the run on H (:258) and the run on -H (:261-267) are independent recursions -- one batch of two vectors,
    // the second with the negated operator (bit 1 of the epilogue's negate mask); each sees the arithmetic of a run of its own
    const int64_t N = op.n;
    const int mm = (int)std::min<int64_t>(lanc_m, op.m->N);
    if (mm < 1) return sd_set_err(ctx, SD_EARG, "lanc_m must be >= 1");
    DBuf v; RC(v.alloc(ctx, 4 * N));
    RC(start_vector_op(op, v.p, psi0_a, on_dev, 2 * N, seed));
    RC(start_vector_op(op, v.p + 2 * N, psi0_b, on_dev, 2 * N, seed + 0x9E3779B97F4A7C15ULL));
    int rc = 0;
    for (int k = 0; k < 2; ++k) {
      const double nrm = norm_dev(op, v.p + 2 * N * k, 2 * N, &rc); RC(rc);
      RC(sd_k_scale_div(ctx, v.p + 2 * N * k, v.p + 2 * N * k, 2 * N, nrm));            // :40
    }
    std::vector<double> al, be;
    RC(lanczos_fused(op, 2, v.p, mm, 0, /*negate mask: vector 1*/ 2, 1e-12, al, be));
    RC(extremal_from_coeffs(ctx, mm, 1e-12, al.data(), be.data(), &lo, &hi));
    *Emax = hi;
    RC(extremal_from_coeffs(ctx, mm, 1e-12, al.data() + mm, be.data() + mm, &lo, &hi));
    *Emin = -hi;
    return SD_OK;
  }
  RC(extremal_dev(op, lanc_m, 1e-12, psi0_a, on_dev, seed, 0, &lo, &hi));                            // src/Lanczos.jl:258
  *Emax = hi;
  RC(extremal_dev(op, lanc_m, 1e-12, psi0_b, on_dev, seed + 0x9E3779B97F4A7C15ULL, 1, &lo, &hi));   // :261-267
  *Emin = -hi;
  return SD_OK;
}

extern "C" int sd_lanczos_extremal(sd_ctx *ctx, const sd_model *m, int lanc_m, double tol, const void *psi0,
                                   uint64_t seed, int negate, double *emin, double *emax) { return abi_guard(ctx, [&]() -> int {
  Op op; RC(op.init(ctx, m, nullptr));
  if (!emin || !emax) return sd_set_err(ctx, SD_EARG, "null output");
  return extremal_dev(op, lanc_m, tol, psi0, false, seed, negate, emin, emax);
}); }

extern "C" int sd_lanczos_extremal_sharded(sd_ctx *ctx, const sd_model *m, sd_comm *comm, int lanc_m, double tol, const void *psi0_dev,
                                           uint64_t seed, int negate, double *emin, double *emax) { return abi_guard(ctx, [&]() -> int {
  Op op; RC(op.init(ctx, m, comm));
  if (!emin || !emax) return sd_set_err(ctx, SD_EARG, "null output");
  return extremal_dev(op, lanc_m, tol, psi0_dev, true, seed, negate, emin, emax);
}); }

extern "C" int sd_energy_bounds(sd_ctx *ctx, const sd_model *m, int lanc_m, const void *psi0_a, const void *psi0_b,
                                uint64_t seed, double *Emin, double *Emax) { return abi_guard(ctx, [&]() -> int {
  Op op; RC(op.init(ctx, m, nullptr));
  if (!Emin || !Emax) return sd_set_err(ctx, SD_EARG, "null output");
  return energy_bounds_core(op, lanc_m, psi0_a, psi0_b, false, seed, Emin, Emax);
}); }

extern "C" int sd_energy_bounds_sharded(sd_ctx *ctx, const sd_model *m, sd_comm *comm, int lanc_m, uint64_t seed,
                                        double *Emin, double *Emax) { return abi_guard(ctx, [&]() -> int {
  Op op; RC(op.init(ctx, m, comm));
  if (!Emin || !Emax) return sd_set_err(ctx, SD_EARG, "null output");
  return energy_bounds_core(op, lanc_m, nullptr, nullptr, true, seed, Emin, Emax);
}); }

extern "C" int sd_apply_sharded(sd_ctx *ctx, const sd_model *m, sd_comm *comm, int dtype, void *out_dev, const void *psi_dev,
                                int64_t n_local, int overlap) { return abi_guard(ctx, [&]() -> int {
  if (!ctx) return SD_EARG;
  if (!m || !out_dev || !psi_dev) return sd_set_err(ctx, SD_EARG, "null argument");
  if (dtype != SD_F64 && dtype != SD_C128) return sd_set_err(ctx, SD_EARG, "dtype must be SD_F64 or SD_C128");
  if (out_dev == psi_dev) return sd_set_err(ctx, SD_EARG, "out must not alias psi");
  Op op; RC(op.init(ctx, m, comm));
  if (n_local != op.n) return sd_set_err(ctx, SD_EDIM, "vector length does not match the local basis dimension");
  op.overlap = overlap != 0;
  op.use_callback = false;      // operator level: always the built-in H
  sd_epi_args ea;
  RC(op.apply(dtype, (double *)out_dev, (const double *)psi_dev, SD_EPI_PLAIN, ea));
  SD_HIP(ctx, hipStreamSynchronize(ctx->stream));   // the halo / send buffers go back to the pool
  return SD_OK;
}); }

extern "C" int sd_dot_sharded(sd_ctx *ctx, sd_comm *comm, int dtype, const void *x, const void *y, int64_t n_local,
                              double *out2) { return abi_guard(ctx, [&]() -> int {
  if (!ctx) return SD_EARG;
  if (!x || !y || !out2 || n_local < 0) return sd_set_err(ctx, SD_EARG, "bad argument");
  if (dtype != SD_F64 && dtype != SD_C128) return sd_set_err(ctx, SD_EARG, "bad dtype");
  SD_HIP(ctx, hipSetDevice(ctx->device));
  RC(sd_k_dot(ctx, dtype == SD_C128 ? 2 : 1, (const double *)x, (const double *)y, n_local, 4));
  RC(sd_comm_allreduce_dev(ctx, comm, ctx->d_scalars + 4, 2));
  return sd_read_scalars(ctx, 4, 2, out2);
}); }

extern "C" int sd_lanczos_groundstate(sd_ctx *ctx, const sd_model *m, int lanc_m, double tol, double orth_tol, const double *psi0,
                                      uint64_t seed, double *E0, double *psi_gs, int *m_actual_out) { return abi_guard(ctx, [&]() -> int {
  Op op; RC(op.init(ctx, m, nullptr));
  if (!E0 || !psi_gs) return sd_set_err(ctx, SD_EARG, "null output");
  const int64_t N = m->N;
  const int mm = (int)std::min<int64_t>(lanc_m, N);
  if (mm < 1) return sd_set_err(ctx, SD_EARG, "lanc_m must be >= 1");
  DBuf V, w, tmp;
  RC(V.alloc(ctx, N * (int64_t)mm)); RC(w.alloc(ctx, N)); RC(tmp.alloc(ctx, N));
  if (psi0) RC(h2d(ctx, V.p, psi0, N));
  else RC(sd_k_fill_randn(ctx, V.p, N, seed, 0));
  int rc = 0;
  double nrm = norm_dev(op, V.p, N, &rc); RC(rc);
  RC(sd_k_scale_div(ctx, V.p, V.p, N, nrm));                                             // :100,105
  std::vector<double> alpha(mm, 0.0), beta(mm, 0.0);
  int m_actual = mm;
  // The reference's orthogonality check of step j (:142-153: dot(V[:,k], w/beta) for every k <= j) as the sequential loop
  // would run it: corrects w and beta[j-1] when a test fires; *broke = 1 on breakdown (beta < tol).  The tests between two
  // corrections all use the same w/beta, so they are taken in one pass (sd_k_mdot) and the first one that fires is handled
  // exactly as the reference's sequential loop would; the rest is tested again.
  auto check_and_correct = [&](int j, double *wj, double *scratch_vec, int *broke) -> int {
    double s[2];
    std::vector<double> chk(j);
    *broke = 0;
    for (int k = 1; k <= j;) {
      RC(sd_k_scale_div(ctx, scratch_vec, wj, N, beta[j - 1]));
      RC(sd_k_mdot(ctx, V.p + N * (int64_t)(k - 1), N, j - k + 1, scratch_vec, N, chk.data()));
      int hit = -1;
      for (int q = 0; q < j - k + 1 && hit < 0; ++q)
        if (std::fabs(chk[q]) > orth_tol) hit = k + q;
      if (hit < 0) break;
      double *vk = V.p + N * (int64_t)(hit - 1);
      RC(sd_k_dot(ctx, 1, vk, wj, N, 4)); RC(sd_read_scalars(ctx, 4, 1, s));
      RC(sd_k_sub2(ctx, wj, vk, nullptr, N, s[0], 0.0));
      beta[j - 1] = norm_dev(op, wj, N, &rc); RC(rc);
      if (beta[j - 1] < tol) { *broke = 1; break; }                                       // inner break only (:150)
      k = hit + 1;
    }
    return SD_OK;
  };
  if (ctx->gs_blocked && !ctx->user_apply && mm >= 2) {
    // Passes that sum their producer's partial lists themselves (kernels_blas1.hip, k_gs_*): a step is the apply, one launch per
    // block of 8 columns, the update and the normalising pass -- no reduction launches, alpha_j and beta_j stay on the device --
    // and the orthogonality check of step j rides along with the Gram-Schmidt passes of step j + 1 (they read the same columns;
    // w_j / beta_j is V[:,j+1] itself), which removes a sweep over all columns per step.  ONE host synchronisation per step, to
    // look at the check (and beta) of the step before.  The one hit the reference's check loop finds on EVERY step -- the v_{j-1}
    // component that :129 puts back after the re-orthogonalisation had removed it -- is repaired inside the
    // update (k_gs_correct: w -= dot(v_{j-1}, w) v_{j-1}, then beta_j = norm(w), as :147-148).  If a check still fires -- orthogonality
    // lost beyond orth_tol, which the full re-orthogonalisation does not let happen in practice -- the step before is run through
    // the reference's loop itself and the current step is redone.
    const int nb = sd_k_gs_blocks(N);
    const size_t lst = (size_t)nb * 8;
    DBuf w2, scr, lists, ab, chkd;
    RC(w2.alloc(ctx, N));
    RC(scr.alloc(ctx, (int64_t)((size_t)(mm / 8 + 4) * lst)));
    RC(lists.alloc(ctx, (int64_t)(4 * lst)));                      // alpha partials | |w|^2 partials of the two latest steps | the update's pair
    RC(ab.alloc(ctx, 2 * (int64_t)mm + 2)); RC(chkd.alloc(ctx, (int64_t)mm + 16));
    SD_HIP(ctx, hipMemsetAsync(ab.p, 0, sizeof(double) * (2 * (size_t)mm + 2), ctx->stream));
    double *d_al = ab.p, *d_be = ab.p + mm, *apart = lists.p;
    auto n2list = [&](int j) { return lists.p + lst * (size_t)(1 + (j & 1)); };
    std::vector<double> hchk(mm + 16), hb(2);
    bool deferred = true;                 // false for the redo of a step whose predecessor was just checked the sequential way
    int j = 1;
    while (j <= mm) {
      double *vj = V.p + N * (int64_t)(j - 1);
      double *t = (j & 1) ? w.p : w2.p, *wprev = (j & 1) ? w2.p : w.p;     // w_{j-1} stays intact while step j runs
      RC(plain_op(ctx, m, SD_F64, t, vj));                                                // :113
      const bool chk_now = deferred && j >= 2;
      RC(sd_k_gs_chain(ctx, t, V.p, N, j, N, chk_now ? vj : nullptr, scr.p, apart, chkd.p));   // :116-124 (+ the check of step j-1)
      RC(sd_k_gs_update(ctx, t, vj, j == 1 ? nullptr : V.p + N * (int64_t)(j - 2), N, apart, n2list(j - 1), d_al + (j - 1),
                        j == 1 ? nullptr : d_be + (j - 2), n2list(j), lists.p + 3 * lst));  // :127-129, the k = j-1 repair (:142-148), |w|^2
      if (j < mm) RC(sd_k_gs_scale(ctx, V.p + N * (int64_t)j, t, N, n2list(j), d_be + (j - 1)));   // :133, :155
      if (j >= 2) {
        // the step before: beta_{j-1} (breakdown, :136-139) and its orthogonality check (:142-153)
        if (chk_now) SD_HIP(ctx, hipMemcpyAsync(hchk.data(), chkd.p, sizeof(double) * (size_t)(j - 1), hipMemcpyDeviceToHost, ctx->stream));
        RC(read_back(ctx, hb.data(), d_be + (j - 2), sizeof(double)));
        if (deferred) beta[j - 2] = hb[0];
        if (!(beta[j - 2] >= tol)) { m_actual = j - 1; break; }                            // (NaN counts as a breakdown)
        bool fired = false;
        if (chk_now)
          for (int k = 0; k < j - 1 && !fired; ++k) fired = std::fabs(hchk[k]) > orth_tol;
        if (fired) {
          int broke = 0;
          RC(check_and_correct(j - 1, wprev, t, &broke));
          if (broke) { m_actual = j - 1; break; }
          RC(sd_k_scale_div(ctx, vj, wprev, N, beta[j - 2]));                              // :155 with the corrected w, beta
          // the device copy of |w_{j-1}|^2 (a one-entry list) and of beta_{j-1} follow the correction
          std::vector<double> one(lst, 0.0); one[0] = beta[j - 2] * beta[j - 2];
          SD_HIP(ctx, hipMemcpyAsync(n2list(j - 1), one.data(), sizeof(double) * lst, hipMemcpyHostToDevice, ctx->stream));
          SD_HIP(ctx, hipMemcpyAsync(d_be + (j - 2), &beta[j - 2], sizeof(double), hipMemcpyHostToDevice, ctx->stream));
          SD_HIP(ctx, hipStreamSynchronize(ctx->stream));
          deferred = false;
          continue;                                                                        // redo step j on the corrected v_j
        }
      }
      deferred = true;
      ++j;
    }
    std::vector<double> host(2 * (size_t)mm);
    RC(read_back(ctx, host.data(), ab.p, sizeof(double) * host.size()));
    for (int k = 0; k < m_actual; ++k) alpha[k] = host[k];
    for (int k = 0; k + 1 < m_actual; ++k) beta[k] = host[mm + k];
  } else
  for (int j = 1; j <= mm; ++j) {
    double *vj = V.p + N * (int64_t)(j - 1);
    RC(plain_op(ctx, m, SD_F64, w.p, vj));                                                // :113
    double s[2];
    // :116-124: w -= dot(V[:,k], w) V[:,k] for k = 1..j-1, then alpha_j = dot(V[:,j], w) -- one chain of fused
    // subtract-and-dot kernels whose scalars stay on the device; only alpha_j comes back to the host
    // (default: in blocks of 8 columns, classical Gram-Schmidt inside a block -- the coefficients differ from the sequential
    // chain's by O(eps * |coeff|), half the passes over memory; sd_ctx_set_gs_blocked(ctx, 0): the reference's column order)
    if (ctx->gs_blocked) RC(sd_k_bgs_chain(ctx, w.p, V.p, N, j, N, 4));
    else RC(sd_k_mgs_chain(ctx, w.p, V.p, N, j, N, 4));
    RC(sd_read_scalars(ctx, 4, 1, s));
    alpha[j - 1] = s[0];                                                                 // :124
    RC(sd_k_sub2(ctx, w.p, vj, j == 1 ? nullptr : V.p + N * (int64_t)(j - 2), N, alpha[j - 1],
                 j == 1 ? 0.0 : beta[j - 2]));                                           // :127-129
    if (j < mm) {
      beta[j - 1] = norm_dev(op, w.p, N, &rc); RC(rc);                                   // :133
      if (beta[j - 1] < tol) { m_actual = j; break; }                                    // :136-139
      int broke = 0;
      RC(check_and_correct(j, w.p, tmp.p, &broke));                                      // :142-153
      if (broke) m_actual = j;                                                           // inner break only (:150): the step goes on
      RC(sd_k_scale_div(ctx, V.p + N * (int64_t)j, w.p, N, beta[j - 1]));                 // :155
    }
  }
  std::vector<double> ev(m_actual), Z((size_t)m_actual * m_actual);
  if (sd_symtridiag_eig(m_actual, alpha.data(), beta.data(), ev.data(), Z.data()))       // :164-165
    return sd_set_err(ctx, SD_EINTERNAL, "tridiagonal eigen-solver did not converge");
  *E0 = ev[0];                                                                           // :167
  RC(sd_k_gemv_cols(ctx, w.p, V.p, N, m_actual, Z.data()));                              // :170 (first eigenvector = column 0)
  nrm = norm_dev(op, w.p, N, &rc); RC(rc);
  RC(sd_k_scale_div(ctx, w.p, w.p, N, nrm));                                             // :171
  RC(d2h(ctx, psi_gs, w.p, N));
  if (m_actual_out) *m_actual_out = m_actual;
  return SD_OK;
}); }

extern "C" int sd_lanczos_tridiag(sd_ctx *ctx, const sd_model *m, const void *v, int64_t n, int lanc_m, double tol,
                                  double *alpha, double *beta, int *m_eff, double *norm_v) { return abi_guard(ctx, [&]() -> int {
  Op op; RC(op.init(ctx, m, nullptr));
  if (n != m->N) return sd_set_err(ctx, SD_EDIM, "vector length does not match the basis dimension");
  if (!v || !alpha || !beta || !m_eff || !norm_v) return sd_set_err(ctx, SD_EARG, "null argument");
  if (lanc_m < 1) return sd_set_err(ctx, SD_EARG, "lanc_m must be >= 1");
  DBuf vc; RC(vc.alloc(ctx, 2 * n));
  RC(h2d(ctx, vc.p, v, 2 * n));
  int rc = 0;
  const double normv = norm_dev(op, vc.p, 2 * n, &rc); RC(rc);
  if (normv == 0) return sd_set_err(ctx, SD_EZERO, "starting vector has zero norm");     // :210-212
  RC(sd_k_scale_div(ctx, vc.p, vc.p, 2 * n, normv));
  *norm_v = normv;
  return tridiag_dev(op, vc.p, lanc_m, tol, alpha, beta, m_eff);
}); }

// krylov_time_evolve; on_dev: psi0 / psit are device vectors (psit ComplexF64; may alias a ComplexF64 psi0).
// log_norm != null: the imaginary-time form (the reference's krylov_imaginary_time_evolution,
// src/TimeEvolution/QuantumTypicality.jl:154-211) on the same Lanczos vectors -- exp(-dt theta_l) in place of the phase, one
// projection; psit = exp(-dt H) psi0 / |.| and *log_norm = ln |exp(-dt H) psi0| (the reference returns the un-normalised vector;
// the weights are formed as exp(-dt (theta_l - theta_min)) and dt theta_min goes into the logarithm, so nothing overflows).
static int krylov_evolve_core(Op &op, int dtype, const void *psi0, int64_t n, double dt, int kry_m, void *psit, bool on_dev,
                              double *log_norm = nullptr, double *min_beta = nullptr) {
  sd_ctx *ctx = op.ctx;
  if (!psi0 || !psit) return sd_set_err(ctx, SD_EARG, "null vector");
  auto emit = [&](const double *src) -> int {          // result to the caller
    if (!on_dev) return d2h(ctx, psit, src, 2 * n);
    RC(d2d(ctx, (double *)psit, src, 2 * n));
    SD_HIP(ctx, hipStreamSynchronize(ctx->stream));   // the work vectors go back to the pool: nothing may still use them
    return SD_OK;
  };
  if (n != op.n) return sd_set_err(ctx, SD_EDIM, "vector length does not match the (local) basis dimension");
  if (dtype != SD_F64 && dtype != SD_C128) return sd_set_err(ctx, SD_EARG, "bad dtype");
  if (kry_m < 1) return sd_set_err(ctx, SD_EARG, "kry_m must be >= 1");
  const int nc = dtype == SD_C128 ? 2 : 1;
  // all Krylov vectors are kept complex on the device; a real psi0 keeps exactly-zero imaginary parts
  std::vector<DBuf> V(kry_m);
  DevIn in;
  DBuf w;
  RC(w.alloc(ctx, 2 * n));
  RC(in.stage(ctx, dtype, psi0, on_dev, n));
  int rc = 0;
  const double norm0 = norm_dev(op, in.p, nc * n, &rc); RC(rc);
  RC(V[0].alloc(ctx, 2 * n));
  RC(sd_k_promote(ctx, V[0].p, in.p, nc, n));
  if (norm0 == 0) {                                                                       // :145-147
    if (log_norm) return sd_set_err(ctx, SD_EZERO, "starting vector has zero norm");
    return emit(V[0].p);
  }
  RC(sd_k_scale_div(ctx, V[0].p, V[0].p, 2 * n, norm0));                                  // :148
  // the Lanczos part is queued without host round trips (see lanczos_coeffs): alpha_j (complex) and beta_j stay on the device
  // and are read back once; the break on |beta_j| < 1e-14 (:162-168) is applied to the values afterwards
  // V[j] holds the un-normalised u_{j+1} = w_j (k_lanczos_fold): no normalising pass; the final combination divides its
  // coefficients by beta_j instead
  DBuf ab; RC(ab.alloc(ctx, 5 * (int64_t)kry_m + 2));
  double *d_al = ab.p, *d_be = ab.p + 2 * (int64_t)kry_m, *d_n2 = ab.p + 3 * (int64_t)kry_m;   // alpha as (re, im) pairs, beta, |w_j|^2 at [2j]
  SD_HIP(ctx, hipMemsetAsync(ab.p, 0, sizeof(double) * (5 * (size_t)kry_m + 2), ctx->stream));
  sd_epi_args ea;
  const double *n2c = nullptr, *n2p = nullptr;
  const bool fused = lanczos_fused_ok(op, 1);          // launch-bound sizes: two launches per step (see lanczos_fused)
  DBuf n2l;
  const int nt = op.m->dm.n_singles, nbf = sd_k_lanczos_fold_blocks(n);
  if (fused) { RC(n2l.alloc(ctx, 3 * 2 * (int64_t)nbf)); ea.no_reduce = 1; }
  auto n2buf = [&](int j) { return n2l.p + (size_t)(j % 3) * 2 * (size_t)nbf; };
  for (int j = 1; fused && j <= kry_m; ++j) {
    double *t = w.p;
    if (j < kry_m) { RC(V[j].alloc(ctx, 2 * n)); t = V[j].p; }
    RC(op.apply(SD_C128, t, V[j - 1].p, SD_EPI_DOT, ea));                                 // per-tile pairs of <u|Hu> (re, im) -> ctx->d_partials
    const double *pc = j > 1 ? n2buf(j - 1) : nullptr, *pp = j > 2 ? n2buf(j - 2) : nullptr;
    if (j == kry_m) {
      RC(sd_k_lanczos_fold_scalars_p(ctx, 1, 2, ctx->d_partials, nt, pc, nbf, d_al + 2 * (j - 1), j > 1 ? d_be + (j - 2) : nullptr, 0));
      break;
    }
    RC(sd_k_lanczos_fold_p(ctx, t, V[j - 1].p, j > 1 ? V[j - 2].p : nullptr, n, 1, n, 2, ctx->d_partials, nt, pc, pp, nbf,
                           d_al + 2 * (j - 1), j > 1 ? d_be + (j - 2) : nullptr, 0, n2buf(j), nbf));   // :156-161
  }
  for (int j = 1; !fused && j <= kry_m; ++j) {
    double *t = w.p;
    if (j < kry_m) { RC(V[j].alloc(ctx, 2 * n)); t = V[j].p; }
    RC(op.apply(SD_C128, t, V[j - 1].p, SD_EPI_DOT, ea));                                 // :153,155 -> d_scalars[0..1]
    RC(op.reduce(ctx->d_scalars + 0, 2));
    if (j == kry_m) {
      RC(sd_k_lanczos_fold_scalars(ctx, 2, ctx->d_scalars + 0, n2c, d_al + 2 * (j - 1), j > 1 ? d_be + (j - 2) : nullptr));
      break;
    }
    double *n2o = d_n2 + 2 * (int64_t)j;
    RC(sd_k_lanczos_fold(ctx, t, V[j - 1].p, j > 1 ? V[j - 2].p : nullptr, n, 2, ctx->d_scalars + 0, n2c, n2p,
                         d_al + 2 * (j - 1), j > 1 ? d_be + (j - 2) : nullptr, n2o));      // :156-161
    RC(op.reduce(n2o, 1));
    n2p = n2c; n2c = n2o;
  }
  std::vector<double> hostab(3 * (size_t)kry_m);
  RC(read_back(ctx, hostab.data(), ab.p, sizeof(double) * 3 * (size_t)kry_m));
  std::vector<double> alr(kry_m, 0.0), beta(kry_m, 0.0);
  int m_eff = kry_m;
  for (int j = 1; j <= kry_m; ++j) {
    alr[j - 1] = hostab[2 * (size_t)(j - 1)];
    if (j < kry_m) {
      beta[j - 1] = hostab[2 * (size_t)kry_m + (j - 1)];
      if (min_beta && !(std::fabs(beta[j - 1]) >= *min_beta)) *min_beta = std::fabs(beta[j - 1]);   // driven_evolve_core's record
      if (!(std::fabs(beta[j - 1]) >= 1e-14)) { m_eff = j; break; }                       // :162-168
    }
  }
  // reduced problem on the host (:175-182).  Deviation (documented in DESIGN.md): Re(alpha) enters a
  // symmetric tridiagonal solve instead of the reference's general complex eigen of the same matrix.
  std::vector<double> ev(m_eff), Q((size_t)m_eff * m_eff), yr(m_eff, 0.0), yi(m_eff, 0.0);
  if (sd_symtridiag_eig(m_eff, alr.data(), beta.data(), ev.data(), Q.data()))
    return sd_set_err(ctx, SD_EINTERNAL, "tridiagonal eigen-solver did not converge");
  for (int l = 0; l < m_eff; ++l) {
    const double ph = -ev[l] * dt;
    const double cr = log_norm ? std::exp(-(ev[l] - ev[0]) * dt) : std::cos(ph), ci = log_norm ? 0.0 : std::sin(ph);
    const double q0 = Q[(size_t)m_eff * l] * norm0;
    for (int k = 0; k < m_eff; ++k) {
      const double qk = Q[k + (size_t)m_eff * l];
      yr[k] += qk * cr * q0; yi[k] += qk * ci * q0;
    }
  }
  {                                                                                       // :185-188, one fused pass
    std::vector<const double *> cols(m_eff);
    for (int k = 0; k < m_eff; ++k) cols[k] = V[k].p;
    for (int k = 1; k < m_eff; ++k) { yr[k] /= beta[k - 1]; yi[k] /= beta[k - 1]; }     // V[k] = beta_k v_{k+1}
    RC(sd_k_ccombine(ctx, w.p, cols.data(), n, m_eff, yr.data(), yi.data()));
  }
  const double nn = norm_dev(op, w.p, 2 * n, &rc); RC(rc);
  if (log_norm) {
    if (!(nn > 0)) return sd_set_err(ctx, SD_EZERO, "the imaginary-time state has zero norm");
    *log_norm = std::log(nn) - ev[0] * dt;
  }
  RC(sd_k_scale_div(ctx, w.p, w.p, 2 * n, nn));                                           // :190
  return emit(w.p);
}

extern "C" int sd_krylov_evolve(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi0, int64_t n, double dt,
                                int kry_m, void *psit) { return abi_guard(ctx, [&]() -> int {
  Op op; RC(op.init(ctx, m, nullptr));
  return krylov_evolve_core(op, dtype, psi0, n, dt, kry_m, psit, false);
}); }

extern "C" int sd_krylov_evolve_dev(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi0_dev, int64_t n, double dt,
                                    int kry_m, void *psit_dev) { return abi_guard(ctx, [&]() -> int {
  Op op; RC(op.init(ctx, m, nullptr));
  return krylov_evolve_core(op, dtype, psi0_dev, n, dt, kry_m, psit_dev, true);
}); }

extern "C" int sd_krylov_evolve_sharded(sd_ctx *ctx, const sd_model *m, sd_comm *comm, int dtype, const void *psi0_dev,
                                        int64_t n_local, double dt, int kry_m, void *psit_dev) { return abi_guard(ctx, [&]() -> int {
  Op op; RC(op.init(ctx, m, comm));
  return krylov_evolve_core(op, dtype, psi0_dev, n_local, dt, kry_m, psit_dev, true);
}); }

// The Chebyshev term loop (src/TimeEvolution/Chebyshev.jl:93-121) for a coefficient array: pt = sum_{k < cheb_n} c_k T_k(H~) phi_0
// with H~ = (H - b)/a and c = cheb_n (re, im) pairs.  pprev holds phi_0 and is consumed, pcur / pnext are work vectors, pt must be
// none of them.  batch > 1: `batch` vectors stored n elements apart in every buffer share the launches (sd_epi_args::batch; the
// caller has checked that the plan allows it) -- each sees the arithmetic of a loop of its own.
static int cheb_terms(Op &op, double *pprev, double *pcur, double *pnext, double *pt, int64_t n, double a, double b, const double *c,
                      int cheb_n, int batch) {
  sd_ctx *ctx = op.ctx;
  sd_epi_args ea; ea.a = a; ea.b = b;
  if (batch > 1) { ea.batch = batch; ea.bstride = n; }
  const int64_t nb = n * batch;                     // the elementwise start runs over the whole batch at once
  ctx->n_applies += batch - 1;                      // (Op::apply counts one)
  RC(op.apply(SD_C128, pcur, pprev, SD_EPI_RESCALE, ea));                                 // :93
  RC(sd_k_cheb_init(ctx, pt, pprev, pcur, nb, c[0], c[1], cheb_n >= 2 ? c[2] : 0.0, cheb_n >= 2 ? c[3] : 0.0,
                    cheb_n >= 2));                                                        // :96-102
  // :110-121, one fused pass per term.  Terms are taken in pairs: the first of a pair only advances the recurrence, the
  // second adds both terms to psi_t in order (c_k phi_k is exact in the apply's input vector), so psi_t is read and
  // written once per two terms -- same bits as one accumulation per term, 72 instead of 80 B/row per term.
  int k = 2;
  ea.accv = pt;
  if ((cheb_n - 2) % 2 == 1) {
    ea.prev = pprev; ea.c_re = c[2 * k]; ea.c_im = c[2 * k + 1];
    ctx->n_applies += batch - 1;
    RC(op.apply(SD_C128, pnext, pcur, SD_EPI_CHEB, ea));
    double *t = pprev; pprev = pcur; pcur = pnext; pnext = t;
    ++k;
  }
  for (; k + 1 <= cheb_n - 1; k += 2) {
    ea.prev = pprev;
    ctx->n_applies += batch - 1;
    RC(op.apply(SD_C128, pnext, pcur, SD_EPI_RECUR, ea));                                 // phi_k
    { double *t = pprev; pprev = pcur; pcur = pnext; pnext = t; }
    ea.prev = pprev; ea.c0_re = c[2 * k]; ea.c0_im = c[2 * k + 1]; ea.c_re = c[2 * k + 2]; ea.c_im = c[2 * k + 3];
    ctx->n_applies += batch - 1;
    RC(op.apply(SD_C128, pnext, pcur, SD_EPI_CHEB2, ea));                                 // phi_{k+1}; psi_t += c_k phi_k + c_{k+1} phi_{k+1}
    { double *t = pprev; pprev = pcur; pcur = pnext; pnext = t; }
  }
  return SD_OK;
}

// chebyshev_time_evolve on device vectors: psi0_dev (c128, n elements) is read, psit_dev receives psi(t); they may be the
// same buffer (psi0 is copied into the recursion's own vectors first).  host_in / host_out select the host-pointer form.
static int chebyshev_evolve_core(Op &op, const void *psi0, bool host_in, int64_t n, double dt, int cheb_n,
                                 double Emin, double Emax, void *psit, bool host_out) {
  sd_ctx *ctx = op.ctx;
  if (!psi0 || !psit) return sd_set_err(ctx, SD_EARG, "null vector");
  if (n != op.n) return sd_set_err(ctx, SD_EDIM, "vector length does not match the (local) basis dimension");
  if (cheb_n < 1) return sd_set_err(ctx, SD_EARG, "cheb_n must be >= 1");               // :65
  const double a = (Emax - Emin) / (2 * 0.9999), b = (Emax + Emin) / 2;                   // :70-71
  if (!std::isfinite(a) || !std::isfinite(b) || !std::isfinite(dt)) return sd_set_err(ctx, SD_EARG, "the time step and the energy bounds must be finite");
  if (!(std::fabs(a * dt) <= SD_CHEB_ZMAX)) return sd_set_err(ctx, SD_EARG, "a * dt is too large for one Chebyshev step (above 1e6): take several steps");
  std::vector<double> c(2 * (size_t)cheb_n);
  RC(sd_chebyshev_coeffs(cheb_n, a, b, dt, c.data()));                                    // dt < 0 evolves backwards, as the reference's besselj does
  DBuf b0, b1, b2, ptb;
  RC(b0.alloc(ctx, 2 * n)); RC(b1.alloc(ctx, 2 * n)); RC(b2.alloc(ctx, 2 * n));
  double *pprev = b0.p, *pcur = b1.p, *pnext = b2.p;
  if (host_in) RC(h2d(ctx, pprev, psi0, 2 * n));                                          // :90
  else RC(d2d(ctx, pprev, (const double *)psi0, 2 * n));
  double *pt = (double *)psit;                    // psi_t accumulates in the caller's device buffer when there is one
  if (host_out) { RC(ptb.alloc(ctx, 2 * n)); pt = ptb.p; }
  RC(cheb_terms(op, pprev, pcur, pnext, pt, n, a, b, c.data(), cheb_n, 1));
  if (host_out) RC(d2h(ctx, psit, pt, 2 * n));
  else SD_HIP(ctx, hipStreamSynchronize(ctx->stream));   // the work vectors go back to the pool: nothing may still use them
  return SD_OK;
}

extern "C" int sd_chebyshev_evolve(sd_ctx *ctx, const sd_model *m, const void *psi0, int64_t n, double dt, int cheb_n,
                                   double Emin, double Emax, void *psit) { return abi_guard(ctx, [&]() -> int {
  Op op; RC(op.init(ctx, m, nullptr));
  return chebyshev_evolve_core(op, psi0, true, n, dt, cheb_n, Emin, Emax, psit, true);
}); }

extern "C" int sd_chebyshev_evolve_dev(sd_ctx *ctx, const sd_model *m, const void *psi0_dev, int64_t n, double dt, int cheb_n,
                                       double Emin, double Emax, void *psit_dev) { return abi_guard(ctx, [&]() -> int {
  Op op; RC(op.init(ctx, m, nullptr));
  return chebyshev_evolve_core(op, psi0_dev, false, n, dt, cheb_n, Emin, Emax, psit_dev, false);
}); }

extern "C" int sd_chebyshev_evolve_sharded(sd_ctx *ctx, const sd_model *m, sd_comm *comm, const void *psi0_dev, int64_t n_local,
                                           double dt, int cheb_n, double Emin, double Emax, void *psit_dev) { return abi_guard(ctx, [&]() -> int {
  Op op; RC(op.init(ctx, m, comm));
  return chebyshev_evolve_core(op, psi0_dev, false, n_local, dt, cheb_n, Emin, Emax, psit_dev, false);
}); }

extern "C" int sd_kpm_moments(sd_ctx *ctx, const sd_model *m, const void *phi, int64_t n, int M, double a, double b,
                              double *mu) { return abi_guard(ctx, [&]() -> int {
  Op op; RC(op.init(ctx, m, nullptr));
  if (n != m->N) return sd_set_err(ctx, SD_EDIM, "vector length does not match the basis dimension");
  if (!phi || !mu) return sd_set_err(ctx, SD_EARG, "null argument");
  DBuf ph; RC(ph.alloc(ctx, 2 * n));
  RC(h2d(ctx, ph.p, phi, 2 * n));
  return moments_dev(op, ph.p, M, a, b, mu);
}); }

extern "C" int sd_kpm_moments_sharded(sd_ctx *ctx, const sd_model *m, sd_comm *comm, const void *phi_dev, int64_t n_local,
                                      int M, double a, double b, double *mu) { return abi_guard(ctx, [&]() -> int {
  Op op; RC(op.init(ctx, m, comm));
  if (n_local != op.n) return sd_set_err(ctx, SD_EDIM, "vector length does not match the local basis dimension");
  if (!phi_dev || !mu) return sd_set_err(ctx, SD_EARG, "null argument");
  RC(moments_dev(op, (const double *)phi_dev, M, a, b, mu));
  SD_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return SD_OK;
}); }

namespace {
// H is real in the S^z basis, so for a real psi0 phi_{2pi-q} = conj(phi_q): the moments mu_n and the Lanczos coefficients
// alpha_j, beta_j of q and of 2pi - q agree, and so do the rows S(q, w).  same_as[j] = i < j when q[j] = 2 pi k - q[i] (to 8 ulp)
// and psi0 is real -- Float64, or ComplexF64 whose imaginary parts are all zero (counted on the device, summed over the ranks) --,
// else -1.  momenta(model) always holds both members of a pair; the reference recomputes the second row (src/KPM_Sqw.jl:218-252,
// src/LanczosSqw.jl:63-77), which differs from the copy by the rounding of exp(iqr) only.  Not with a caller's
// operator (it need not be real); sd_ctx_set_kpm_pair_q(ctx, 0) switches it off.
int pair_momenta(Op &op, int dtype, const double *psic, int64_t n, const double *q, int Qn, std::vector<int> &same_as) {
  sd_ctx *ctx = op.ctx;
  same_as.assign((size_t)std::max(Qn, 0), -1);
  if (!ctx->kpm_pair_q || ctx->user_apply || Qn < 2) return SD_OK;
  bool real_psi = dtype == SD_F64;
  if (!real_psi) {
    RC(sd_k_imag_count(ctx, psic, n, 6));
    RC(op.reduce(ctx->d_scalars + 6, 1));
    double cnt[1]; RC(sd_read_scalars(ctx, 6, 1, cnt));
    real_psi = cnt[0] == 0.0;
  }
  if (!real_psi) return SD_OK;
  const double two_pi = 6.283185307179586476925286766559;
  for (int j = 1; j < Qn; ++j)
    for (int i = 0; i < j; ++i) {
      if (same_as[i] >= 0) continue;
      const double sum = q[i] + q[j], k = std::nearbyint(sum / two_pi);
      const double tol = 8 * 2.220446049250313e-16 * std::max(two_pi, std::max(std::fabs(q[i]), std::fabs(q[j])));
      if (std::fabs(sum - k * two_pi) <= tol) { same_as[j] = i; break; }
    }
  return SD_OK;
}

// ---- S(q,w): kpm_sqw (src/KPM_Sqw.jl:191-256), lanczos_sqw (src/LanczosSqw.jl:47-80) and their transverse forms ----
// How one row S(q, .) is made from phi_q -- all that differs between the KPM and the Lanczos calls.  The recursion runs on
// `op`, the sector phi_q lives in; sqw_core below owns everything else.
struct Spectrum {
  Op &op;
  const double *omega; int W;
  double E0 = 0.0;
  bool batchable = true;
  Spectrum(Op &o, const double *om, int w) : op(o), omega(om), W(w) {}
  virtual int check() const = 0;                                           // the method's own arguments
  virtual int start(Op &os, const double *psic, double *scratch) = 0;      // E0 from psi0 (sector os; scratch: n elements), once per call
  virtual bool can_batch(int Qb) const = 0;                                // may Qb momenta share their launches?
  virtual int one(double *phi, double norm_phi, double *Srow) = 0;         // phi: normalised, consumed
  virtual int batch(double *phib, int Qk, const double *norms, double *const *rows) = 0;   // Qk normalised vectors back to back
};

struct KpmSpectrum : Spectrum {
  int have_ab; double a, b; int kpm_m, kernel; uint64_t seed;
  std::vector<double> mu, g;
  KpmSpectrum(Op &o, const double *om, int w, int have_ab_, double a_, double b_, int kpm_m_, int kernel_, uint64_t seed_)
      : Spectrum(o, om, w), have_ab(have_ab_), a(a_), b(b_), kpm_m(kpm_m_), kernel(kernel_), seed(seed_) {}
  int check() const override { return kpm_m < 2 ? sd_set_err(op.ctx, SD_EARG, "kpm_m must be >= 2") : SD_OK; }
  int start(Op &os, const double *psic, double *scratch) override {
    sd_ctx *ctx = os.ctx;
    sd_epi_args ea;
    double s[2];
    RC(os.apply(SD_C128, scratch, psic, SD_EPI_DOT, ea));                                   // :208-209 (only <psi0|H psi0> is kept)
    RC(os.reduce(ctx->d_scalars + 0, 2));
    RC(sd_read_scalars(ctx, 0, 2, s));
    E0 = s[0];
    if (!have_ab) {                                                                         // :212-214 (the recursion's sector)
      double Emin, Emax;
      RC(energy_bounds_core(op, 80, nullptr, nullptr, true, seed, &Emin, &Emax));
      sd_kpm_rescaling_from_bounds(Emin, Emax, &a, &b);
    }
    mu.resize(kpm_m); g.resize(kpm_m);
    sd_kpm_kernel(kpm_m, kernel, g.data());
    return SD_OK;
  }
  // Launch-bound sizes: the momenta's vectors share their launches (moments_dev_batched): five batches of vectors (phi + the
  // recursion's three + nothing else) within 4 GiB, vectors of at most 2^22 rows.  sd_ctx_set_q_batch(ctx, 0): one momentum at a time.
  bool can_batch(int Qb) const override {
    return batchable && Qb >= 2 && launches_shareable(op) && (int64_t)Qb * op.n * 16 * 4 <= ((int64_t)4 << 30);
  }
  void row(double *muk, double norm_phi, double *Srow) const {
    for (int k = 0; k < kpm_m; ++k) muk[k] *= g[k];                                         // :53
    sd_kpm_reconstruct(muk, kpm_m, omega, W, a, b, E0, Srow);
    const double n2 = norm_phi * norm_phi;
    for (int iw = 0; iw < W; ++iw) Srow[iw] *= n2;                                          // :252
  }
  int one(double *phi, double norm_phi, double *Srow) override {
    RC(moments_dev(op, phi, kpm_m, a, b, mu.data()));
    row(mu.data(), norm_phi, Srow);
    return SD_OK;
  }
  int batch(double *phib, int Qk, const double *norms, double *const *rows) override {
    std::vector<double> mub((size_t)Qk * (size_t)kpm_m);
    std::vector<char> okv;
    RC(moments_dev_batched(op, phib, Qk, kpm_m, a, b, mub.data(), okv));
    for (int k = 0; k < Qk; ++k) {
      double *muk = mub.data() + (size_t)k * (size_t)kpm_m;
      if (!okv[k]) RC(moments_dev(op, phib + 2 * op.n * k, kpm_m, a, b, muk));              // the guard fired: the reference's loop
      row(muk, norms[k], rows[k]);
    }
    return SD_OK;
  }
};

struct LanczosSpectrum : Spectrum {
  int lanc_m; double eta; int broaden, mm = 1;
  std::vector<double> alpha, beta;
  LanczosSpectrum(Op &o, const double *om, int w, int lanc_m_, double eta_, int broaden_)
      : Spectrum(o, om, w), lanc_m(lanc_m_), eta(eta_), broaden(broaden_) {}
  int check() const override {
    if (broaden != SD_BROADEN_LORENTZ && broaden != SD_BROADEN_GAUSS) return sd_set_err(op.ctx, SD_EARG, "unknown broadening");
    return lanc_m < 1 ? sd_set_err(op.ctx, SD_EARG, "lanc_m must be >= 1") : SD_OK;
  }
  int start(Op &os, const double *psic, double *scratch) override {
    sd_ctx *ctx = os.ctx;
    RC(plain_op(ctx, os.m, SD_C128, scratch, psic));                                        // src/LanczosSqw.jl:58
    // E0 = real(dot(conj(psi0c), tmp)) (sic, :59): dot conjugates its first argument again, so this is Re sum psi_i*tmp_i,
    // the product sum WITHOUT conjugation (equal to <psi|H|psi> for a real psi0).  Reduced on the device.
    RC(sd_k_dotu(ctx, psic, scratch, os.n, 4));
    double s[2]; RC(sd_read_scalars(ctx, 4, 2, s));
    E0 = s[0];
    mm = (int)std::max<int64_t>(std::min<int64_t>(lanc_m, op.n), 1);
    alpha.resize(mm); beta.resize(mm);
    return SD_OK;
  }
  // launch-bound sizes: all momenta in one recursion (src/LanczosSqw.jl:65 threads over them)
  bool can_batch(int Qb) const override { return batchable && op.ctx->q_batch && Qb >= 2 && lanczos_fused_ok(op, Qb); }
  int row(int m_eff, double norm_phi, double *Srow) const {
    int rs = sd_spectral_from_tridiagonal(alpha.data(), beta.data(), m_eff, norm_phi, E0, omega, W, eta, broaden, Srow);
    return rs ? sd_set_err(op.ctx, rs, "spectral_from_tridiagonal failed") : SD_OK;
  }
  int one(double *phi, double norm_phi, double *Srow) override {
    int m_eff = 0;
    RC(tridiag_dev(op, phi, lanc_m, 1e-12, alpha.data(), beta.data(), &m_eff));             // :73
    return row(m_eff, norm_phi, Srow);
  }
  int batch(double *phib, int Qk, const double *norms, double *const *rows) override {
    std::vector<double> al, be;
    RC(lanczos_fused(op, Qk, phib, mm, 1, 0, 1e-12, al, be));                               // :73
    for (int k = 0; k < Qk; ++k) {
      int m_eff = 0;
      tridiag_trim(mm, 1e-12, al.data() + (size_t)k * mm, be.data() + (size_t)k * mm, alpha.data(), beta.data(), &m_eff);
      RC(row(m_eff, norms[k], rows[k]));
    }
    return SD_OK;
  }
};

// The one S(q,w) driver.  psi0 (host vector, or device rows when on_dev) lives in the sector of `os`; make_phi(psic, q, out)
// writes phi_q = O_q psi0 (ComplexF64) into the sector of sp.op, where sp turns it into the row S(q, .) of Smat (Qn x W).
template <class MakePhi>
int sqw_core(Op &os, int dtype, const void *psi0, bool on_dev, int64_t n, const MakePhi &make_phi, Spectrum &sp, const double *q,
             int Qn, double *Smat) {
  sd_ctx *ctx = os.ctx;
  const int W = sp.W;
  const int64_t nd = sp.op.n;
  if (n != os.n) return sd_set_err(ctx, SD_EDIM, "psi0 length does not match the (local) basis dimension of its sector");
  if (dtype != SD_F64 && dtype != SD_C128) return sd_set_err(ctx, SD_EARG, "bad dtype");
  RC(sp.check());
  if (!psi0 || !Smat || (Qn > 0 && !q) || (W > 0 && !sp.omega)) return sd_set_err(ctx, SD_EARG, "null argument");
  const int nc = dtype == SD_C128 ? 2 : 1;
  DBuf psic, phi;
  RC(psic.alloc(ctx, 2 * n)); RC(phi.alloc(ctx, 2 * n));
  {
    DevIn in;
    RC(in.stage(ctx, dtype, psi0, on_dev, n));
    RC(sd_k_promote(ctx, psic.p, in.p, nc, n));                                           // :202
  }
  // phi doubles as the scratch for H psi0 (only E0 is kept): the recursion then holds psi0, phi and its three work vectors --
  // five vectors of n elements plus halo and send buffer on a shard
  RC(sp.start(os, psic.p, phi.p));
  if (nd != n) RC(phi.alloc(ctx, 2 * nd));                                                // phi_q lives in the recursion's sector
  // every pair (q, 2 pi - q) of the list is computed once for a real psi0 (pair_momenta)
  std::vector<int> same_as, live;
  RC(pair_momenta(os, dtype, psic.p, n, q, Qn, same_as));
  for (int iq = 0; iq < Qn; ++iq) if (same_as[iq] < 0) live.push_back(iq);
  const int Qb = (int)live.size();
  if (sp.can_batch(Qb)) {
    DBuf phib, nrm;
    RC(phib.alloc(ctx, 2 * nd * Qb)); RC(nrm.alloc(ctx, 2 * (int64_t)Qb));
    for (int k = 0; k < Qb; ++k) {
      RC(make_phi(psic.p, q[live[k]], phib.p + 2 * nd * k));                              // :223
      RC(sd_k_nrm2sq_to(ctx, phib.p + 2 * nd * k, 2 * nd, nrm.p + 2 * k));
    }
    std::vector<double> hn(2 * (size_t)Qb);
    RC(read_back(ctx, hn.data(), nrm.p, sizeof(double) * hn.size()));
    // zero vectors (:226-229) drop out of the batch; the rest are normalised in place (:231)
    std::vector<double *> kept; std::vector<double> norms;
    for (int k = 0; k < Qb; ++k) {
      const double nphi = std::sqrt(hn[2 * (size_t)k]);
      double *Srow = Smat + (size_t)live[k] * W;
      if (nphi == 0) { for (int iw = 0; iw < W; ++iw) Srow[iw] = 0.0; continue; }
      const int dst = (int)kept.size();
      if (dst != k) RC(d2d(ctx, phib.p + 2 * nd * dst, phib.p + 2 * nd * k, 2 * nd));
      RC(sd_k_scale_div(ctx, phib.p + 2 * nd * dst, phib.p + 2 * nd * dst, 2 * nd, nphi));
      kept.push_back(Srow); norms.push_back(nphi);
    }
    if (!kept.empty()) RC(sp.batch(phib.p, (int)kept.size(), norms.data(), kept.data()));
  } else {
    int rc = 0;
    for (int iq : live) {                                                                 // :218 (serial over q)
      double *Srow = Smat + (size_t)iq * W;
      RC(make_phi(psic.p, q[iq], phi.p));                                                 // :223
      const double norm_phi = norm_dev(sp.op, phi.p, 2 * nd, &rc); RC(rc);
      if (norm_phi == 0) { for (int iw = 0; iw < W; ++iw) Srow[iw] = 0.0; continue; }     // :226-229, src/LanczosSqw.jl:67-70
      RC(sd_k_scale_div(ctx, phi.p, phi.p, 2 * nd, norm_phi));                            // :231
      RC(sp.one(phi.p, norm_phi, Srow));
    }
  }
  for (int iq = 0; iq < Qn; ++iq)
    if (same_as[iq] >= 0) std::memcpy(Smat + (size_t)iq * W, Smat + (size_t)same_as[iq] * W, sizeof(double) * (size_t)W);
  SD_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return SD_OK;
}

// phi_q = S^z_q psi0 in psi0's own sector (src/KPM_Sqw.jl:223)
auto szq_of(sd_ctx *ctx, const sd_model *m) {
  return [=](const double *psic, double q, double *out) { return sd_launch_szq(ctx, m, SD_C128, psic, q, out); };
}

// ---- transverse S(q,w): S^+- and S^-+ between adjacent sectors (DESIGN.md "Transverse S(q,w)") ----
// The caller owns both models: src holds psi0, dst is the sector S^-_q (op SD_SPIN_MINUS) or S^+_q (SD_SPIN_PLUS) maps it to.
// E0 comes from src, the recursion (bounds, moments, tridiagonal) runs on dst's H.  H is real in both sectors, so the rows
// of q and 2 pi - q agree for a real psi0 here too.
auto spm_q_of(sd_ctx *ctx, const sd_model *src, const sd_model *dst, int op) {
  return [=](const double *psic, double q, double *out) { return sd_launch_spm_q(ctx, src, dst, op, SD_C128, psic, q, out); };
}
template <class T>
bool same_bits(const std::vector<T> &x, const std::vector<T> &y) {
  return x.size() == y.size() && (x.empty() || std::memcmp(x.data(), y.data(), sizeof(T) * x.size()) == 0);
}
int spm_check(sd_ctx *ctx, const sd_model *src, const sd_model *dst, int op) {
  if (!ctx) return SD_EARG;
  if (!src || !dst) return sd_set_err(ctx, SD_EARG, "null model");
  if (op != SD_SPIN_MINUS && op != SD_SPIN_PLUS) return sd_set_err(ctx, SD_EARG, "op must be SD_SPIN_MINUS or SD_SPIN_PLUS");
  if (src->L != dst->L) return sd_set_err(ctx, SD_EARG, "source and target models have different L");
  if (!same_bits(src->hop_i, dst->hop_i) || !same_bits(src->hop_j, dst->hop_j) || !same_bits(src->hop_J, dst->hop_J))
    return sd_set_err(ctx, SD_EARG, "source and target models have different hopping lists");
  if (!same_bits(src->zz_i, dst->zz_i) || !same_bits(src->zz_j, dst->zz_j) || !same_bits(src->zz_J, dst->zz_J))
    return sd_set_err(ctx, SD_EARG, "source and target models have different zz lists");
  if (!same_bits(src->field, dst->field)) return sd_set_err(ctx, SD_EARG, "source and target models have different fields");
  if ((src->nup < 0) != (dst->nup < 0)) return sd_set_err(ctx, SD_EARG, "one model is a sector, the other the full basis");
  if (src->nup >= 0 && dst->nup != src->nup + (op == SD_SPIN_MINUS ? -1 : 1))
    return sd_set_err(ctx, SD_EARG, op == SD_SPIN_MINUS ? "target nup must be source nup - 1 for S^-" : "target nup must be source nup + 1 for S^+");
  if (src->nranks != 1 || dst->nranks != 1) return sd_set_err(ctx, SD_EARG, "transverse operators need unsharded models");
  if (ctx->user_apply) return sd_set_err(ctx, SD_EARG, "a caller's operator is installed on this context: it belongs to one sector");
  if (!src->dev_ready || !dst->dev_ready) return sd_set_err(ctx, SD_EARG, "model has no device tables (created without a context)");
  return SD_OK;
}

// phi = S^-+_q psi0 as a vector (host pointers, or device pointers when on_dev)
int spm_q_core(sd_ctx *ctx, const sd_model *src, const sd_model *dst, int op, int dtype_in, const void *psi0, int64_t n_src,
               double q, void *phi, int64_t n_dst, bool on_dev) {
  RC(spm_check(ctx, src, dst, op));
  if (!psi0 || !phi) return sd_set_err(ctx, SD_EARG, "null argument");
  if (dtype_in != SD_F64 && dtype_in != SD_C128) return sd_set_err(ctx, SD_EARG, "bad dtype");
  if (n_src != src->N) return sd_set_err(ctx, SD_EDIM, "psi0 length does not match the source basis dimension");
  if (n_dst != dst->N) return sd_set_err(ctx, SD_EDIM, "output length does not match the target basis dimension");
  SD_HIP(ctx, hipSetDevice(ctx->device));
  DevIn in;
  DevOut out;
  RC(in.stage(ctx, dtype_in, psi0, on_dev, n_src));
  RC(out.open(ctx, phi, on_dev, 2 * n_dst));
  RC(sd_launch_spm_q(ctx, src, dst, op, dtype_in, in.p, q, out.p));
  return out.close(false);                                 // the device form takes nothing from the pool
}
// ---- site-resolved KPM moments (the quantity of the reference's src/TimeEvolution/KPM.jl) ----
// mu_n^{ij} = <psi0| S^z_i T_n(H~) S^z_j |psi0> for the sources j = sources[0..ns) against ALL sites i: per source
// v_0 = S^z_j psi0 (k_spin_op), v_1 = H~ v_0 (SD_EPI_RESCALE), v_n = 2 H~ v_{n-1} - v_{n-2} (SD_EPI_RECUR), and after each vector
// one projection pass <S^z_i psi0|v_n>, i = 1..L (sd_launch_site_project) whose 2L + 2 doubles land in a slot of their own on the
// device: the whole recursion is queued without a host round trip and read back once.  psi0: device, `dtype`, N rows -- the bra
// stays in its own element type.  mu: ns x M x L complex (re, im).  Sources share their launches (sd_epi_args::batch) under
// the conditions of KpmSpectrum::can_batch; a source of a batch sees the arithmetic of a recursion of its own.
int site_moments_dev(Op &op, int dtype, const double *psi0, const int *sources, int ns, int M, double a, double b, double *mu) {
  sd_ctx *ctx = op.ctx;
  const sd_model *m = op.m;
  const int64_t N = op.n;
  const int L = m->L;
  if (m->nranks != 1) return sd_set_err(ctx, SD_EARG, "site moments need an unsharded model");
  if (dtype != SD_F64 && dtype != SD_C128) return sd_set_err(ctx, SD_EARG, "bad dtype");
  if (M < 2) return sd_set_err(ctx, SD_EARG, "kpm_m must be >= 2");
  if (ns < 1 || !sources) return sd_set_err(ctx, SD_EARG, "at least one source site is needed");
  for (int s = 0; s < ns; ++s)
    if (sources[s] < 1 || sources[s] > L) return sd_set_err(ctx, SD_EARG, "source site " + std::to_string(sources[s]) + " is outside 1..L");
  if (!(a > 0.0) || !std::isfinite(a) || !std::isfinite(b)) return sd_set_err(ctx, SD_EARG, "the rescaling needs a finite a > 0 and a finite b");
  if (!psi0 || !mu) return sd_set_err(ctx, SD_EARG, "null argument");
  int Qmax = 1;
  if (ns >= 2 && launches_shareable(op))
    Qmax = (int)std::min<int64_t>(ns, std::max<int64_t>(1, ((int64_t)4 << 30) / (std::max<int64_t>(N, 1) * 16 * 4)));
  const int64_t slot = 2 * (int64_t)L + 2, srow = slot * M;
  DBuf psic, b0, b1, b2, res;
  RC(psic.alloc(ctx, 2 * N));
  RC(b0.alloc(ctx, 2 * N * Qmax)); RC(b1.alloc(ctx, 2 * N * Qmax)); RC(b2.alloc(ctx, 2 * N * Qmax));
  RC(res.alloc(ctx, srow * ns));
  RC(sd_k_promote(ctx, psic.p, psi0, dtype == SD_C128 ? 2 : 1, N));
  for (int s0 = 0; s0 < ns; s0 += Qmax) {
    const int Qb = std::min(Qmax, ns - s0);
    double *v_prev = b0.p, *v_curr = b1.p, *v_next = b2.p;
    double *r0 = res.p + srow * s0;
    auto project = [&](const double *v, int n) {
      return sd_launch_site_project(ctx, m, dtype, psi0, 0, v, N, Qb, r0 + slot * n, srow);
    };
    for (int k = 0; k < Qb; ++k) RC(sd_launch_spin_op(ctx, m, SD_C128, sources[s0 + k], SD_SPIN_Z, psic.p, v_prev + 2 * N * k));
    RC(project(v_prev, 0));
    sd_epi_args ea; ea.a = a; ea.b = b;
    ea.batch = Qb; ea.bstride = N;
    ctx->n_applies += Qb - 1;                                   // (Op::apply counts one)
    RC(op.apply(SD_C128, v_curr, v_prev, SD_EPI_RESCALE, ea));
    RC(project(v_curr, 1));
    for (int n = 2; n <= M - 1; ++n) {
      ea.prev = v_prev;
      ctx->n_applies += Qb - 1;
      RC(op.apply(SD_C128, v_next, v_curr, SD_EPI_RECUR, ea));
      RC(project(v_next, n));
      double *t = v_prev; v_prev = v_curr; v_curr = v_next; v_next = t;
    }
  }
  std::vector<double> hs((size_t)(srow * ns));
  RC(read_back(ctx, hs.data(), res.p, sizeof(double) * hs.size()));
  for (int s = 0; s < ns; ++s) {
    const double *h = hs.data() + (size_t)(srow * s);
    const double n0 = h[2 * L];
    for (int n = 0; n < M; ++n) {
      const double n2 = h[(size_t)(slot * n) + 2 * L];
      if (!std::isfinite(n2) || n2 > 1e6 * n0)
        return sd_set_err(ctx, SD_EARG, "the Chebyshev vectors grow (|v_" + std::to_string(n) + "|^2 = " + std::to_string(n2) + " from |v_0|^2 = " +
                                            std::to_string(n0) + "): a = " + std::to_string(a) + ", b = " + std::to_string(b) +
                                            " do not contain the spectrum");
      std::memcpy(mu + ((size_t)s * M + n) * 2 * L, h + (size_t)(slot * n), sizeof(double) * 2 * (size_t)L);
    }
  }
  return SD_OK;
}

int site_project_core(sd_ctx *ctx, const sd_model *m, int dtype_bra, const void *bra, const void *ket, int64_t n, double *out,
                      bool on_dev) {
  RC(check_unsharded_model(ctx, m));
  if (n != m->N) return sd_set_err(ctx, SD_EDIM, "vector length does not match the basis dimension");
  if (!ket || !out) return sd_set_err(ctx, SD_EARG, "null argument");
  DevIn b, k;
  DBuf res;
  RC(b.stage(ctx, dtype_bra, bra, on_dev, n));
  RC(k.stage(ctx, SD_C128, ket, on_dev, n));
  const int L = m->L;
  RC(res.alloc(ctx, 2 * (int64_t)L + 2));
  RC(sd_launch_site_project(ctx, m, dtype_bra, b.p, 0, k.p, n, 1, res.p, 2 * (int64_t)L + 2));
  return read_back(ctx, out, res.p, sizeof(double) * 2 * (size_t)L);
}

int site_moments_core(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi0, int64_t n, const int *sources, int ns, int M,
                      double a, double b, double *mu, bool on_dev) {
  Op op; RC(op.init(ctx, m, nullptr));
  if (n != m->N) return sd_set_err(ctx, SD_EDIM, "psi0 length does not match the basis dimension");
  DevIn in;
  RC(in.stage(ctx, dtype, psi0, on_dev, n));
  return site_moments_dev(op, dtype, in.p, sources, ns, M, a, b, mu);
}

// E0, a, b and the damping factors exactly as kpm_sqw forms them (KpmSpectrum::start), then the site moments of a host psi0
int site_spectral_moments(Op &op, KpmSpectrum &sp, int dtype, const void *psi0, int64_t n, const int *sources, int ns,
                          std::vector<double> &mu) {
  sd_ctx *ctx = op.ctx;
  if (op.m->nranks != 1) return sd_set_err(ctx, SD_EARG, "site correlations need an unsharded model");
  if (n != op.n) return sd_set_err(ctx, SD_EDIM, "psi0 length does not match the basis dimension");
  RC(sp.check());
  if (sp.W > 0 && !sp.omega) return sd_set_err(ctx, SD_EARG, "null argument");
  DevIn in;
  RC(in.stage(ctx, dtype, psi0, false, n));
  {
    DBuf psic, scratch;
    RC(psic.alloc(ctx, 2 * n)); RC(scratch.alloc(ctx, 2 * n));
    RC(sd_k_promote(ctx, psic.p, in.p, dtype == SD_C128 ? 2 : 1, n));
    RC(sp.start(op, psic.p, scratch.p));
  }
  mu.assign((size_t)std::max(ns, 0) * (size_t)sp.kpm_m * (size_t)op.m->L * 2, 0.0);
  return site_moments_dev(op, dtype, in.p, sources, ns, sp.kpm_m, sp.a, sp.b, mu.data());
}
}  // namespace

// kpm_sqw; psi0: host vector (unsharded form) or this rank's rows on the device (sharded form)
extern "C" int sd_kpm_sqw(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi0, int64_t n, const double *q, int Qn,
                          const double *omega, int W, int have_ab, double a, double b, int kpm_m, int kernel,
                          uint64_t seed, double *Smat) { return abi_guard(ctx, [&]() -> int {
  Op op; RC(op.init(ctx, m, nullptr));
  KpmSpectrum sp(op, omega, W, have_ab, a, b, kpm_m, kernel, seed);
  return sqw_core(op, dtype, psi0, false, n, szq_of(ctx, m), sp, q, Qn, Smat);
}); }

extern "C" int sd_kpm_sqw_sharded(sd_ctx *ctx, const sd_model *m, sd_comm *comm, int dtype, const void *psi0_dev,
                                  int64_t n_local, const double *q, int Qn, const double *omega, int W, int have_ab, double a,
                                  double b, int kpm_m, int kernel, uint64_t seed, double *Smat) { return abi_guard(ctx, [&]() -> int {
  Op op; RC(op.init(ctx, m, comm));
  KpmSpectrum sp(op, omega, W, have_ab, a, b, kpm_m, kernel, seed);
  return sqw_core(op, dtype, psi0_dev, true, n_local, szq_of(ctx, m), sp, q, Qn, Smat);
}); }

extern "C" int sd_lanczos_sqw(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi0, int64_t n, const double *q, int Qn,
                              const double *omega, int W, int lanc_m, double eta, int broaden, double *Smat) { return abi_guard(ctx, [&]() -> int {
  Op op; RC(op.init(ctx, m, nullptr));
  LanczosSpectrum sp(op, omega, W, lanc_m, eta, broaden);
  return sqw_core(op, dtype, psi0, false, n, szq_of(ctx, m), sp, q, Qn, Smat);
}); }

extern "C" int sd_spm_q(sd_ctx *ctx, const sd_model *src, const sd_model *dst, int op, int dtype_in, const void *psi0_host,
                        int64_t n_src, double q, void *phi_out_host, int64_t n_dst) {
  return abi_guard(ctx, [&]() -> int { return spm_q_core(ctx, src, dst, op, dtype_in, psi0_host, n_src, q, phi_out_host, n_dst, false); });
}
extern "C" int sd_spm_q_dev(sd_ctx *ctx, const sd_model *src, const sd_model *dst, int op, int dtype_in, const void *psi0_dev,
                            int64_t n_src, double q, void *phi_out_dev, int64_t n_dst) {
  return abi_guard(ctx, [&]() -> int { return spm_q_core(ctx, src, dst, op, dtype_in, psi0_dev, n_src, q, phi_out_dev, n_dst, true); });
}

extern "C" int sd_kpm_sqw_transverse(sd_ctx *ctx, const sd_model *src, const sd_model *dst, int op, int dtype, const void *psi0,
                                     int64_t n, const double *q, int Qn, const double *omega, int W, int have_ab, double a,
                                     double b, int kpm_m, int kernel, uint64_t seed, double *Smat) { return abi_guard(ctx, [&]() -> int {
  RC(spm_check(ctx, src, dst, op));
  Op os; RC(os.init(ctx, src, nullptr));
  Op od; RC(od.init(ctx, dst, nullptr));
  KpmSpectrum sp(od, omega, W, have_ab, a, b, kpm_m, kernel, seed);
  sp.batchable = false;      // one momentum at a time, as before: sharing launches here is a separate, measured change
  return sqw_core(os, dtype, psi0, false, n, spm_q_of(ctx, src, dst, op), sp, q, Qn, Smat);
}); }

extern "C" int sd_lanczos_sqw_transverse(sd_ctx *ctx, const sd_model *src, const sd_model *dst, int op, int dtype,
                                         const void *psi0, int64_t n, const double *q, int Qn, const double *omega, int W,
                                         int lanc_m, double eta, int broaden, double *Smat) { return abi_guard(ctx, [&]() -> int {
  RC(spm_check(ctx, src, dst, op));
  Op os; RC(os.init(ctx, src, nullptr));
  Op od; RC(od.init(ctx, dst, nullptr));
  LanczosSpectrum sp(od, omega, W, lanc_m, eta, broaden);
  sp.batchable = false;      // one momentum at a time, as before: sharing launches here is a separate, measured change
  return sqw_core(os, dtype, psi0, false, n, spm_q_of(ctx, src, dst, op), sp, q, Qn, Smat);
}); }

extern "C" int sd_site_project(sd_ctx *ctx, const sd_model *m, int dtype_bra, const void *bra_host, const void *ket_host, int64_t n,
                               double *out) {
  return abi_guard(ctx, [&]() -> int { return site_project_core(ctx, m, dtype_bra, bra_host, ket_host, n, out, false); });
}
extern "C" int sd_site_project_dev(sd_ctx *ctx, const sd_model *m, int dtype_bra, const void *bra_dev, const void *ket_dev, int64_t n,
                                   double *out) {
  return abi_guard(ctx, [&]() -> int { return site_project_core(ctx, m, dtype_bra, bra_dev, ket_dev, n, out, true); });
}

extern "C" int sd_kpm_site_moments(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi0_host, int64_t n, const int *sources,
                                   int ns, int M, double a, double b, double *mu_out) {
  return abi_guard(ctx, [&]() -> int { return site_moments_core(ctx, m, dtype, psi0_host, n, sources, ns, M, a, b, mu_out, false); });
}
extern "C" int sd_kpm_site_moments_dev(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi0_dev, int64_t n, const int *sources,
                                       int ns, int M, double a, double b, double *mu_out) {
  return abi_guard(ctx, [&]() -> int { return site_moments_core(ctx, m, dtype, psi0_dev, n, sources, ns, M, a, b, mu_out, true); });
}

extern "C" int sd_kpm_reconstruct_signed(const double *mu, int kpm_m, const double *omega, int W, double a, double b, double E0,
                                         double *out) {
  if (kpm_m < 1 || W < 0 || !mu || !out || (W > 0 && !omega)) return SD_EARG;
  const double PI = 3.14159265358979323846;
  for (int iw = 0; iw < W; ++iw) {
    const double x = (omega[iw] + E0 - b) / a;
    if (!(std::fabs(x) < 1.0)) { out[iw] = 0.0; continue; }
    double tm = 1.0, tc = x, sum_val = mu[0];                          // T_0, T_1
    for (int n = 1; n < kpm_m; ++n) {
      sum_val += 2.0 * mu[n] * tc;
      const double tn = 2.0 * x * tc - tm;
      tm = tc; tc = tn;
    }
    out[iw] = sum_val / (a * (PI * std::sqrt(1.0 - x * x)));
  }
  return SD_OK;
}

extern "C" int sd_kpm_site_correlations(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi0, int64_t n, const int *sources,
                                        int ns, const double *omega, int W, int have_ab, double a, double b, int kpm_m, int kernel,
                                        uint64_t seed, double *C_out) { return abi_guard(ctx, [&]() -> int {
  Op op; RC(op.init(ctx, m, nullptr));
  if (!C_out) return sd_set_err(ctx, SD_EARG, "null argument");
  KpmSpectrum sp(op, omega, W, have_ab, a, b, kpm_m, kernel, seed);
  std::vector<double> mu;
  RC(site_spectral_moments(op, sp, dtype, psi0, n, sources, ns, mu));
  const int L = m->L, M = kpm_m;
  std::vector<double> mre(M), mim(M), cre(std::max(W, 1)), cim(std::max(W, 1));
  for (int s = 0; s < ns; ++s)
    for (int i = 0; i < L; ++i) {
      for (int k = 0; k < M; ++k) {
        const double *e = mu.data() + (((size_t)s * M + k) * L + i) * 2;
        mre[k] = sp.g[k] * e[0]; mim[k] = sp.g[k] * e[1];
      }
      sd_kpm_reconstruct_signed(mre.data(), M, omega, W, sp.a, sp.b, sp.E0, cre.data());
      sd_kpm_reconstruct_signed(mim.data(), M, omega, W, sp.a, sp.b, sp.E0, cim.data());
      double *row = C_out + ((size_t)i * ns + s) * (size_t)W * 2;
      for (int iw = 0; iw < W; ++iw) { row[2 * iw] = cre[iw]; row[2 * iw + 1] = cim[iw]; }
    }
  return SD_OK;
}); }

extern "C" int sd_kpm_sqw_sites(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi0, int64_t n, const double *q, int Qn,
                                const double *omega, int W, const int *sources, int ns, int translation_invariant, int have_ab,
                                double a, double b, int kpm_m, int kernel, uint64_t seed, double *Smat,
                                double *defect_out) { return abi_guard(ctx, [&]() -> int {
  Op op; RC(op.init(ctx, m, nullptr));
  const int L = m->L, M = kpm_m;
  if (!Smat || (Qn > 0 && !q) || Qn < 0) return sd_set_err(ctx, SD_EARG, "null argument");
  if (ns < 1 || !sources) return sd_set_err(ctx, SD_EARG, "at least one source site is needed");
  if (translation_invariant) {
    if (ns != 1) return sd_set_err(ctx, SD_EARG, "translation_invariant takes exactly one source site");
  } else {
    if (ns != L) return sd_set_err(ctx, SD_EARG, "without translation_invariant the sources must be all L sites, each once");
    std::vector<char> seen((size_t)L + 1, 0);
    for (int s = 0; s < ns; ++s) {
      if (sources[s] < 1 || sources[s] > L) return sd_set_err(ctx, SD_EARG, "source site " + std::to_string(sources[s]) + " is outside 1..L");
      if (seen[sources[s]]++) return sd_set_err(ctx, SD_EARG, "without translation_invariant the sources must be all L sites, each once");
    }
  }
  KpmSpectrum sp(op, omega, W, have_ab, a, b, kpm_m, kernel, seed);
  std::vector<double> mu;
  RC(site_spectral_moments(op, sp, dtype, psi0, n, sources, ns, mu));
  double defect = 0.0;
  const double quarter = mu[((size_t)0 * L + (sources[0] - 1)) * 2];          // mu_0^{jj} = |psi0|^2 / 4
  std::vector<double> muq(M), cr(L), ci(L);
  for (int iq = 0; iq < Qn; ++iq) {
    for (int r = 0; r < L; ++r) { cr[r] = std::cos(q[iq] * (double)r); ci[r] = std::sin(q[iq] * (double)r); }
    for (int k = 0; k < M; ++k) {
      double sre = 0.0, sim = 0.0;
      for (int s = 0; s < ns; ++s) {
        const int rj = sources[s] - 1;
        const double *e = mu.data() + ((size_t)s * M + k) * L * 2;
        double tre = 0.0, tim = 0.0;                                          // sum_i e^{-iq r_i} mu^{ij}
        for (int i = 0; i < L; ++i) { tre += cr[i] * e[2 * i] + ci[i] * e[2 * i + 1]; tim += cr[i] * e[2 * i + 1] - ci[i] * e[2 * i]; }
        sre += cr[rj] * tre - ci[rj] * tim;                                   // times e^{+iq r_j}
        sim += cr[rj] * tim + ci[rj] * tre;
      }
      if (translation_invariant) {
        muq[k] = sre;
        if (quarter > 0.0) defect = std::max(defect, std::fabs(sim) / quarter);
        else if (sim != 0.0) defect = HUGE_VAL;
      } else {
        muq[k] = sre / (double)L;
      }
      muq[k] *= sp.g[k];
    }
    sd_kpm_reconstruct(muq.data(), M, omega, W, sp.a, sp.b, sp.E0, Smat + (size_t)iq * W);
  }
  if (defect_out) *defect_out = defect;
  return SD_OK;
}); }

// --------------------------------------------------------------------------
// Finite temperature by dynamical quantum typicality; the reference's unreachable module
// src/TimeEvolution/QuantumTypicality.jl is the model, on this library's own definitions.
// --------------------------------------------------------------------------
namespace {

// e_k = exp(-z) I_k(z), k = 0 .. n_used - 1, and n_used = the first k with k > z and e_k < 2^-53 e_0.  Ratios r_k = I_k / I_{k-1}
// from the continued fraction r_k = 1 / (2k/z + r_{k+1}) started far above the last term kept, products t_k = r_1 ... r_k and the
// normalisation exp(z) = I_0 + 2 sum_k I_k: all terms positive, no cancellation, no overflow at any z.  Extended precision on
// the host, so that the rounded values are the correctly scaled Bessel functions to an ulp.
void scaled_bessel_i(double z, std::vector<double> &e, int *n_used) {
  if (z == 0.0) { e.assign(1, 1.0); *n_used = 1; return; }
  const int ktop = (int)std::ceil(z) + 128;
  std::vector<long double> t((size_t)ktop + 2);
  long double r = 0.0L;
  for (int k = ktop; k >= 1; --k) { r = 1.0L / (2.0L * (long double)k / (long double)z + r); t[k] = r; }
  t[0] = 1.0L;
  for (int k = 1; k <= ktop; ++k) t[k] *= t[k - 1];
  long double S = 0.0L;
  for (int k = ktop; k >= 1; --k) S += t[k];
  S = 2.0L * S + t[0];
  const double e0 = (double)(t[0] / S);
  int nu = ktop;
  for (int k = 1; k <= ktop; ++k)
    if ((double)k > z && (double)(t[k] / S) < 0x1p-53 * e0) { nu = k; break; }
  e.resize(nu);
  for (int k = 0; k < nu; ++k) e[k] = (double)(t[k] / S);
  *n_used = nu;
}

// Emin, Emax as given, or (Emax <= Emin) estimated as estimate_energy_bounds does; a spectrum of one point (a one-state sector)
// gets half a unit on either side so that the rescaling H~ = (H - b)/a exists
int typicality_bounds(Op &op, uint64_t seed, double *Emin, double *Emax) {
  if (!std::isfinite(*Emin) || !std::isfinite(*Emax)) return sd_set_err(op.ctx, SD_EARG, "the energy bounds must be finite");
  if (*Emax > *Emin) return SD_OK;
  RC(energy_bounds_core(op, 80, nullptr, nullptr, true, seed, Emin, Emax));
  if (!(*Emax - *Emin > 1e-8 * std::max(1.0, std::max(std::fabs(*Emin), std::fabs(*Emax))))) { *Emin -= 0.5; *Emax += 0.5; }
  return SD_OK;
}

constexpr double SD_IMAG_ZMAX = 600.0;

// v (device, ComplexF64, n elements) <- exp(-tau H) v / |.|, *log_norm = ln |exp(-tau H) v|.  Chebyshev: with H = a H~ + b,
// exp(-tau H) = exp(-tau (b - a)) sum_k c_k T_k(H~), c_k = (2 - delta_k0) (-1)^k exp(-z) I_k(z), z = a tau, through the term loop
// of chebyshev_time_evolve; z > 600 is split into equal sub-steps, renormalised after each, the logarithms added up.
int imag_evolve_dev(Op &op, double *v, int64_t n, double tau, int method, int cheb_n, int kry_m, double Emin, double Emax,
                    uint64_t seed, double *log_norm) {
  sd_ctx *ctx = op.ctx;
  if (!(tau >= 0.0) || !std::isfinite(tau)) return sd_set_err(ctx, SD_EARG, "the imaginary time must be finite and >= 0");
  if (cheb_n < 0) return sd_set_err(ctx, SD_EARG, "cheb_n must be >= 0 (0: automatic)");
  int rc = 0;
  if (method == SD_EVOLVE_KRYLOV) return krylov_evolve_core(op, SD_C128, v, n, tau, kry_m, v, true, log_norm);
  if (method != SD_EVOLVE_CHEBYSHEV) return sd_set_err(ctx, SD_EARG, "unknown evolution method");
  RC(typicality_bounds(op, seed, &Emin, &Emax));
  const double a = (Emax - Emin) / (2 * 0.9999), b = (Emax + Emin) / 2;
  const double z = a * tau;
  if (!(z <= SD_CHEB_ZMAX * SD_IMAG_ZMAX)) return sd_set_err(ctx, SD_EARG, "a * tau is too large: more than 1e6 sub-steps of z = 600");
  const int nsub = z > SD_IMAG_ZMAX ? (int)std::ceil(z / SD_IMAG_ZMAX) : 1;
  const double tsub = tau / nsub;
  std::vector<double> e;
  int nu = 0;
  scaled_bessel_i(a * tsub, e, &nu);
  const int nterm = cheb_n > 0 ? std::min(cheb_n, nu) : nu;
  std::vector<double> c(2 * (size_t)nterm, 0.0);
  for (int k = 0; k < nterm; ++k) c[2 * k] = (k == 0 ? 1.0 : 2.0) * ((k & 1) ? -e[k] : e[k]);
  DBuf b0, b1, b2;
  RC(b0.alloc(ctx, 2 * n)); RC(b1.alloc(ctx, 2 * n)); RC(b2.alloc(ctx, 2 * n));
  double ln = 0.0;
  for (int s = 0; s < nsub; ++s) {
    RC(d2d(ctx, b0.p, v, 2 * n));
    RC(cheb_terms(op, b0.p, b1.p, b2.p, v, n, a, b, c.data(), nterm, 1));
    const double nn = norm_dev(op, v, 2 * n, &rc); RC(rc);
    if (!(nn > 0) || !std::isfinite(nn)) return sd_set_err(ctx, SD_EZERO, "the imaginary-time state has zero or non-finite norm");
    RC(sd_k_scale_div(ctx, v, v, 2 * n, nn));
    ln += std::log(nn) - tsub * (b - a);
  }
  SD_HIP(ctx, hipStreamSynchronize(ctx->stream));
  *log_norm = ln;
  return SD_OK;
}

int imag_evolve_core(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi0, int64_t n, double tau, int method, int cheb_n,
                     int kry_m, double Emin, double Emax, void *out, double *log_norm, bool on_dev) {
  Op op; RC(op.init(ctx, m, nullptr));
  if (n != op.n) return sd_set_err(ctx, SD_EDIM, "vector length does not match the basis dimension");
  if (!out || !log_norm) return sd_set_err(ctx, SD_EARG, "null argument");
  DevIn in;
  DevOut o;
  RC(in.stage(ctx, dtype, psi0, on_dev, n));
  RC(o.open(ctx, out, on_dev, 2 * n));
  double *v = o.p;
  if (dtype == SD_C128 && in.p == v) { /* in place */ }
  else RC(sd_k_promote(ctx, v, in.p, dtype == SD_C128 ? 2 : 1, n));
  if (tau == 0.0) {
    int rc = 0;
    const double nn = norm_dev(op, v, 2 * n, &rc); RC(rc);
    if (!(nn > 0)) return sd_set_err(ctx, SD_EZERO, "starting vector has zero norm");
    RC(sd_k_scale_div(ctx, v, v, 2 * n, nn));
    *log_norm = std::log(nn);
  } else {
    RC(imag_evolve_dev(op, v, n, tau, method, cheb_n, kry_m, Emin, Emax, 0, log_norm));
  }
  return o.close(true);                                    // the work vectors go back to the pool
}

// an operator of the typicality driver: kind, site or momentum, device weights of a current, device tables of the energy current
struct DqtOp {
  int kind = 0; int site = 0; double q = 0.0; DBuf wt; DList dl;
  int init(sd_ctx *ctx, const sd_model *m, int kind_, double param, const double *w, bool is_A) {
    kind = kind_;
    if (kind == SD_DQT_ENERGY_CURRENT) {
      if (w) return sd_set_err(ctx, SD_EARG, "the energy current takes no weights (w must be NULL)");
      if (param != 0.0 && param != 1.0) return sd_set_err(ctx, SD_EARG, "the energy current's parameter is the geometry: 0 a line, 1 a ring");
      std::vector<sd_dterm> list;
      std::string err;
      const int rc = sd_build_energy_current(m, param == 1.0, list, err);
      if (rc) return sd_set_err(ctx, rc, err);
      return dl.init(ctx, m, list.data(), (int)list.size());
    }
    if (kind == SD_DQT_SZ_SITE) {
      site = (int)param;
      if ((double)site != param || site < 1 || site > m->L) return sd_set_err(ctx, SD_EARG, "site is outside 1..L");
    } else if (kind == SD_DQT_SZ_Q) {
      q = param;
      if (!std::isfinite(q)) return sd_set_err(ctx, SD_EARG, "the momentum must be finite");
    } else if (kind == SD_DQT_CURRENT) {
      RC(current_weights(ctx, m, w, wt));
    } else if (!(kind == SD_DQT_SZ_ALL && is_A)) {
      return sd_set_err(ctx, SD_EARG, is_A ? "unknown operator kind" : "unknown operator kind (SD_DQT_SZ_ALL is for the measured operator only)");
    }
    return SD_OK;
  }
};

}  // namespace

extern "C" int sd_chebyshev_imag_coeffs(int n_max, double a, double tau, double *c, int *n_used) {
  if (!c || !n_used || n_max < 1) return SD_EARG;
  const double z = a * tau;
  if (!(z >= 0.0) || z > SD_IMAG_ZMAX) return SD_EARG;
  try {
    std::vector<double> e;
    scaled_bessel_i(z, e, n_used);
    if (*n_used > n_max) return SD_EARG;
    for (int k = 0; k < *n_used; ++k) c[k] = (k == 0 ? 1.0 : 2.0) * ((k & 1) ? -e[k] : e[k]);
  } catch (...) { return SD_ENOMEM; }
  return SD_OK;
}

extern "C" int sd_imag_evolve(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi0_host, int64_t n, double tau, int method,
                              int cheb_n, int kry_m, double Emin, double Emax, void *out_host, double *log_norm) {
  return abi_guard(ctx, [&]() -> int { return imag_evolve_core(ctx, m, dtype, psi0_host, n, tau, method, cheb_n, kry_m, Emin, Emax, out_host, log_norm, false); });
}
extern "C" int sd_imag_evolve_dev(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi0_dev, int64_t n, double tau, int method,
                                  int cheb_n, int kry_m, double Emin, double Emax, void *out_dev, double *log_norm) {
  return abi_guard(ctx, [&]() -> int { return imag_evolve_core(ctx, m, dtype, psi0_dev, n, tau, method, cheb_n, kry_m, Emin, Emax, out_dev, log_norm, true); });
}

extern "C" int sd_dqt_correlations(sd_ctx *ctx, const sd_model *m, double beta, const void *r_host, uint64_t seed, int B_kind,
                                   double B_param, const double *w_B, int A_kind, double A_param, const double *w_A,
                                   const double *times, int nt, int method, int cheb_n, int kry_m, double Emin, double Emax,
                                   double *num, double *den, double *energy, double *log_norm) { return abi_guard(ctx, [&]() -> int {
  Op op; RC(op.init(ctx, m, nullptr));
  const int64_t n = op.n;
  const int L = m->L;
  if (!times || nt < 1 || !num || !den || !energy || !log_norm) return sd_set_err(ctx, SD_EARG, "null argument");
  if (!(beta >= 0.0) || !std::isfinite(beta)) return sd_set_err(ctx, SD_EARG, "beta must be finite and >= 0");
  if (!(times[0] >= 0.0)) return sd_set_err(ctx, SD_EARG, "times must start at t >= 0");
  for (int k = 0; k < nt; ++k)
    if (!std::isfinite(times[k]) || (k > 0 && times[k] < times[k - 1])) return sd_set_err(ctx, SD_EARG, "times must be finite and non-decreasing");
  if (method != SD_EVOLVE_CHEBYSHEV && method != SD_EVOLVE_KRYLOV) return sd_set_err(ctx, SD_EARG, "unknown evolution method");
  if (cheb_n < 0) return sd_set_err(ctx, SD_EARG, "cheb_n must be >= 0 (0: automatic)");
  if (method == SD_EVOLVE_KRYLOV && kry_m < 1) return sd_set_err(ctx, SD_EARG, "kry_m must be >= 1");
  DqtOp Bo, Ao;
  RC(Bo.init(ctx, m, B_kind, B_param, w_B, false));
  RC(Ao.init(ctx, m, A_kind, A_param, w_A, true));
  const int nA = A_kind == SD_DQT_SZ_ALL ? L : 1;
  const int64_t mrow = A_kind == SD_DQT_SZ_ALL ? 2 * (int64_t)L + 2 : 2;      // doubles filed per time point
  // the two states live back to back -- psi_beta at [0, n), phi = B psi_beta at [n, 2n) -- so that one batched launch serves both
  DBuf s0, s1, w0, w1, tmp, meas;
  RC(s0.alloc(ctx, 4 * n)); RC(tmp.alloc(ctx, 2 * n)); RC(meas.alloc(ctx, mrow * nt));
  double *S = s0.p;
  int rc = 0;
  // 1. the start vector: the caller's, or the counter-based normal stream of `seed` (sd_fill_randn_host gives the same on the host)
  if (r_host) RC(h2d(ctx, S, r_host, 2 * n));
  else RC(sd_k_fill_randn(ctx, S, 2 * n, seed, 0));
  const double nr = norm_dev(op, S, 2 * n, &rc); RC(rc);
  if (!(nr > 0) || !std::isfinite(nr)) return sd_set_err(ctx, SD_EZERO, "starting vector has zero norm");
  RC(sd_k_scale_div(ctx, S, S, 2 * n, nr));
  // 2. psi_beta = exp(-beta H / 2) r, normalised; the sample's partition weight is exp(2 log_norm)
  if (method == SD_EVOLVE_CHEBYSHEV) RC(typicality_bounds(op, seed, &Emin, &Emax));
  double ln = 0.0;
  if (beta > 0.0) RC(imag_evolve_dev(op, S, n, 0.5 * beta, method, cheb_n, kry_m, Emin, Emax, seed, &ln));
  *log_norm = ln;
  *den = std::exp(2.0 * ln);
  // 3. energy = <psi|H|psi> / <psi|psi>
  {
    sd_epi_args ea;
    double s[4];
    RC(op.apply(SD_C128, tmp.p, S, SD_EPI_DOT, ea));
    RC(sd_k_nrm2sq(ctx, S, 2 * n, 2));
    RC(sd_read_scalars(ctx, 0, 4, s));
    *energy = s[0] / s[2];
  }
  // 4. phi = B psi_beta
  double *phi = S + 2 * n;
  if (B_kind == SD_DQT_SZ_SITE) RC(sd_launch_spin_op(ctx, m, SD_C128, Bo.site, SD_SPIN_Z, S, phi));
  else if (B_kind == SD_DQT_SZ_Q) RC(sd_launch_szq(ctx, m, SD_C128, S, Bo.q, phi));
  else if (B_kind == SD_DQT_ENERGY_CURRENT) RC(sd_launch_dcurrent(ctx, m, SD_C128, S, nullptr, Bo.dl.groups, Bo.dl.n_groups, Bo.dl.terms, phi, nullptr));
  else RC(sd_launch_current(ctx, m, SD_C128, S, nullptr, Bo.wt.p, phi, nullptr));
  double nphi = 0.0;
  if (method == SD_EVOLVE_KRYLOV) { nphi = norm_dev(op, phi, 2 * n, &rc); RC(rc); }
  // 5. both states forward in time, a measurement after every step, everything filed on the device
  const bool batched = launches_shareable(op);               // two vectors of at most 2^22 rows: well inside the 4 GiB of can_batch
  const double a = (Emax - Emin) / (2 * 0.9999), b = (Emax + Emin) / 2;
  double *T = nullptr;
  if (method == SD_EVOLVE_CHEBYSHEV && times[nt - 1] > 0.0) {
    RC(s1.alloc(ctx, 4 * n)); RC(w0.alloc(ctx, 4 * n)); RC(w1.alloc(ctx, 4 * n));
    T = s1.p;
  }
  std::vector<double> c;
  double c_dt = -1.0, t_prev = 0.0;
  int nterm = 0;
  for (int k = 0; k < nt; ++k) {
    const double dt = times[k] - t_prev;
    t_prev = times[k];
    if (dt > 0.0 && method == SD_EVOLVE_CHEBYSHEV) {
      if (dt != c_dt) {                                      // equal steps reuse their coefficients
        if (!(a * dt <= SD_CHEB_ZMAX)) return sd_set_err(ctx, SD_EARG, "a * dt is too large for one Chebyshev step (above 1e6): give more time points");
        nterm = cheb_n > 0 ? cheb_n : cheb_auto_terms(a * dt);
        c.resize(2 * (size_t)nterm);
        RC(sd_chebyshev_coeffs(nterm, a, b, dt, c.data()));
        c_dt = dt;
      }
      if (batched) {
        RC(cheb_terms(op, S, w0.p, w1.p, T, n, a, b, c.data(), nterm, 2));
      } else {
        for (int v = 0; v < 2; ++v) RC(cheb_terms(op, S + 2 * n * v, w0.p + 2 * n * v, w1.p + 2 * n * v, T + 2 * n * v, n, a, b, c.data(), nterm, 1));
      }
      std::swap(S, T);
    } else if (dt > 0.0) {
      // krylov_time_evolve normalises its result; a unitary step conserves the norm, so phi gets its own back
      RC(krylov_evolve_core(op, SD_C128, S, n, dt, kry_m, S, true));
      RC(krylov_evolve_core(op, SD_C128, S + 2 * n, n, dt, kry_m, S + 2 * n, true));
      if (nphi > 0.0) RC(sd_k_scale_div(ctx, S + 2 * n, S + 2 * n, 2 * n, 1.0 / nphi));
    }
    const double *psi = S, *ph = S + 2 * n;
    double *dst = meas.p + mrow * k;
    if (A_kind == SD_DQT_SZ_SITE) {
      RC(sd_launch_spin_op(ctx, m, SD_C128, Ao.site, SD_SPIN_Z, psi, tmp.p));
      RC(sd_k_dot_to(ctx, 2, tmp.p, ph, n, dst));
    } else if (A_kind == SD_DQT_SZ_Q) {                      // the adjoint: <S^z_q psi | phi>
      RC(sd_launch_szq(ctx, m, SD_C128, psi, Ao.q, tmp.p));
      RC(sd_k_dot_to(ctx, 2, tmp.p, ph, n, dst));
    } else if (A_kind == SD_DQT_SZ_ALL) {
      RC(sd_launch_site_project(ctx, m, SD_C128, psi, 0, ph, n, 1, dst, mrow));
    } else if (A_kind == SD_DQT_ENERGY_CURRENT) {
      RC(sd_launch_dcurrent(ctx, m, SD_C128, ph, psi, Ao.dl.groups, Ao.dl.n_groups, Ao.dl.terms, nullptr, dst));
    } else {
      RC(sd_launch_current(ctx, m, SD_C128, ph, psi, Ao.wt.p, nullptr, dst));
    }
  }
  std::vector<double> h((size_t)(mrow * nt));
  RC(read_back(ctx, h.data(), meas.p, sizeof(double) * h.size()));
  for (int k = 0; k < nt; ++k)
    std::memcpy(num + (size_t)2 * nA * k, h.data() + (size_t)mrow * k, sizeof(double) * 2 * (size_t)nA);
  return SD_OK;
}); }

// --------------------------------------------------------------------------
// The lowest eigenpairs by thick-restart Lanczos (include/spindyn.h, sd_lanczos_eigenpairs)
// --------------------------------------------------------------------------

// eigen(Symmetric(A)) by cyclic Jacobi rotations (row-cyclic sweeps until the off-diagonal norm is below u |A|_F)
extern "C" int sd_sym_eig(int n, const double *A_in, double *w, double *Z) {
  if (n < 1 || n > SD_EIGS_MAX_BASIS || !A_in || !w || !Z) return SD_EARG;
  try {
    std::vector<double> A((size_t)n * n);
    for (int c = 0; c < n; ++c)
      for (int r = c; r < n; ++r) A[r + (size_t)n * c] = A[c + (size_t)n * r] = A_in[r + (size_t)n * c];
    std::fill(Z, Z + (size_t)n * n, 0.0);
    for (int i = 0; i < n; ++i) Z[i + (size_t)n * i] = 1.0;
    double fro2 = 0.0;
    for (double x : A) fro2 += x * x;
    const double u = 1.1102230246251565e-16, stop2 = u * u * fro2;
    bool done = n == 1 || fro2 == 0.0;
    for (int sweep = 0; sweep < 100 && !done; ++sweep) {
      for (int p = 0; p < n - 1; ++p)
        for (int q = p + 1; q < n; ++q) {
          const double apq = A[p + (size_t)n * q];
          if (apq == 0.0) continue;
          const double theta = (A[q + (size_t)n * q] - A[p + (size_t)n * p]) / (2.0 * apq);
          const double t = std::copysign(1.0, theta) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
          const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
          double *cp = A.data() + (size_t)n * p, *cq = A.data() + (size_t)n * q;
          for (int k = 0; k < n; ++k) { const double a = cp[k], b = cq[k]; cp[k] = c * a - s * b; cq[k] = s * a + c * b; }   // A <- A J
          for (int k = 0; k < n; ++k) {                                                                               // A <- J^T A
            double *col = A.data() + (size_t)n * k;
            const double a = col[p], b = col[q];
            col[p] = c * a - s * b; col[q] = s * a + c * b;
          }
          A[p + (size_t)n * q] = A[q + (size_t)n * p] = 0.0;
          double *zp = Z + (size_t)n * p, *zq = Z + (size_t)n * q;
          for (int k = 0; k < n; ++k) { const double a = zp[k], b = zq[k]; zp[k] = c * a - s * b; zq[k] = s * a + c * b; }
        }
      double off2 = 0.0;
      for (int c = 0; c < n; ++c)
        for (int r = c + 1; r < n; ++r) off2 += A[r + (size_t)n * c] * A[r + (size_t)n * c];
      done = 2.0 * off2 <= stop2;
    }
    if (!done) return SD_EINTERNAL;
    std::vector<int> order(n);
    for (int i = 0; i < n; ++i) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return A[a + (size_t)n * a] < A[b + (size_t)n * b]; });
    std::vector<double> zc(Z, Z + (size_t)n * n);
    for (int k = 0; k < n; ++k) {
      w[k] = A[order[k] + (size_t)n * order[k]];
      std::memcpy(Z + (size_t)n * k, zc.data() + (size_t)n * order[k], sizeof(double) * n);
    }
    return SD_OK;
  } catch (...) {
    return SD_ENOMEM;
  }
}

namespace {

// include/spindyn.h, sd_lanczos_eigenpairs.  The basis is `mb` columns of ld doubles (ld even: the rotation then runs in its
// 16-byte form) plus the work vector w; columns 0..c-1 are locked, c..c+l-1 hold the Ritz vectors kept by the last restart
// (values th, couplings s to column c+l), column c+l onwards are the Lanczos vectors of the current block.
int eigs_core(Op &op, int dtype, int nev, int basis_size, double tol, int64_t max_applies, int confirm, const void *psi0, bool on_dev,
              uint64_t seed, double *evals, void *evecs, double *residuals, sd_eigs_info *info) {
  sd_ctx *ctx = op.ctx;
  const sd_model *m = op.m;
  if (m->nranks != 1) return sd_set_err(ctx, SD_EARG, "lanczos_eigenpairs: a sharded model is not supported");
  if (dtype != SD_F64 && dtype != SD_C128) return sd_set_err(ctx, SD_EARG, "bad dtype");
  if (!evals || !residuals || !info) return sd_set_err(ctx, SD_EARG, "null output");
  const int64_t N = m->N;
  if (nev < 1) return sd_set_err(ctx, SD_EARG, "lanczos_eigenpairs: nev must be >= 1");
  if (nev > SD_EIGS_MAX_NEV || nev > N) return sd_set_err(ctx, SD_EARG, "lanczos_eigenpairs: nev must be <= min(N, 24)");
  if (basis_size > SD_EIGS_MAX_BASIS) return sd_set_err(ctx, SD_EARG, "lanczos_eigenpairs: basis_size must be <= 128");
  if (basis_size < nev + 3 && basis_size < N) return sd_set_err(ctx, SD_EARG, "lanczos_eigenpairs: basis_size must be >= nev + 3 (or the basis dimension, if smaller)");
  if (!(tol >= 0.0)) return sd_set_err(ctx, SD_EARG, "lanczos_eigenpairs: tol must be >= 0");
  const int mb = (int)std::min<int64_t>(basis_size, N);
  const int nc = dtype == SD_C128 ? 2 : 1;
  const int64_t nd = nc * N, ld = nd + (nd & 1);
  const int64_t applies0 = ctx->n_applies;
  *info = sd_eigs_info{};
  info->basis_size = mb;
  info->workspace_vectors = mb + 1;

  DBuf V, w, sc, Qd;
  RC(V.alloc(ctx, ld * mb)); RC(w.alloc(ctx, nd));
  constexpr int CO = 2 * SD_EIGS_MAX_BASIS;                       // sc: coefficients of round 1 | of round 2 | |w|^2
  RC(sc.alloc(ctx, 2 * CO + 2)); RC(Qd.alloc(ctx, (int64_t)SD_EIGS_MAX_BASIS * SD_EIGS_MAX_KEEP));
  std::vector<double> hs(2 * CO + 2);
  auto col = [&](int j) { return V.p + ld * (int64_t)j; };

  // one round of classical Gram-Schmidt of w against columns 0..ncols-1 in blocks of 8: all dots first, then the subtractions
  auto cgs_round = [&](int ncols, double *coef, double *n2) -> int {
    for (int c0 = 0; c0 < ncols; c0 += SD_EIGS_BLOCK_COLS)
      RC(sd_k_block_dots(ctx, nc, col(c0), ld, std::min(SD_EIGS_BLOCK_COLS, ncols - c0), w.p, N, coef + 2 * c0));
    for (int c0 = 0; c0 < ncols; c0 += SD_EIGS_BLOCK_COLS)
      RC(sd_k_block_axpy(ctx, nc, w.p, col(c0), ld, std::min(SD_EIGS_BLOCK_COLS, ncols - c0), coef + 2 * c0, N,
                         c0 + SD_EIGS_BLOCK_COLS >= ncols ? n2 : nullptr));
    return SD_OK;
  };
  int c = 0, l = 0, n_fresh = 0;
  double scale = 0.0, scale_run = 0.0;
  std::vector<double> lam, th, s;
  // w (already filled) orthogonalised twice against the locked columns and normalised -> column c; *ok = 0: nothing was left of it
  auto seat_start = [&](int *ok) -> int {
    if (c > 0) { RC(cgs_round(c, sc.p, nullptr)); RC(cgs_round(c, sc.p + CO, nullptr)); }
    int rc = 0;
    const double nrm = norm_dev(op, w.p, nd, &rc); RC(rc);
    *ok = nrm > 0.0 && std::isfinite(nrm);
    if (*ok) RC(sd_k_scale_div(ctx, col(c), w.p, nd, nrm));
    l = 0;
    return SD_OK;
  };
  auto fresh_start = [&](int *ok) -> int {
    RC(sd_k_fill_randn(ctx, w.p, nd, seed + 0x9E3779B97F4A7C15ULL * (uint64_t)(++n_fresh), 0));
    return seat_start(ok);
  };

  // Thick-restart Lanczos on the columns behind the locked ones until `target` columns are locked.  *stopped: max_applies was
  // reached; *exhausted: the locked columns span everything that is left.
  auto run = [&](int target, bool *stopped, bool *exhausted) -> int {
    *stopped = *exhausted = false;
    while (c < target) {
      const int mact = mb - c;
      std::vector<double> T((size_t)mact * mact, 0.0);
      for (int i = 0; i < l; ++i) { T[i + (size_t)mact * i] = th[i]; T[l + (size_t)mact * i] = T[i + (size_t)mact * l] = s[i]; }
      int ja = l;
      double beta = 0.0;
      bool broke = false;
      for (int j = c + l; j < mb; ++j) {
        if (max_applies > 0 && ctx->n_applies - applies0 >= max_applies) { *stopped = true; return SD_OK; }
        sd_epi_args ea;
        RC(op.apply(dtype, w.p, col(j), SD_EPI_PLAIN, ea));
        RC(cgs_round(j + 1, sc.p, nullptr)); RC(cgs_round(j + 1, sc.p + CO, sc.p + 2 * CO));
        RC(read_back(ctx, hs.data(), sc.p, sizeof(double) * hs.size()));
        const int jj = j - c;
        const double alpha = hs[2 * j] + hs[CO + 2 * j];
        beta = std::sqrt(hs[2 * CO]);
        T[jj + (size_t)mact * jj] = alpha;
        ja = jj + 1;
        scale_run = std::max(scale_run, std::fabs(alpha));
        if (!(beta > 1e-12 * scale_run)) { broke = true; break; }
        scale_run = std::max(scale_run, beta);
        if (j + 1 < mb) {
          T[jj + 1 + (size_t)mact * jj] = T[jj + (size_t)mact * (jj + 1)] = beta;
          RC(sd_k_scale_div(ctx, col(j + 1), w.p, nd, beta));
        }
      }
      std::vector<double> Tj((size_t)ja * ja), ev(ja), Z((size_t)ja * ja);
      for (int a = 0; a < ja; ++a)
        for (int b = 0; b < ja; ++b) Tj[b + (size_t)ja * a] = T[b + (size_t)mact * a];
      if (sd_sym_eig(ja, Tj.data(), ev.data(), Z.data())) return sd_set_err(ctx, SD_EINTERNAL, "Jacobi eigen-solver did not converge");
      scale = std::max(scale, std::max(std::fabs(ev[0]), std::fabs(ev[ja - 1])));
      scale_run = std::max(scale_run, scale);
      const double bl = broke ? 0.0 : beta;
      const int need = target - c;
      int nconv = 0;
      while (nconv < ja && nconv < need && std::fabs(bl * Z[(ja - 1) + (size_t)ja * nconv]) <= tol * scale) ++nconv;
      int kk = nconv;
      if (!broke) {
        const int buffer = std::min(8, std::max(2, (mact - need) / 3));
        kk = std::max(nconv, std::min(std::min(need + buffer, SD_EIGS_MAX_KEEP), mact - 1));
      }
      if (kk > 0) {
        SD_HIP(ctx, hipMemcpyAsync(Qd.p, Z.data(), sizeof(double) * (size_t)ja * kk, hipMemcpyHostToDevice, ctx->stream));
        RC(sd_k_basis_rotate(ctx, col(c), ld, nd, ja, Qd.p, kk));
        SD_HIP(ctx, hipStreamSynchronize(ctx->stream));
        ++info->restarts;
      }
      for (int i = 0; i < nconv; ++i) lam.push_back(ev[i]);
      c += nconv;
      if (broke) {
        if (c >= target) { l = 0; return SD_OK; }
        int ok = 0;
        if (c < N && c < mb) RC(fresh_start(&ok));
        if (!ok) { *exhausted = true; return SD_OK; }
      } else {
        l = kk - nconv;
        th.assign(ev.begin() + nconv, ev.begin() + kk);
        s.resize(l);
        for (int i = 0; i < l; ++i) s[i] = bl * Z[(ja - 1) + (size_t)ja * (nconv + i)];
        if (c + l >= mb) { *exhausted = c < target; return SD_OK; }      // no column left for the residual direction
        RC(sd_k_scale_div(ctx, col(c + l), w.p, nd, beta));
      }
    }
    return SD_OK;
  };

  // the start vector
  int ok = 0;
  if (psi0) RC(on_dev ? d2d(ctx, w.p, (const double *)psi0, nd) : h2d(ctx, w.p, psi0, nd));
  else RC(sd_k_fill_randn(ctx, w.p, nd, seed, 0));
  RC(seat_start(&ok));
  if (!ok) return sd_set_err(ctx, SD_EZERO, "starting vector has zero norm");
  bool stopped = false, exhausted = false;
  RC(run(nev, &stopped, &exhausted));
  // further copies of degenerate levels, levels the first sequence missed, and the first level above the window
  while (confirm && !stopped && !exhausted && c >= nev && c < N && (mb - c >= 2 || mb == N) && c < mb) {
    const int c0 = c;
    RC(fresh_start(&ok));
    if (!ok) break;
    RC(run(c0 + 1, &stopped, &exhausted));
    if (c == c0) break;
    std::vector<double> sorted(lam.begin(), lam.begin() + c0);
    std::sort(sorted.begin(), sorted.end());
    const double mu = lam.back();
    if (mu <= sorted[nev - 1] + tol * scale) continue;
    info->next_level = mu; info->have_next_level = 1;
    lam.pop_back(); c = c0;
    break;
  }

  // ascending order, normalised, with the true residuals
  std::vector<int> order(c);
  for (int i = 0; i < c; ++i) order[i] = i;
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return lam[a] < lam[b]; });
  const int nout = std::min(nev, c);
  if (c > nev) { info->next_level = lam[order[nev]]; info->have_next_level = 1; }   // a locked level beyond the window is the next one
  for (int i = 0; i < nout; ++i) {
    double *x = col(order[i]);
    int rc = 0;
    const double nrm = norm_dev(op, x, nd, &rc); RC(rc);
    RC(sd_k_scale_div(ctx, x, x, nd, nrm));
    sd_epi_args ea;
    RC(op.apply(dtype, w.p, x, SD_EPI_PLAIN, ea));
    RC(sd_k_sub2(ctx, w.p, x, nullptr, nd, lam[order[i]], 0.0));
    residuals[i] = norm_dev(op, w.p, nd, &rc); RC(rc);
    evals[i] = lam[order[i]];
    if (evecs) {
      double *dst = (double *)evecs + nd * (int64_t)i;
      RC(on_dev ? d2d(ctx, dst, x, nd) : d2h(ctx, dst, x, nd));
    }
  }
  SD_HIP(ctx, hipStreamSynchronize(ctx->stream));
  info->converged = nout;
  info->applies = ctx->n_applies - applies0;
  info->scale = scale;
  return SD_OK;
}

}  // namespace

extern "C" int sd_lanczos_eigenpairs(sd_ctx *ctx, const sd_model *m, int dtype, int nev, int basis_size, double tol, int64_t max_applies,
                                     int confirm, const void *psi0, uint64_t seed, double *evals, void *evecs, double *residuals,
                                     sd_eigs_info *info) { return abi_guard(ctx, [&]() -> int {
  Op op; RC(op.init(ctx, m, nullptr));
  return eigs_core(op, dtype, nev, basis_size, tol, max_applies, confirm, psi0, false, seed, evals, evecs, residuals, info);
}); }
extern "C" int sd_lanczos_eigenpairs_dev(sd_ctx *ctx, const sd_model *m, int dtype, int nev, int basis_size, double tol,
                                         int64_t max_applies, int confirm, const void *psi0, uint64_t seed, double *evals, void *evecs,
                                         double *residuals, sd_eigs_info *info) { return abi_guard(ctx, [&]() -> int {
  Op op; RC(op.init(ctx, m, nullptr));
  return eigs_core(op, dtype, nev, basis_size, tol, max_applies, confirm, psi0, true, seed, evals, evecs, residuals, info);
}); }

// the solver's kernels on the caller's device vectors (include/spindyn.h)
extern "C" int sd_basis_rotate_dev(sd_ctx *ctx, void *V, int64_t ld, int64_t n, int mm, const double *Q, int k) {
  return abi_guard(ctx, [&]() -> int {
  if (!ctx) return SD_EARG;
  if (mm < 1 || k < 1 || k > mm || mm > SD_EIGS_MAX_BASIS || k > SD_EIGS_MAX_KEEP)
    return sd_set_err(ctx, SD_EARG, "basis rotation: need 1 <= k <= m <= 128 and k <= 32");
  if (!V || !Q || n < 0 || ld < n) return sd_set_err(ctx, SD_EARG, "bad argument");
  SD_HIP(ctx, hipSetDevice(ctx->device));
  DBuf Qd; RC(Qd.alloc(ctx, (int64_t)mm * k));
  SD_HIP(ctx, hipMemcpyAsync(Qd.p, Q, sizeof(double) * (size_t)mm * k, hipMemcpyHostToDevice, ctx->stream));
  RC(sd_k_basis_rotate(ctx, (double *)V, ld, n, mm, Qd.p, k));
  SD_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return SD_OK;
}); }
extern "C" int sd_block_dots_dev(sd_ctx *ctx, int dtype, const void *V, int64_t ld, int ncols, const void *w, int64_t n, double *out) {
  return abi_guard(ctx, [&]() -> int {
  if (!ctx) return SD_EARG;
  if (dtype != SD_F64 && dtype != SD_C128) return sd_set_err(ctx, SD_EARG, "bad dtype");
  if (ncols < 1 || ncols > SD_EIGS_BLOCK_COLS || !V || !w || !out || n < 0 || ld < n) return sd_set_err(ctx, SD_EARG, "bad argument");
  SD_HIP(ctx, hipSetDevice(ctx->device));
  const int nc = dtype == SD_C128 ? 2 : 1;
  DBuf o; RC(o.alloc(ctx, 2 * SD_EIGS_BLOCK_COLS));
  RC(sd_k_block_dots(ctx, nc, (const double *)V, ld * nc, ncols, (const double *)w, n, o.p));
  RC(read_back(ctx, out, o.p, sizeof(double) * 2 * (size_t)ncols));
  return SD_OK;
}); }
extern "C" int sd_block_axpy_dev(sd_ctx *ctx, int dtype, void *w, const void *V, int64_t ld, int ncols, const double *coef, int64_t n) {
  return abi_guard(ctx, [&]() -> int {
  if (!ctx) return SD_EARG;
  if (dtype != SD_F64 && dtype != SD_C128) return sd_set_err(ctx, SD_EARG, "bad dtype");
  if (ncols < 1 || ncols > SD_EIGS_BLOCK_COLS || !V || !w || !coef || n < 0 || ld < n) return sd_set_err(ctx, SD_EARG, "bad argument");
  SD_HIP(ctx, hipSetDevice(ctx->device));
  const int nc = dtype == SD_C128 ? 2 : 1;
  DBuf cf; RC(cf.alloc(ctx, 2 * SD_EIGS_BLOCK_COLS));
  SD_HIP(ctx, hipMemcpyAsync(cf.p, coef, sizeof(double) * 2 * (size_t)ncols, hipMemcpyHostToDevice, ctx->stream));
  RC(sd_k_block_axpy(ctx, nc, (double *)w, (const double *)V, ld * nc, ncols, cf.p, n, nullptr));
  SD_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return SD_OK;
}); }

// ---- driven dynamics: H(t) = H0 + sum_k f_k(t) D_k with diagonal drives ----
namespace {

int drive_table(sd_ctx *ctx, const sd_model *m, const sd_drive *drives, int K, const double *coef, sd_drive_table &tb) {
  std::string err;
  const int rc = sd_drive_build(m, drives, K, coef, tb, err);
  return rc ? sd_set_err(ctx, rc, err) : SD_OK;
}

// out = (sum_k coef[k] D_k) psi (+ y), or with_h0: out = (H0 + sum_k coef[k] D_k) psi with the built-in H0 (operator level, as
// sd_apply: a caller's operator may call it)
int drive_apply_core(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi, int64_t n, const sd_drive *drives, int K,
                     const double *coef, const void *y, void *out, bool with_h0, bool on_dev) {
  Op op; RC(op.init(ctx, m, nullptr));
  if (dtype != SD_F64 && dtype != SD_C128) return sd_set_err(ctx, SD_EARG, "dtype must be SD_F64 or SD_C128");
  if (K > 0 && !coef) return sd_set_err(ctx, SD_EARG, "null coefficients");
  const double none = 0.0;
  sd_drive_table tb;
  RC(drive_table(ctx, m, drives, K, coef ? coef : &none, tb));
  if (n != m->N) return sd_set_err(ctx, SD_EDIM, "vector length does not match the basis dimension");
  if (!psi || !out) return sd_set_err(ctx, SD_EARG, "null argument");
  if (on_dev && out == psi) return sd_set_err(ctx, SD_EARG, "out must not alias psi");
  DevIn in;
  DevOut o;
  RC(in.stage(ctx, dtype, psi, on_dev, n));
  RC(o.open(ctx, out, on_dev, vec_doubles(dtype, n)));
  const double *yd = (const double *)y;
  if (!on_dev && y) { RC(h2d(ctx, o.p, y, vec_doubles(dtype, n))); yd = o.p; }     // the host form's y rides in the result block
  if (with_h0) {
    op.use_callback = false;
    op.drive = &tb;
    RC(op.apply(dtype, o.p, in.p, SD_EPI_PLAIN, sd_epi_args()));
  } else {
    RC(sd_launch_drive_epilogue(ctx, m, dtype, o.p, yd, in.p, SD_EPI_PLAIN, sd_epi_args(), tb));
  }
  return o.close(true);                                    // no pool block is in flight: see the table of DESIGN.md 4.5
}

// psi <- exp(-i tau_s (H0 + sum_k coef[s K + k] D_k)) psi for s = 0 .. n_stages-1 by krylov_evolve_core on the driven operator, the
// state on the device between stages.  The work vectors of a stage go back to the context's pool and the next stage takes the same
// blocks: they are allocated once.  A stage without a table (K == 0, or every coefficient exactly zero) runs the built-in path.
int driven_evolve_core(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi0, int64_t n, const sd_drive *drives, int K,
                       int n_stages, const double *tau, const double *coef, int kry_m, void *psit, bool on_dev, sd_driven_info *info) {
  Op op; RC(op.init(ctx, m, nullptr));
  if (info) { info->stages = 0; info->applies = 0; info->min_beta = INFINITY; }
  if (!psi0 || !psit) return sd_set_err(ctx, SD_EARG, "null vector");
  if (n_stages < 1 || !tau) return sd_set_err(ctx, SD_EARG, "a driven evolution needs at least one stage and its durations");
  if (K > 0 && !coef) return sd_set_err(ctx, SD_EARG, "null coefficients");
  if (dtype != SD_F64 && dtype != SD_C128) return sd_set_err(ctx, SD_EARG, "bad dtype");
  if (n != op.n) return sd_set_err(ctx, SD_EDIM, "vector length does not match the basis dimension");
  if (kry_m < 1) return sd_set_err(ctx, SD_EARG, "kry_m must be >= 1");
  sd_drive_table tb;
  RC(drive_table(ctx, m, drives, K, nullptr, tb));                       // the limits, before anything runs
  for (int s = 0; s < n_stages; ++s) {
    if (!std::isfinite(tau[s])) return sd_set_err(ctx, SD_EARG, "a stage duration is not finite");
    for (int k = 0; k < K; ++k)
      if (!std::isfinite(coef[(size_t)s * K + k])) return sd_set_err(ctx, SD_EARG, "a stage coefficient is not finite");
  }
  DevIn in;
  DevOut state;
  RC(in.stage(ctx, dtype, psi0, on_dev, n));
  RC(state.open(ctx, psit, on_dev, 2 * n));
  double *cur = state.p;
  const int64_t applies0 = ctx->n_applies;
  double min_beta = INFINITY;
  for (int s = 0; s < n_stages; ++s) {
    const double *c = K > 0 ? coef + (size_t)s * K : nullptr;
    bool driven = false;
    for (int k = 0; k < K; ++k) driven = driven || c[k] != 0.0;
    op.drive = nullptr;
    if (driven) { RC(drive_table(ctx, m, drives, K, c, tb)); op.drive = &tb; }
    RC(krylov_evolve_core(op, s == 0 ? dtype : SD_C128, s == 0 ? in.p : cur, n, tau[s], kry_m, cur, true, nullptr, &min_beta));
    if (info) { info->stages = s + 1; info->applies = ctx->n_applies - applies0; info->min_beta = min_beta; }
  }
  op.drive = nullptr;
  return state.close(false);                               // krylov_evolve_core has drained the stream
}

// ---- hopping drives on top: H(t) = H0 + sum_k c_k(t) O_k, every O_k diagonal or a hopping drive ----

int hop_table(sd_ctx *ctx, const sd_model *m, const sd_hop_drive *hops, int KH, int K, const double *coef, sd_hop_table &ht) {
  std::string err;
  const int rc = sd_hop_build(m, hops, KH, K, coef, ht, err);
  return rc ? sd_set_err(ctx, rc, err) : SD_OK;
}

// The device slot of a call's hop table, one block of the context's pool: SD_HOP_MAX_BONDS site words, then as many (x, y) pairs.
// The words go up when the set of switched-on drives changes (once per call unless a coefficient passes through exactly zero), the
// weights with every table.  Every user of the slot drains the stream before the next upload and before the block goes back.
struct HopSlot {
  DBuf buf;
  HopDev dev;
  uint32_t words_of = ~0u;                                 // the switched-on drives whose words are on the device
  int upload(sd_ctx *ctx, const sd_hop_table &ht, int KH, const double *coef) {
    if (!buf.p) {
      RC(buf.alloc_bytes(ctx, SD_HOP_MAX_BONDS * (sizeof(uint32_t) + 2 * sizeof(double))));
      dev.bits = (const uint32_t *)buf.p;
      dev.xy = (const double *)((const char *)buf.p + SD_HOP_MAX_BONDS * sizeof(uint32_t));
    }
    uint32_t on = 0;
    for (int k = 0; k < KH; ++k) on |= (coef[k] != 0.0 ? 1u : 0u) << k;
    dev.n = ht.n;
    dev.complex_form = ht.complex_form;
    if (ht.n == 0) return SD_OK;
    if (on != words_of) { RC(sd_xfer_h2d(ctx, (void *)dev.bits, ht.bits, sizeof(uint32_t) * (size_t)ht.n)); words_of = on; }
    return sd_xfer_h2d(ctx, (void *)dev.xy, ht.xy, 2 * sizeof(double) * (size_t)ht.n);
  }
};

// with_h0: out = (H0 + sum_k coef[k] D_k + sum_k coef[K + k] B_k) psi with the built-in H0 (operator level); else K == 0 and
// out = (sum_k coef[k] B_k) psi (+ y).  A list without a term in effect runs drive_apply_core's calls.
int hop_apply_core(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi, int64_t n, const sd_drive *drives, int K,
                   const sd_hop_drive *hops, int KH, const double *coef, const void *y, void *out, bool with_h0, bool on_dev) {
  Op op; RC(op.init(ctx, m, nullptr));
  if (dtype != SD_F64 && dtype != SD_C128) return sd_set_err(ctx, SD_EARG, "dtype must be SD_F64 or SD_C128");
  if (K < 0 || KH < 0) return sd_set_err(ctx, SD_EARG, "negative drive count");
  if (K + KH > 0 && !coef) return sd_set_err(ctx, SD_EARG, "null coefficients");
  sd_drive_table tb;
  sd_hop_table ht;
  const double none = 0.0;
  RC(drive_table(ctx, m, drives, K, K > 0 ? coef : &none, tb));
  RC(hop_table(ctx, m, hops, KH, K, KH > 0 ? coef + K : nullptr, ht));
  if (KH == 0) ht.n = 0;
  if (ht.complex_form && dtype != SD_C128)
    return sd_set_err(ctx, SD_EARG, "a hopping drive with complex weights needs a ComplexF64 vector");
  if (n != m->N) return sd_set_err(ctx, SD_EDIM, "vector length does not match the basis dimension");
  if (!psi || !out) return sd_set_err(ctx, SD_EARG, "null argument");
  const size_t bytes = sizeof(double) * (size_t)vec_doubles(dtype, n);
  if (on_dev && (ranges_overlap(out, bytes, psi, bytes) || (y && ranges_overlap(y, bytes, psi, bytes))))
    return sd_set_err(ctx, SD_EARG, "out and y must not share memory with psi");
  if (ht.n == 0 && with_h0) return drive_apply_core(ctx, m, dtype, psi, n, drives, K, coef, nullptr, out, true, on_dev);
  HopSlot slot;
  RC(slot.upload(ctx, ht, KH, coef ? coef + K : nullptr));
  DevIn in;
  DevOut o;
  RC(in.stage(ctx, dtype, psi, on_dev, n));
  RC(o.open(ctx, out, on_dev, vec_doubles(dtype, n)));
  const double *yd = (const double *)y;
  if (!on_dev && y) { RC(h2d(ctx, o.p, y, vec_doubles(dtype, n))); yd = o.p; }     // the host form's y rides in the result block
  if (with_h0) {
    op.use_callback = false;
    op.drive = K > 0 ? &tb : nullptr;
    op.hop = &slot.dev;
    RC(op.apply(dtype, o.p, in.p, SD_EPI_PLAIN, sd_epi_args()));
  } else {
    RC(sd_launch_hop_drive_epilogue(ctx, m, dtype, o.p, yd, in.p, SD_EPI_PLAIN, sd_epi_args(), nullptr, slot.dev.n, slot.dev.complex_form,
                                    slot.dev.bits, slot.dev.xy));
  }
  return o.close(true);                                    // the slot goes back to the pool: nothing may still read it
}

// driven_evolve_core with hopping drives: coef[n_stages x (K + KH)], the diagonal columns first.  A stage without a hop term in
// effect runs driven_evolve_core's calls.  Complex form: an SD_F64 psi0 is promoted once, before the first stage.
int driven_hop_evolve_core(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi0, int64_t n, const sd_drive *drives, int K,
                           const sd_hop_drive *hops, int KH, int n_stages, const double *tau, const double *coef, int kry_m, void *psit,
                           bool on_dev, sd_driven_info *info) {
  if (KH == 0) return driven_evolve_core(ctx, m, dtype, psi0, n, drives, K, n_stages, tau, coef, kry_m, psit, on_dev, info);
  Op op; RC(op.init(ctx, m, nullptr));
  if (info) { info->stages = 0; info->applies = 0; info->min_beta = INFINITY; }
  if (!psi0 || !psit) return sd_set_err(ctx, SD_EARG, "null vector");
  if (n_stages < 1 || !tau) return sd_set_err(ctx, SD_EARG, "a driven evolution needs at least one stage and its durations");
  if (K < 0 || KH < 0) return sd_set_err(ctx, SD_EARG, "negative drive count");
  if (!coef) return sd_set_err(ctx, SD_EARG, "null coefficients");
  if (dtype != SD_F64 && dtype != SD_C128) return sd_set_err(ctx, SD_EARG, "bad dtype");
  if (n != op.n) return sd_set_err(ctx, SD_EDIM, "vector length does not match the basis dimension");
  if (kry_m < 1) return sd_set_err(ctx, SD_EARG, "kry_m must be >= 1");
  sd_drive_table tb;
  sd_hop_table ht;
  RC(drive_table(ctx, m, drives, K, nullptr, tb));                       // the limits, before anything runs
  RC(hop_table(ctx, m, hops, KH, K, nullptr, ht));
  const bool complex_form = ht.complex_form != 0;
  const int KT = K + KH;
  for (int s = 0; s < n_stages; ++s) {
    if (!std::isfinite(tau[s])) return sd_set_err(ctx, SD_EARG, "a stage duration is not finite");
    for (int k = 0; k < KT; ++k)
      if (!std::isfinite(coef[(size_t)s * KT + k])) return sd_set_err(ctx, SD_EARG, "a stage coefficient is not finite");
  }
  DevIn in;
  DevOut state;
  HopSlot slot;
  RC(in.stage(ctx, dtype, psi0, on_dev, n));
  RC(state.open(ctx, psit, on_dev, 2 * n));
  double *cur = state.p;
  bool started = false;                                                  // cur holds the state (ComplexF64)
  if (complex_form && dtype == SD_F64) { RC(sd_k_promote(ctx, cur, in.p, 1, n)); started = true; }
  const int64_t applies0 = ctx->n_applies;
  double min_beta = INFINITY;
  for (int s = 0; s < n_stages; ++s) {
    const double *c = coef + (size_t)s * KT;
    bool driven = false;
    for (int k = 0; k < K; ++k) driven = driven || c[k] != 0.0;
    op.drive = nullptr;
    op.hop = nullptr;
    if (driven) { RC(drive_table(ctx, m, drives, K, c, tb)); op.drive = &tb; }
    RC(hop_table(ctx, m, hops, KH, K, c + K, ht));
    if (ht.n > 0) { RC(slot.upload(ctx, ht, KH, c + K)); op.hop = &slot.dev; }
    RC(krylov_evolve_core(op, started ? SD_C128 : dtype, started ? cur : in.p, n, tau[s], kry_m, cur, true, nullptr, &min_beta));
    started = true;
    if (info) { info->stages = s + 1; info->applies = ctx->n_applies - applies0; info->min_beta = min_beta; }
  }
  op.drive = nullptr;
  op.hop = nullptr;
  return state.close(false);                               // krylov_evolve_core has drained the stream
}

}  // namespace

extern "C" int sd_hop_apply(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi_host, int64_t n, const sd_hop_drive *hops, int KH,
                            const double *coef, const void *y_host, void *out_host) { return abi_guard(ctx, [&]() -> int {
  return hop_apply_core(ctx, m, dtype, psi_host, n, nullptr, 0, hops, KH, coef, y_host, out_host, false, false);
}); }
extern "C" int sd_hop_apply_dev(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi_dev, int64_t n, const sd_hop_drive *hops, int KH,
                                const double *coef, const void *y_dev, void *out_dev) { return abi_guard(ctx, [&]() -> int {
  return hop_apply_core(ctx, m, dtype, psi_dev, n, nullptr, 0, hops, KH, coef, y_dev, out_dev, false, true);
}); }
extern "C" int sd_driven_hop_apply(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi_host, int64_t n, const sd_drive *drives,
                                   int K, const sd_hop_drive *hops, int KH, const double *coef, void *out_host) {
  return abi_guard(ctx, [&]() -> int {
  return hop_apply_core(ctx, m, dtype, psi_host, n, drives, K, hops, KH, coef, nullptr, out_host, true, false);
}); }
extern "C" int sd_driven_hop_apply_dev(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi_dev, int64_t n, const sd_drive *drives,
                                       int K, const sd_hop_drive *hops, int KH, const double *coef, void *out_dev) {
  return abi_guard(ctx, [&]() -> int {
  return hop_apply_core(ctx, m, dtype, psi_dev, n, drives, K, hops, KH, coef, nullptr, out_dev, true, true);
}); }
extern "C" int sd_driven_hop_evolve(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi0_host, int64_t n, const sd_drive *drives,
                                    int K, const sd_hop_drive *hops, int KH, int n_stages, const double *tau, const double *coef,
                                    int kry_m, void *psit_host, sd_driven_info *info) { return abi_guard(ctx, [&]() -> int {
  return driven_hop_evolve_core(ctx, m, dtype, psi0_host, n, drives, K, hops, KH, n_stages, tau, coef, kry_m, psit_host, false, info);
}); }
extern "C" int sd_driven_hop_evolve_dev(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi0_dev, int64_t n, const sd_drive *drives,
                                        int K, const sd_hop_drive *hops, int KH, int n_stages, const double *tau, const double *coef,
                                        int kry_m, void *psit_dev, sd_driven_info *info) { return abi_guard(ctx, [&]() -> int {
  return driven_hop_evolve_core(ctx, m, dtype, psi0_dev, n, drives, K, hops, KH, n_stages, tau, coef, kry_m, psit_dev, true, info);
}); }


extern "C" int sd_diag_apply(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi_host, int64_t n, const sd_drive *drives, int K,
                             const double *coef, const void *y_host, void *out_host) { return abi_guard(ctx, [&]() -> int {
  return drive_apply_core(ctx, m, dtype, psi_host, n, drives, K, coef, y_host, out_host, false, false);
}); }
extern "C" int sd_diag_apply_dev(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi_dev, int64_t n, const sd_drive *drives, int K,
                                 const double *coef, const void *y_dev, void *out_dev) { return abi_guard(ctx, [&]() -> int {
  return drive_apply_core(ctx, m, dtype, psi_dev, n, drives, K, coef, y_dev, out_dev, false, true);
}); }
extern "C" int sd_driven_apply(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi_host, int64_t n, const sd_drive *drives, int K,
                               const double *coef, void *out_host) { return abi_guard(ctx, [&]() -> int {
  return drive_apply_core(ctx, m, dtype, psi_host, n, drives, K, coef, nullptr, out_host, true, false);
}); }
extern "C" int sd_driven_apply_dev(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi_dev, int64_t n, const sd_drive *drives,
                                   int K, const double *coef, void *out_dev) { return abi_guard(ctx, [&]() -> int {
  return drive_apply_core(ctx, m, dtype, psi_dev, n, drives, K, coef, nullptr, out_dev, true, true);
}); }
extern "C" int sd_driven_evolve(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi0_host, int64_t n, const sd_drive *drives, int K,
                                int n_stages, const double *tau, const double *coef, int kry_m, void *psit_host,
                                sd_driven_info *info) { return abi_guard(ctx, [&]() -> int {
  return driven_evolve_core(ctx, m, dtype, psi0_host, n, drives, K, n_stages, tau, coef, kry_m, psit_host, false, info);
}); }
extern "C" int sd_driven_evolve_dev(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi0_dev, int64_t n, const sd_drive *drives,
                                    int K, int n_stages, const double *tau, const double *coef, int kry_m, void *psit_dev,
                                    sd_driven_info *info) { return abi_guard(ctx, [&]() -> int {
  return driven_evolve_core(ctx, m, dtype, psi0_dev, n, drives, K, n_stages, tau, coef, kry_m, psit_dev, true, info);
}); }
