/*
 * spindyn.h -- C ABI of libspindyn.so, the MI355X-native (gfx950 HIP) engine for
 * the matrix-free spin-1/2 Hamiltonian apply H|psi> and the recursions built on
 * it (Lanczos / Krylov / Chebyshev / KPM).
 *
 * The reference (javahedi/SpinDynamics.jl) has no FFI layer; its de-facto
 * operator seam is the Julia callable  applyH!(out, psi, model)  handed to every
 * solver (src/Lanczos.jl:27-29,87-89,196-198,255; src/TimeEvolution/Krylov.jl:
 * 136-137; src/TimeEvolution/Chebyshev.jl:61-62; src/Hamiltonian.jl:286-288) and
 * supplied by PublicAPI as Hamiltonian.apply_H! (src/PublicAPI.jl:28,62,70,79).
 * Each entry point below names the reference function it replaces; the Julia
 * `ccall` stubs a maintainer would add are in INTEGRATION.md and julia/.
 *
 * Conventions
 *  - plain C types only; every function returns an int status (SD_OK == 0).
 *  - dtype: SD_F64 (Float64) or SD_C128 (ComplexF64, interleaved re,im).
 *  - sites are 1-based as in the reference's bond tuples (i, j, J).
 *  - basis indices are 0-based at this ABI (reference index = idx0 + 1).
 *  - "host" pointers are caller-owned host memory, only touched during the call.
 *    "dev" pointers are device (HIP) pointers on the context's device.
 *  - a sd_model is immutable once set up -- creation, then at most one sd_model_set_shard[_mode] call before any other
 *    thread sees it -- and may then be shared between threads; everything a call may change (stream, scratch, the
 *    kpm switches, a caller's operator) lives in the sd_ctx, which must not be used concurrently: one context per thread.
 */
#ifndef SPINDYN_H
#define SPINDYN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* status codes.  Mapping to the reference's Julia exceptions:
 *   SD_EARG   -> ArgumentError      (src/Basis.jl:10-16, src/SpinModel.jl:80, src/PublicAPI.jl:34,87,152)
 *   SD_EDIM   -> DimensionMismatch / AssertionError (src/Hamiltonian.jl:63-66,220,289)
 *   SD_EZERO  -> error("starting vector has zero norm") (src/Lanczos.jl:210-212)
 */
#define SD_OK 0
#define SD_EARG 1
#define SD_EDIM 2
#define SD_EZERO 3
#define SD_ENOMEM 4
#define SD_EHIP 5
#define SD_ENODEV 6
#define SD_EINTERNAL 7
#define SD_ECOMM 8   /* RCCL / exchange callback failure */

#define SD_F64 1
#define SD_C128 2

/* KPM damping kernels (src/KPM_Sqw.jl:131-145); anything else = no damping */
#define SD_KERNEL_JACKSON 0
#define SD_KERNEL_LORENTZ 1
#define SD_KERNEL_NONE 2
/* broadening for the Lanczos spectral function (src/LanczosSqw.jl:29-40) */
#define SD_BROADEN_LORENTZ 0
#define SD_BROADEN_GAUSS 1

typedef struct sd_ctx sd_ctx;
typedef struct sd_model sd_model;

/* ---- library / context ------------------------------------------------ */
const char *sd_version(void);
/* number of HIP devices visible (0 when there is no GPU; never fails) */
int sd_device_count(void);
/* Creates a context on HIP device `device` with its own stream.  Fails with
 * SD_ENODEV when no GPU is present: there is no CPU fallback in this library. */
int sd_ctx_create(int device, sd_ctx **out);
void sd_ctx_destroy(sd_ctx *ctx);
/* Use an externally owned hipStream_t (e.g. torch's current stream) for all
 * launches of this context; NULL restores the context's own stream. */
int sd_ctx_set_stream(sd_ctx *ctx, void *hip_stream);
/* Chebyshev moments (sd_kpm_moments, sd_kpm_sqw): on != 0 (default) computes two moments per apply from
 * mu_2n = 2<v_n|v_n> - mu_0, mu_2n+1 = 2Re<v_n|v_n+1> - mu_1 (v_n = T_n(H~)phi); on == 0 runs the reference's loop
 * (src/KPM_Sqw.jl:103-124), one moment <phi|v_k> per apply.  Same moments up to rounding. */
int sd_ctx_set_kpm_doubling(sd_ctx *ctx, int on);
/* sd_kpm_sqw / sd_kpm_sqw_sharded / sd_lanczos_sqw with a REAL psi0 (Float64, or ComplexF64 whose imaginary parts are all zero -- checked on
 * the device): on != 0 (default) computes the moments once per pair of momenta (q, 2 pi - q) of the list and copies the row,
 * because H is real and phi_{2pi-q} = conj(phi_q) gives the same moments (and the same Lanczos coefficients); on == 0 runs every
 * q on its own, as the reference does (src/KPM_Sqw.jl:218-252, src/LanczosSqw.jl:63-77).  The copied row differs from a recomputed one by the rounding of exp(iqr) only (<= 1e-13
 * on S).  Never used with a caller's operator (sd_ctx_set_apply_callback). */
int sd_ctx_set_kpm_pair_q(sd_ctx *ctx, int on);
/* sd_kpm_sqw / sd_lanczos_sqw on one GPU: the reference threads over the momenta (src/KPM_Sqw.jl:218, src/LanczosSqw.jl:65).  on != 0
 * (default; env SD_Q_BATCH=0 changes the default) lets the momenta's vectors share every launch of the recursion where a single
 * vector cannot fill the chip (vectors of at most 2^22 rows, tiled plans): one batched apply per step for all momenta.  Each
 * momentum sees exactly the arithmetic of a recursion of its own -- S(q, w) is bit-identical; on == 0: one momentum at a time. */
int sd_ctx_set_q_batch(sd_ctx *ctx, int on);
/* sd_lanczos_groundstate re-orthogonalises H v_j against v_1 .. v_{j-1} (src/Lanczos.jl:116-124).  on != 0 (default): in blocks
 * of 8 columns -- the coefficients of a block are its dots with w as it stands when the block begins (classical Gram-Schmidt
 * inside a block, modified between blocks), one pass over w per block instead of per column.  With v_k orthonormal to rounding
 * the coefficients differ from the reference's column-by-column chain by O(eps |coeff|): E0 to 1e-12, the vector to 1e-8.
 * on == 0: the reference's order, column by column. */
int sd_ctx_set_gs_blocked(sd_ctx *ctx, int on);
/* Operator applications (built-in H or the caller's operator) that the recursion-level entry points have queued on this
 * context since it was created: one per recursion step.  The difference across a call says how many steps it really ran
 * (e.g. how soon a queued Lanczos recursion noticed a breakdown). */
int64_t sd_ctx_apply_count(const sd_ctx *ctx);
/* A context keeps between calls: the device staging buffers of the host-pointer operator calls (sd_apply,
 * sd_apply_rescaled: two vectors), its reduction scratch, and the work vectors of the recursion-level calls (a pool of at
 * most SD_POOL_MAX_GB = 96 GB by default: a hipMalloc/hipFree pair costs 0.3-0.6 ms whatever the size, as long as
 * 15-30 recursion steps of a small system -- the role of the reference's `workspace` argument,
 * src/TimeEvolution/Chebyshev.jl:61-66).  This call frees all
 * of them; they are re-created on demand. */
int sd_ctx_release_scratch(sd_ctx *ctx);
int sd_ctx_synchronize(sd_ctx *ctx);
/* last error text of this context ("" if none); valid until the next call */
const char *sd_last_error(const sd_ctx *ctx);
/* text for a status code */
const char *sd_status_string(int status);

/* ---- model (replaces SpinModel.Model, src/SpinModel.jl:6-38) ------------ */
/* nup = -1 selects the full 2^L basis (`nup === nothing`).  states/idxmap are
 * never passed: the basis order of build_sector_basis (src/Basis.jl:37-53) is
 * reproduced from closed-form combinatorial ranking.  ctx may be NULL: the
 * model is then host-only (basis queries work, device applies do not). */
int sd_model_create(sd_ctx *ctx, int L, int nup,
                    int n_hop, const int *hop_i, const int *hop_j, const double *hop_J,
                    int n_zz, const int *zz_i, const int *zz_j, const double *zz_J,
                    const double *field /* L entries or NULL */, sd_model **out);
/* XXZChain(L; Jxy, Jz, hz, nup, boundary) -- src/SpinModel.jl:63-90.
 * boundary: 0 = :open, 1 = :periodic; anything else -> SD_EARG. */
int sd_xxz_chain(sd_ctx *ctx, int L, double Jxy, double Jz, double hz, int nup, int boundary,
                 sd_model **out);
void sd_model_destroy(sd_model *m);
int64_t sd_model_dim(const sd_model *m);      /* length(model.states) */
int sd_model_L(const sd_model *m);
int sd_model_nup(const sd_model *m);          /* -1 for the full basis */
/* which device path the apply takes: 0 generic (per-row rank/unrank), 1 tiled (prefix-run tiles, LDS staged suffix
 * hops), 2 full-basis tiles of 2^10 rows */
int sd_model_path(const sd_model *m);
/* model.states[start .. start+count)  (host computation, 0-based start) */
int sd_model_states(const sd_model *m, int64_t start, int64_t count, uint64_t *states_out);
/* get(model.idxmap, state, 0) - 1 : 0-based index of each state, -1 if absent */
int sd_model_rank(const sd_model *m, const uint64_t *states, int64_t n, int64_t *idx_out);

/* ---- operator level (replaces applyH!(out, psi, model)) ----------------- */
/* apply_H!   src/Hamiltonian.jl:211-273.  out is overwritten, must not alias
 * psi, n must equal sd_model_dim (SD_EDIM otherwise). */
int sd_apply(sd_ctx *ctx, const sd_model *m, int dtype, void *out_host, const void *psi_host, int64_t n);
int sd_apply_dev(sd_ctx *ctx, const sd_model *m, int dtype, void *out_dev, const void *psi_dev, int64_t n);
/* apply_rescaled_H!   src/Hamiltonian.jl:286-301:  out = (H psi - b psi) / a, fused in one pass */
int sd_apply_rescaled(sd_ctx *ctx, const sd_model *m, int dtype, void *out_host, const void *psi_host,
                      int64_t n, double a, double b);
int sd_apply_rescaled_dev(sd_ctx *ctx, const sd_model *m, int dtype, void *out_dev, const void *psi_dev,
                          int64_t n, double a, double b);
/* The operator as a callable at the recursion level.  Every reference solver takes `applyH!` as an argument
 * (src/Lanczos.jl:27-29, src/TimeEvolution/Chebyshev.jl:61-64, src/KPM_Sqw.jl:95-98, ...).  With a callback installed in a
 * context, every recursion entry point called on THAT context (lanczos_*, energy_bounds, krylov / chebyshev evolve, kpm_*,
 * *_sqw, and their _dev / _sharded forms) calls fn for out <- H psi instead of the built-in kernel and applies its own fused
 * step (rescale, recurrence, dot products) in a second, elementwise pass.  fn gets DEVICE pointers of n_local elements of
 * `dtype` and the HIP stream the call must be ordered on (enqueue there, or finish before returning); out never aliases psi;
 * a nonzero return aborts the call with SD_ECOMM.  The operator-level entries (sd_apply*, sd_apply_sharded*) always run the
 * built-in operator, so fn may call them -- on a sharded model sd_apply_sharded, which includes the halo exchange.
 * fn == NULL restores the built-in operator.  The callback belongs to the context, not to the model: models stay immutable
 * and shareable, and another thread's recursions (on its own context) are unaffected. */
typedef int (*sd_apply_fn)(void *user, int dtype, void *out_dev, const void *psi_dev, int64_t n_local, void *hip_stream);
int sd_ctx_set_apply_callback(sd_ctx *ctx, sd_apply_fn fn, void *user);
/* Sz_q_vector   src/Hamiltonian.jl:307-337.  phi_out is always ComplexF64. */
int sd_szq(sd_ctx *ctx, const sd_model *m, int dtype_in, const void *psi0_host, int64_t n, double q,
           void *phi_out_host);
int sd_szq_dev(sd_ctx *ctx, const sd_model *m, int dtype_in, const void *psi0_dev, int64_t n, double q,
               void *phi_out_dev);

/* Fused Chebyshev term on device vectors (all ComplexF64, length n):
 *   phi_next = 2*(H phi_curr - b phi_curr)/a - phi_prev ;  psi_t += c * phi_next
 * = one iteration of src/TimeEvolution/Chebyshev.jl:110-121 in a single pass. */
int sd_cheb_step_dev(sd_ctx *ctx, const sd_model *m, void *phi_next_dev, const void *phi_curr_dev,
                     const void *phi_prev_dev, void *psi_t_dev, int64_t n, double a, double b,
                     double c_re, double c_im);

/* Timed loop for benchmarks: `reps` applies out<-H psi (ping-pong between the
 * two buffers) bracketed by hipEvents on the context's stream; returns the
 * average milliseconds per apply.  Both buffers are device pointers. */
int sd_bench_apply_dev(sd_ctx *ctx, const sd_model *m, int dtype, void *buf_a_dev, void *buf_b_dev,
                       int64_t n, int reps, float *ms_per_apply);

/* ---- recursion level ---------------------------------------------------- */
/* All vectors are host arrays; the recursion runs entirely on the device
 * (apply kernel + BLAS-1 kernels), only scalars cross per iteration.
 * psi0 arguments marked "or NULL" are drawn from the library's counter-based
 * normal generator keyed by `seed` when NULL (the reference uses Julia's
 * randn, whose stream cannot be reproduced outside Julia). */

/* lanczos_extremal   src/Lanczos.jl:27-84   (ComplexF64 start vector) */
int sd_lanczos_extremal(sd_ctx *ctx, const sd_model *m, int lanc_m, double tol,
                        const void *psi0_c128_host /* or NULL */, uint64_t seed, int negate,
                        double *emin, double *emax);
/* estimate_energy_bounds   src/Lanczos.jl:255-271 */
int sd_energy_bounds(sd_ctx *ctx, const sd_model *m, int lanc_m,
                     const void *psi0_a_c128_host /* or NULL */, const void *psi0_b_c128_host /* or NULL */,
                     uint64_t seed, double *emin, double *emax);
/* lanczos_groundstate   src/Lanczos.jl:87-181   (Float64, full re-orthogonalisation) */
int sd_lanczos_groundstate(sd_ctx *ctx, const sd_model *m, int lanc_m, double tol, double orth_tol,
                           const double *psi0_host /* or NULL */, uint64_t seed,
                           double *E0, double *psi_gs_host /* n doubles */, int *m_actual);
/* The lowest nev eigenpairs by thick-restart Lanczos (Wu and Simon) in bounded memory: basis_size + 1 device vectors of `dtype`
 * (not in the reference, which stops at the ground state).
 *   Lanczos with full re-orthogonalisation (classical Gram-Schmidt applied twice, in blocks of 8 columns) fills basis_size columns;
 *   the projected matrix -- arrowhead plus tridiagonal after a restart -- is solved with sd_sym_eig; the lowest `keep` Ritz vectors
 *   of the active block are formed in place by one rotation (sd_basis_rotate_dev) and the residual direction follows them.
 *   keep = (pairs still wanted) + buffer, buffer = a third of the free columns, at least 2 and at most 8; keep <= 32.
 *   Ritz pair i is converged when |beta_m Z[m-1, i]| <= tol * scale, scale = the largest |theta| seen so far; converged pairs are
 *   locked from the bottom up: their columns stay in the basis as deflation and are not rotated again.
 *   Breakdown (beta <= 1e-12 * scale): the block is an invariant subspace and its pairs are exact; while pairs are missing and fewer
 *   than n columns are locked the solver goes on from a fresh seeded random vector orthogonalised twice against the locked columns.
 *   confirm != 0: a single start vector holds one direction per eigenspace, so once nev pairs are locked a new sequence starts from
 *   a fresh seeded random vector orthogonal to the locked set and runs until its lowest Ritz value has converged.  A value at or
 *   below the nev-th level + tol * scale is locked too (a further copy of a degenerate level, or a level the first sequence missed)
 *   and the step repeats; a value above it is reported as info->next_level (the first level above the window) and ends the call.
 *   confirm == 0 skips this: for operators that are projectors onto a sector, which a random vector would leave.
 * evals[nev], residuals[nev] (|H x_i - evals[i] x_i| by one apply each), evecs (n x nev column-major, of `dtype`; or NULL): the
 * lowest min(nev, locked) pairs in ascending order; info->converged of them are valid.  max_applies (<= 0: no bound) bounds the
 * applies of the iteration; when it is reached the pairs locked so far come back with converged < nev and status SD_OK.  The
 * applies of the residuals are counted in info->applies on top.  dtype SD_F64 needs the built-in operator of a real model; a
 * caller's operator (sd_ctx_set_apply_callback) may be either dtype.  The same call gives the same bits.
 * SD_EARG (with the reason in sd_last_error): nev < 1, nev > min(n, 24), basis_size < nev + 3 while n allows more, basis_size > 128,
 * a sharded model, NULL outputs.  basis_size is clamped to n.  SD_ENOMEM: the basis does not fit; the context stays usable.
 * _dev: psi0 and evecs are device pointers. */
#define SD_EIGS_MAX_BASIS 128
#define SD_EIGS_MAX_KEEP 32
#define SD_EIGS_MAX_NEV 24
typedef struct sd_eigs_info {
  int converged;            /* pairs returned (<= nev) */
  int restarts;             /* Ritz rotations of the basis */
  int64_t applies;          /* operator applications of the call, residuals included */
  int basis_size;           /* after clamping to n */
  int workspace_vectors;    /* device vectors of n elements the call held */
  double next_level;        /* first level above the returned ones (confirm != 0 and found) */
  int have_next_level;
  double scale;             /* largest |Ritz value| seen: the estimate of |H| the tolerances are relative to */
} sd_eigs_info;
int sd_lanczos_eigenpairs(sd_ctx *ctx, const sd_model *m, int dtype, int nev, int basis_size, double tol, int64_t max_applies,
                          int confirm, const void *psi0_host /* or NULL */, uint64_t seed, double *evals,
                          void *evecs_host /* or NULL */, double *residuals, sd_eigs_info *info);
int sd_lanczos_eigenpairs_dev(sd_ctx *ctx, const sd_model *m, int dtype, int nev, int basis_size, double tol, int64_t max_applies,
                              int confirm, const void *psi0_dev /* or NULL */, uint64_t seed, double *evals,
                              void *evecs_dev /* or NULL */, double *residuals, sd_eigs_info *info);
/* The solver's three streaming kernels on device vectors (kernels_eigs.hip); each call synchronises the stream.
 * sd_basis_rotate_dev: V[r, c] <- sum_{j < m} V[r, j] Q[j, c] for r < n_doubles, c < k, in place.  V: m columns of leading dimension
 *   ld_doubles >= n_doubles; Q: real, m x k, column-major, host.  Per element the sum runs in ascending j from a zero accumulator,
 *   one multiply then one add per term (no fused multiply-add).  Columns k..m-1 and the ld - n padding keep their bits.  A
 *   ComplexF64 basis is rotated as 2 n doubles (Ritz coefficients of a Hermitian problem in a Lanczos basis are real).
 *   SD_EARG unless 1 <= k <= m <= SD_EIGS_MAX_BASIS and k <= SD_EIGS_MAX_KEEP.
 * sd_block_dots_dev: out[2c], out[2c + 1] = re, im of <V[:, c] | w> (column conjugated; im = 0 for SD_F64), c < ncols <= 8, n
 *   elements, ld in elements, in one pass over w; summed in a fixed order.
 * sd_block_axpy_dev: w <- w - sum_c coef[c] V[:, c], coef[c] = (coef_host[2c], coef_host[2c + 1]) (the imaginary part is ignored
 *   for SD_F64), ascending c, one multiply and one subtraction per real term: x - cr v for real vectors,
 *   re = (re - cr v.re) + ci v.im, im = (im - cr v.im) - ci v.re for complex ones. */
int sd_basis_rotate_dev(sd_ctx *ctx, void *V_dev, int64_t ld_doubles, int64_t n_doubles, int m, const double *Q_host, int k);
int sd_block_dots_dev(sd_ctx *ctx, int dtype, const void *V_dev, int64_t ld, int ncols, const void *w_dev, int64_t n,
                      double *out_host /* 2 per column */);
int sd_block_axpy_dev(sd_ctx *ctx, int dtype, void *w_dev, const void *V_dev, int64_t ld, int ncols, const double *coef_host,
                      int64_t n);
/* lanczos_tridiag   src/Lanczos.jl:196-246.  alpha_out[min(lanc_m,n)], beta_out[min(lanc_m,n)-1] */
int sd_lanczos_tridiag(sd_ctx *ctx, const sd_model *m, const void *v_c128_host, int64_t n, int lanc_m,
                       double tol, double *alpha_out, double *beta_out, int *m_eff, double *norm_v);
/* krylov_time_evolve   src/TimeEvolution/Krylov.jl:136-192.  psit_out is ComplexF64. */
int sd_krylov_evolve(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi0_host, int64_t n,
                     double dt, int kry_m, void *psit_out_c128_host);
/* the same on device vectors (psi0 of `dtype`, psit ComplexF64; psit may be a ComplexF64 psi0).  Returns after the stream
 * has finished. */
int sd_krylov_evolve_dev(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi0_dev, int64_t n,
                         double dt, int kry_m, void *psit_out_c128_dev);
/* ---- driven dynamics: H(t) = H0 + sum_k f_k(t) D_k with diagonal drives (not in the reference) ----
 * H0 is the model as built.  A drive is D = sum_i site_w[i-1] S^z_i + sum_b zz_w[b] S^z_{zz_i[b]} S^z_{zz_j[b]}: site weights (L entries
 * or NULL) plus a zz-bond list of its own (sites 1-based, as sd_model_create; a bond may repeat).  For coefficients c_k the library
 * forms W_i = sum_k c_k site_w_k[i] (from 0.0, ascending k, one multiply then one add per term) and the concatenated bond list
 * (drive order, then list order, weights c_k zz_w_k[b], not merged), and one elementwise kernel adds d(s) psi to H0 psi, where d(s) is
 * the sequential sum, from 0.0, of the site terms +-W_i/2 in site order (skipped when no drive has site weights) and then the bond
 * terms +-V_b/4 in list order (+ for parallel spins), each selected, not multiplied; then one multiply d * psi and one add per
 * component.  Limits, answered with SD_EARG and a message: K <= SD_DRIVE_MAX, at most SD_DRIVE_MAX_BONDS bond terms in all, sites
 * in 1..L, i != j, finite weights and coefficients, an unsharded model.
 * sd_drive_check: the limits alone (host only).
 * sd_diag_apply: out = (sum_k c_k D_k) psi, or that + y when y != NULL (y of psi's dtype; may be out).  out must not alias psi.
 * sd_driven_apply: out = (H0 + sum_k c_k D_k) psi with the built-in H0 (operator level, as sd_apply: a caller's operator may call it,
 *   which makes it an operator for every recursion that takes one).  out must not alias psi.
 * sd_driven_evolve: for stage s = 0 .. n_stages-1, psi <- exp(-i tau[s] (H0 + sum_k coef[s K + k] D_k)) psi by the Krylov propagator
 *   (krylov_time_evolve's arithmetic, normalised by every stage) with the state on the device between stages.  A stage whose
 *   coefficients are all exactly zero (or K == 0) runs the built-in path of sd_krylov_evolve.  A caller's operator installed on the
 *   context (sd_ctx_set_apply_callback) replaces H0 as in every recursion.  psi0 of `dtype`, psit ComplexF64
 *   (psit may be a ComplexF64 psi0).  info (or NULL): stages run, operator applications, the smallest Lanczos beta seen.
 * _dev: the vectors are device pointers; the calls return after the stream has finished. */
#define SD_DRIVE_MAX 16
#define SD_DRIVE_MAX_BONDS 128
typedef struct sd_drive {
  const double *site_w;     /* L entries or NULL */
  int n_zz;
  const int *zz_i;          /* n_zz entries each (NULL allowed when n_zz == 0) */
  const int *zz_j;
  const double *zz_w;
} sd_drive;
typedef struct sd_driven_info {
  int stages;               /* stages run */
  int64_t applies;          /* operator applications of the call */
  double min_beta;          /* smallest Lanczos beta of all stages (+inf when no stage produced one) */
} sd_driven_info;
int sd_drive_check(const sd_model *m, const sd_drive *drives, int K);
int sd_diag_apply(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi_host, int64_t n, const sd_drive *drives, int K,
                  const double *coef, const void *y_host /* or NULL */, void *out_host);
int sd_diag_apply_dev(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi_dev, int64_t n, const sd_drive *drives, int K,
                      const double *coef, const void *y_dev /* or NULL */, void *out_dev);
int sd_driven_apply(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi_host, int64_t n, const sd_drive *drives, int K,
                    const double *coef, void *out_host);
int sd_driven_apply_dev(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi_dev, int64_t n, const sd_drive *drives, int K,
                        const double *coef, void *out_dev);
int sd_driven_evolve(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi0_host, int64_t n, const sd_drive *drives, int K,
                     int n_stages, const double *tau, const double *coef, int kry_m, void *psit_out_c128_host,
                     sd_driven_info *info /* or NULL */);
int sd_driven_evolve_dev(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi0_dev, int64_t n, const sd_drive *drives, int K,
                         int n_stages, const double *tau, const double *coef, int kry_m, void *psit_out_c128_dev,
                         sd_driven_info *info /* or NULL */);
/* ---- hopping drives: H(t) = H0 + sum_k c_k(t) O_k with every O_k a diagonal drive or a hopping drive (not in the reference;
 * DESIGN.md 25) ----
 * A hopping drive is B = sum_b (z_b S^+_{i[b]} S^-_{j[b]} + conj(z_b) S^-_{i[b]} S^+_{j[b]}), z_b = re[b] + i im[b] (im NULL: real
 * weights): Hermitian, so the coefficients stay real.  Sites 1-based, i != j, either orientation, a bond may repeat.  For coefficients
 * c_k the library forms the concatenated list (drive order, then list order, not merged) with weights x_b = c_k re[b], y_b = c_k im[b],
 * one multiply each, and drops the bonds of a drive whose coefficient is exactly 0.0.  A call is in REAL FORM iff every im of every
 * hopping drive passed is NULL or exactly zero -- a property of the drives, not of the coefficients.  One gather kernel then forms,
 * per row with configuration s, acc = (H0 psi)[r] (or y[r], or 0); acc += d(s) psi[r] when the call has a diagonal part (the
 * arithmetic of the diagonal drives above); and for each bond in list order whose two sites differ in s, with v = psi[partner row]:
 * real form acc.c += x_b v.c per component; complex form y' = +y_b when site i[b] is up in s and -y_b when site j[b] is (selected),
 * t = (x_b v.re - y' v.im, x_b v.im + y' v.re), acc += t.  Limits, answered with SD_EARG and a message: K + KH <= SD_DRIVE_MAX, at most
 * SD_HOP_MAX_BONDS terms in all hopping drives together, sites in 1..L, i != j, finite weights and coefficients, an unsharded model, out
 * or y sharing memory with psi, and -- in the two apply entries -- an SD_F64 vector with a complex-form list.  SD_EDIM: a wrong length.
 * sd_hop_drive_check: the limits alone (host only).
 * sd_hop_apply: out = (sum_k c_k B_k) psi, or that + y when y != NULL (y of psi's dtype; may be out).  out must not alias psi.
 * sd_driven_hop_apply: out = (H0 + sum_k coef[k] D_k + sum_k coef[K + k] B_k) psi with the built-in H0 (operator level, as
 *   sd_driven_apply).  out must not alias psi.
 * sd_driven_hop_evolve: sd_driven_evolve with both kinds of drive: coef[n_stages x (K + KH)], stage s at coef + s (K + KH), the K
 *   diagonal columns first.  A stage whose hopping coefficients are all exactly zero runs exactly the calls of sd_driven_evolve.  In
 *   complex form an SD_F64 psi0 is promoted to ComplexF64 once, before the first stage; in real form an SD_F64 first stage stays real.
 * _dev: the vectors are device pointers; the calls return after the stream has finished. */
#define SD_HOP_MAX_BONDS 128
typedef struct sd_hop_drive {
  int n;
  const int *i;             /* n entries each (NULL allowed when n == 0) */
  const int *j;
  const double *re;
  const double *im;         /* n entries or NULL */
} sd_hop_drive;
int sd_hop_drive_check(const sd_model *m, const sd_hop_drive *hops, int KH);
int sd_hop_apply(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi_host, int64_t n, const sd_hop_drive *hops, int KH,
                 const double *coef, const void *y_host /* or NULL */, void *out_host);
int sd_hop_apply_dev(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi_dev, int64_t n, const sd_hop_drive *hops, int KH,
                     const double *coef, const void *y_dev /* or NULL */, void *out_dev);
int sd_driven_hop_apply(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi_host, int64_t n, const sd_drive *drives, int K,
                        const sd_hop_drive *hops, int KH, const double *coef, void *out_host);
int sd_driven_hop_apply_dev(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi_dev, int64_t n, const sd_drive *drives, int K,
                            const sd_hop_drive *hops, int KH, const double *coef, void *out_dev);
int sd_driven_hop_evolve(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi0_host, int64_t n, const sd_drive *drives, int K,
                         const sd_hop_drive *hops, int KH, int n_stages, const double *tau, const double *coef, int kry_m,
                         void *psit_out_c128_host, sd_driven_info *info /* or NULL */);
int sd_driven_hop_evolve_dev(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi0_dev, int64_t n, const sd_drive *drives, int K,
                             const sd_hop_drive *hops, int KH, int n_stages, const double *tau, const double *coef, int kry_m,
                             void *psit_out_c128_dev, sd_driven_info *info /* or NULL */);
/* chebyshev_time_evolve   src/TimeEvolution/Chebyshev.jl:61-124  (psi0 ComplexF64) */
int sd_chebyshev_evolve(sd_ctx *ctx, const sd_model *m, const void *psi0_c128_host, int64_t n, double dt,
                        int cheb_n, double Emin, double Emax, void *psit_out_c128_host);
/* the same on device vectors (ComplexF64, n elements): psi stays on the GPU between the steps of a time evolution.
 * psit_dev may be psi0_dev (in place).  Returns after the stream has finished. */
int sd_chebyshev_evolve_dev(sd_ctx *ctx, const sd_model *m, const void *psi0_c128_dev, int64_t n, double dt,
                            int cheb_n, double Emin, double Emax, void *psit_out_c128_dev);
/* compute_chebyshev_moments   src/KPM_Sqw.jl:95-128 */
int sd_kpm_moments(sd_ctx *ctx, const sd_model *m, const void *phi_c128_host, int64_t n, int M,
                   double a, double b, double *mu_out);
/* get_kernel   src/KPM_Sqw.jl:131-145 (host) */
int sd_kpm_kernel(int M, int kernel, double *g_out);
/* _rescaling_from_bounds   src/KPM_Sqw.jl:13-17 (host) */
int sd_kpm_rescaling_from_bounds(double Emin, double Emax, double *a, double *b);
/* reconstruction part of kpm_sw   src/KPM_Sqw.jl:55-90 (host), moments already damped */
int sd_kpm_reconstruct(const double *mu_damped, int kpm_m, const double *omega, int W, double a, double b,
                       double E0, double *S_out);
/* kpm_sqw   src/KPM_Sqw.jl:191-256.  Smat_out is Qn x W row-major.  When
 * have_ab == 0 the rescaling is estimated as the reference does (two Lanczos
 * runs, lanc_m = 80) with generated start vectors keyed by `seed`. */
int sd_kpm_sqw(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi0_host, int64_t n,
               const double *q, int Qn, const double *omega, int W, int have_ab, double a, double b,
               int kpm_m, int kernel, uint64_t seed, double *Smat_out);
/* spectral_from_tridiagonal   src/LanczosSqw.jl:18-43 (host) */
int sd_spectral_from_tridiagonal(const double *alpha, const double *beta, int m, double norm_phi, double E0,
                                 const double *omega, int W, double eta, int broaden, double *S_out);
/* lanczos_sqw   src/LanczosSqw.jl:49-80 */
int sd_lanczos_sqw(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi0_host, int64_t n,
                   const double *q, int Qn, const double *omega, int W, int lanc_m, double eta, int broaden,
                   double *Smat_out);
/* Transverse S(q,w) between adjacent sectors.  src holds psi0 (sector nup); dst is the sector the operator maps it to:
 * op SD_SPIN_MINUS, S^-_q = L^(-1/2) sum_r e^{iqr} S^-_{r+1}, needs dst.nup == src.nup - 1 (S^{+-}); op SD_SPIN_PLUS, S^+_q,
 * needs dst.nup == src.nup + 1 (S^{-+}).  Two full-basis models of the same L pair up too (dst may be src).  The caller owns
 * both models; they must have the same L and bit-identical hop, zz and field lists, neither may be sharded, and the context
 * may not hold a caller's operator (it belongs to one sector): any mismatch is SD_EARG, sd_last_error names it.
 * sd_spm_q: phi_out (n_dst = dst's dimension, always ComplexF64) = S^-+_q psi0 (n_src = src's dimension, dtype_in).  The
 * rounding is fixed: per target row the terms r = 0..L-1 in ascending order, acc += (c_r x.re - s_r x.im, c_r x.im + s_r x.re)
 * without fused multiply-adds, out = acc / sqrt(L) as (nf acc.re, nf acc.im).  Wrong lengths are SD_EDIM.
 * sd_spm_q_dev: the same on device vectors, ordered on the context's stream. */
int sd_spm_q(sd_ctx *ctx, const sd_model *src, const sd_model *dst, int op, int dtype_in, const void *psi0_host,
             int64_t n_src, double q, void *phi_out_host, int64_t n_dst);
int sd_spm_q_dev(sd_ctx *ctx, const sd_model *src, const sd_model *dst, int op, int dtype_in, const void *psi0_dev,
                 int64_t n_src, double q, void *phi_out_dev, int64_t n_dst);
/* kpm_sqw / lanczos_sqw with phi = S^-+_q psi0 in place of S^z_q psi0 (S^{+-} for SD_SPIN_MINUS, S^{-+} for SD_SPIN_PLUS).
 * psi0 has n = src's dimension; E0 comes from src (kpm: <psi0|H psi0>; lanczos: Re sum psi_i (H psi)_i, as sd_lanczos_sqw);
 * the recursion -- bounds (have_ab == 0: two 80-step Lanczos runs keyed by `seed`), moments, tridiagonal -- runs on dst's H.
 * Normalisation, zero-norm rows, kernels and the |phi|^2 scaling are those of sd_kpm_sqw / sd_lanczos_sqw.  Errors as
 * sd_spm_q. */
int sd_kpm_sqw_transverse(sd_ctx *ctx, const sd_model *src, const sd_model *dst, int op, int dtype, const void *psi0_host,
                          int64_t n, const double *q, int Qn, const double *omega, int W, int have_ab, double a, double b,
                          int kpm_m, int kernel, uint64_t seed, double *Smat_out);
int sd_lanczos_sqw_transverse(sd_ctx *ctx, const sd_model *src, const sd_model *dst, int op, int dtype, const void *psi0_host,
                              int64_t n, const double *q, int Qn, const double *omega, int W, int lanc_m, double eta,
                              int broaden, double *Smat_out);

/* ---- site-resolved KPM correlations (the quantity of the reference's src/TimeEvolution/KPM.jl, kpm_correlation_matrix) ----
 *   mu_n^{ij} = <psi0| S^z_i T_n(H~) S^z_j |psi0>,   C_ij(w) = <psi0| S^z_i delta(w - (H - E0)) S^z_j |psi0>,
 * sites 1-based, r_i = i - 1 as in Sz_q_vector, psi0 properly conjugated (mu is complex; real for a real psi0).  One recursion
 * from S^z_j psi0 gives the moments against ALL L sites i: each Chebyshev step projects v_n = T_n(H~) S^z_j psi0 onto the L
 * vectors S^z_i psi0 in one pass.  Rescaling a, b (0.99 pad; estimated from `seed` when have_ab == 0), kernel g_n,
 * E0 = Re<psi0|H psi0> and x = (w + E0 - b)/a are those of sd_kpm_sqw.  Unsharded models only (SD_EARG otherwise); a caller's
 * operator (sd_ctx_set_apply_callback) is honoured.
 *
 * sd_site_project: out[2(i-1) .. +1] = (re, im) of sum_rows conj(bra[row]) s_i(row) ket[row], s_i = +-1/2, i = 1..L -- bra of
 * `dtype_bra` (n elements, not promoted), ket ComplexF64 (n elements), out 2L host doubles.  One pass over both vectors, sums
 * in a fixed order: the same call gives the same bits.  _dev: bra, ket device pointers; the call synchronises the stream. */
int sd_site_project(sd_ctx *ctx, const sd_model *m, int dtype_bra, const void *bra_host, const void *ket_c128_host, int64_t n,
                    double *out);
int sd_site_project_dev(sd_ctx *ctx, const sd_model *m, int dtype_bra, const void *bra_dev, const void *ket_c128_dev, int64_t n,
                        double *out);
/* mu_out[((s * M + n) * L + (i-1)) * 2 .. +1] = (re, im) of mu_n^{i j_s}, j_s = sources[s] (1-based, ns of them), n = 0..M-1:
 * v_0 = S^z_j psi0, v_1 = H~ v_0, v_n = 2 H~ v_{n-1} - v_{n-2}, a projection after each; M - 1 applies per source, queued without
 * a host round trip and read back once.  Sources share their launches under the conditions of sd_ctx_set_q_batch (bit-identical
 * to one source at a time).  SD_EARG: a source outside 1..L, M < 2, a sharded model, or sum |v_n|^2 not finite or above
 * 1e6 sum |v_0|^2 (a, b do not contain the spectrum; sd_last_error names them).  _dev: psi0 is a device pointer. */
int sd_kpm_site_moments(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi0_host, int64_t n, const int *sources, int ns,
                        int M, double a, double b, double *mu_out);
int sd_kpm_site_moments_dev(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi0_dev, int64_t n, const int *sources, int ns,
                            int M, double a, double b, double *mu_out);
/* sd_kpm_reconstruct without the clamp at zero (off-diagonal C_ij is signed):
 * out[w] = (mu_0 + 2 sum_{n>=1} mu_n T_n(x)) / (a pi sqrt(1 - x^2)), 0 for |x| >= 1; moments already damped (host) */
int sd_kpm_reconstruct_signed(const double *mu_damped, int kpm_m, const double *omega, int W, double a, double b, double E0,
                              double *out);
/* C_out[(((i-1) * ns + s) * W + w) * 2 .. +1] = (re, im) of C_{i j_s}(omega[w]): the damped moments reconstructed unclamped,
 * Re and Im separately. */
int sd_kpm_site_correlations(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi0_host, int64_t n, const int *sources,
                             int ns, const double *omega, int W, int have_ab, double a, double b, int kpm_m, int kernel,
                             uint64_t seed, double *C_out);
/* S^zz(q, w) at every q of the list from the site moments: the rows sd_kpm_sqw returns, Smat_out Qn x W row-major.
 * translation_invariant == 0: ns must be L and sources name every site once;
 *   mu_n(q) = Re (1/L) sum_ij e^{-iq(r_i - r_j)} mu_n^{ij} -- any psi0, any boundary, L recursions for any number of momenta.
 * translation_invariant != 0: ns must be 1; mu_n(q) = Re sum_i e^{-iq(r_i - r_j)} mu_n^{ij} from the one source j -- exact when
 *   psi0 and H are invariant under the cyclic shift (the ground state of a periodic chain): M - 1 applies for ALL momenta.
 *   *defect_out = max_{n,q} |Im sum_i ...| / (|psi0|^2 / 4), which vanishes for an invariant state (1e-14) and is O(0.1) for
 *   a state that is not: the caller decides (the Python mirror raises above ti_tol).  defect_out may be NULL; it is 0 when
 *   translation_invariant == 0. */
int sd_kpm_sqw_sites(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi0_host, int64_t n, const double *q, int Qn,
                     const double *omega, int W, const int *sources, int ns, int translation_invariant, int have_ab, double a,
                     double b, int kpm_m, int kernel, uint64_t seed, double *Smat_out, double *defect_out);

/* ---- finite temperature by dynamical quantum typicality, with the spin current ----------------------------------------
 * The quantity of the reference's src/TimeEvolution/QuantumTypicality.jl (typicality_correlation_function, :33-91), a module
 * the reference never includes and that calls undefined names; built here on this library's own definitions:
 *   psi_beta = exp(-beta H / 2) r for a start vector r;  num_r(t) = <psi_beta(t)| A |phi(t)>,  psi_beta(t) = exp(-iHt) psi_beta,
 *   phi(t) = exp(-iHt) B psi_beta;  den_r = |psi_beta|^2;  <A(t) B>_beta ~ sum_r num_r(t) / sum_r den_r.
 * Unlike the reference (:86-87, which leaves the bra at t = 0) the bra is evolved as well; the model is an argument (the
 * reference hard-wires nup = L/2); operators are descriptors so that the loop stays on the device; no :rk4 method.
 *
 * Spin current.  With hops (i_b, j_b, t_b) the bond current is j_b = i t_b (S^+_{i_b} S^-_{j_b} - S^-_{i_b} S^+_{j_b}): Hermitian,
 * carrying S^z from site i_b to site j_b, i[H, S^z_k] = sum_{b: j_b = k} j_b - sum_{b: i_b = k} j_b.  J_w = sum_b w_b j_b with real
 * weights w (n_hop doubles; NULL: ones, the total current).  Row form, as computed:
 *   (J_w psi)[s] = i * sum_{b: s_{i_b} != s_{j_b}} (w_b t_b sigma_b(s)) * psi[flip_b(s)],  sigma_b = +1 when site i_b is up in s,
 * in hop-list order from a zero accumulator, no fused multiply-add, the factor i as the exact swap (re, im) -> (-im, re).
 * Unsharded models only (SD_EARG otherwise). */
#define SD_EVOLVE_CHEBYSHEV 0
#define SD_EVOLVE_KRYLOV 1
/* c_out[k] = (2 - delta_k0) (-1)^k exp(-z) I_k(z), z = a * tau, k = 0 .. *n_used - 1: exp(-z x) exp(-z) = sum_k c_k T_k(x) on
 * [-1, 1].  *n_used is the first k with k > z and exp(-z) I_k(z) < 2^-53 exp(-z) I_0(z).  Scaled Bessel functions, nothing
 * overflows.  SD_EARG when z < 0, z > 600 or *n_used > n_max (host only). */
int sd_chebyshev_imag_coeffs(int n_max, double a, double tau, double *c_out, int *n_used);
/* out = exp(-tau H) psi0 / |.| (ComplexF64, n elements), *log_norm = ln |exp(-tau H) psi0|; psi0 of `dtype`, tau >= 0.
 * method SD_EVOLVE_CHEBYSHEV: exp(-tau H) = exp(-tau (b - a)) sum_k c_k T_k((H - b)/a) with the coefficients above and
 *   a = (Emax - Emin)/(2 * 0.9999), b = (Emax + Emin)/2 through the term loop of sd_chebyshev_evolve; cheb_n = 0 takes *n_used
 *   terms, cheb_n > 0 at most cheb_n; z = a * tau > 600 is split into equal sub-steps, the vector renormalised after each and the
 *   logarithms added up.  Emax <= Emin: the bounds are estimated as sd_energy_bounds does, seed 0.
 * method SD_EVOLVE_KRYLOV: krylov_imaginary_time_evolution (src/TimeEvolution/QuantumTypicality.jl:154-211) on the Lanczos vectors
 *   of sd_krylov_evolve: exp(-tau theta) in place of the phase, ONE projection on kry_m vectors, no sub-stepping -- accurate
 *   only while tau * (bandwidth) is small against kry_m.
 * _dev: psi0_dev, out_dev device pointers (out_dev may be psi0_dev for a ComplexF64 psi0); the call synchronises the stream. */
int sd_imag_evolve(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi0_host, int64_t n, double tau, int method,
                   int cheb_n, int kry_m, double Emin, double Emax, void *out_c128_host, double *log_norm);
int sd_imag_evolve_dev(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi0_dev, int64_t n, double tau, int method,
                       int cheb_n, int kry_m, double Emin, double Emax, void *out_c128_dev, double *log_norm);
/* out (ComplexF64, n elements) = J_w psi, psi of `dtype`.  _dev: device pointers, out_dev must not alias psi_dev. */
int sd_current_apply(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi_host, int64_t n, const double *w,
                     void *out_c128_host);
int sd_current_apply_dev(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi_dev, int64_t n, const double *w,
                         void *out_c128_dev);
/* out[0..1] (host) = (re, im) of <bra| J_w |ket> WITHOUT writing J_w ket: one pass over bra (`dtype_bra`, not promoted) and ket
 * (ComplexF64) plus the gathers, per-block sums reduced in a fixed order -- no atomics, the same call gives the same bits. */
int sd_current_bracket(sd_ctx *ctx, const sd_model *m, int dtype_bra, const void *bra_host, const void *ket_c128_host, int64_t n,
                       const double *w, double *out);
int sd_current_bracket_dev(sd_ctx *ctx, const sd_model *m, int dtype_bra, const void *bra_dev, const void *ket_c128_dev, int64_t n,
                           const double *w, double *out);
/* operator kinds of sd_dqt_correlations; `param` is the site (1-based) or the momentum q, `w` the weights of a current */
#define SD_DQT_SZ_SITE 0   /* S^z_site */
#define SD_DQT_SZ_Q 1      /* S^z_q of sd_szq; as the measured operator A its adjoint: <S^z_q psi| phi> */
#define SD_DQT_SZ_ALL 2    /* A only: S^z_i for every site i = 1..L at once (nA = L) */
#define SD_DQT_CURRENT 3   /* J_w of the model's hop list (also with a caller's operator) */
#define SD_DQT_ENERGY_CURRENT 4   /* J_E of the model's lists (sd_energy_current_terms, below), as A and as B; `param` is the geometry,
                                     0 a line, 1 a ring; `w` must be NULL (SD_EARG).  The list is built once per call. */
/* One sample of <A(t) B>_beta.  r_host: the start vector (ComplexF64, n = sd_model_dim elements) or NULL for the counter-based
 * normal stream of `seed` (sd_fill_randn_host(x, 2n, seed, 0) gives the same vector on the host); it is normalised first.
 * beta >= 0 (0 skips the imaginary-time step); times[nt] non-decreasing, times[0] >= 0.  method / cheb_n / kry_m / Emin / Emax as
 * sd_imag_evolve (bounds estimated from `seed` when Emax <= Emin); real-time Chebyshev steps take the first k with k > a dt and
 * |J_k(a dt)| < 2^-53 terms when cheb_n == 0, and equal steps share their coefficients.  The two states share their launches
 * under the conditions of sd_ctx_set_q_batch (bit-identical to separate launches).  A caller's operator is honoured for the
 * evolution.  Outputs (host): num_out[(k * nA + i) * 2 .. +1] = (re, im) of <psi(t_k)| A_i |phi(t_k)> for the NORMALISED
 * psi_beta -- num_r(t_k) = *den_out * num_out --, *den_out = exp(2 * *log_norm) = |psi_beta|^2 (may overflow; *log_norm does not),
 * *energy_out = <psi_beta|H|psi_beta> / <psi_beta|psi_beta>.  All measurements are filed on the device and read back once. */
int sd_dqt_correlations(sd_ctx *ctx, const sd_model *m, double beta, const void *r_host, uint64_t seed, int B_kind,
                        double B_param, const double *w_B, int A_kind, double A_param, const double *w_A, const double *times,
                        int nt, int method, int cheb_n, int kry_m, double Emin, double Emax, double *num_out, double *den_out,
                        double *energy_out, double *log_norm);

/* ---- energy current: lists of dressed bond currents -------------------------------------------------------------------
 * With the unit bond current j'_ij = i (S^+_i S^-_j - S^-_i S^+_j) a TERM (i, j, k, c) stands for c S^z_k j'_ij; i != j and k not in
 * {i, j}, or k = 0: no S^z factor.  Sites are 1-based.  A list J = sum of its terms is Hermitian and conserves S^z (fixed-nup sectors
 * and the full basis alike).  Consecutive terms with the same ordered (i, j) form a GROUP.  Row form, as computed (no fused
 * multiply-add):
 *   (J psi)[s] = i * sum_groups [s_i != s_j] (sigma co) psi[s with sites i, j exchanged],  sigma = +1 when site i is up in s,
 *   co = sum over the group's terms, in list order from 0.0, of (k == 0 ? c : (site k up in s ? 0.5 c : -0.5 c)),
 * real and imaginary parts summed separately in group order from zero, the factor i as the exact swap (re, im) -> (-im, re); one
 * gather per group.
 *
 * sd_energy_current_terms: the energy current of the model's lists as such a list (host only; works on a model created without
 *   a context).  H = sum_a h_a with hops t (S^+_i S^-_j + h.c.), zz terms v S^z_i S^z_j and field terms B_i S^z_i; a bond (i, j) sits
 *   at x = i + delta/2, delta = j - i, a field term at x = i; with periodic = 1, delta and every position difference are minimum
 *   images on a ring of L sites.  J_E = (i/2) sum_{a,b} (x_b - x_a) [h_a, h_b]; on a line this is i [H, sum_a x_a h_a].  Terms of
 *   equal (i, j, k) are merged after orienting each to i < j (swapping i and j flips the sign of c), exact zeros dropped, the list
 *   sorted by (i, j, k): that order is part of the interface.  cap = 0: only *n_terms is set.  SD_EARG: a position difference of
 *   exactly +-L/2 with periodic = 1, more than SD_DTERM_MAX terms, 0 < cap < *n_terms, periodic not 0 or 1.
 * sd_dcurrent_apply: out (ComplexF64, n elements) = J psi for an explicit list (a subset of the above: a local energy current; or a
 *   caller's own), psi of `dtype`.  _dev: device pointers, out_dev must not alias psi_dev.
 * sd_dcurrent_bracket: out[0..1] (host) = (re, im) of <bra| J |ket> without writing J ket; bra of `dtype_bra`, ket ComplexF64; sums
 *   in a fixed order, the same call gives the same bits.
 * SD_EARG: i == j, k in {i, j}, a site outside 1..L (k may also be 0), a coefficient that is not finite, n_terms outside
 * 0..SD_DTERM_MAX, out aliasing psi, a sharded model, a model without device tables, another dtype.  SD_EDIM: n is not the basis
 * dimension.  An empty list or a model with no rows gives a zero vector / a zero bracket. */
#define SD_DTERM_MAX 4096
typedef struct sd_dterm { int32_t i, j, k; double c; } sd_dterm;
int sd_energy_current_terms(const sd_model *m, int periodic, sd_dterm *out, int cap, int *n_terms);
int sd_dcurrent_apply(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi_host, int64_t n, const sd_dterm *terms, int n_terms,
                      void *out_c128_host);
int sd_dcurrent_apply_dev(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi_dev, int64_t n, const sd_dterm *terms, int n_terms,
                          void *out_c128_dev);
int sd_dcurrent_bracket(sd_ctx *ctx, const sd_model *m, int dtype_bra, const void *bra_host, const void *ket_c128_host, int64_t n,
                        const sd_dterm *terms, int n_terms, double *out);
int sd_dcurrent_bracket_dev(sd_ctx *ctx, const sd_model *m, int dtype_bra, const void *bra_dev, const void *ket_c128_dev, int64_t n,
                            const sd_dterm *terms, int n_terms, double *out);

/* ---- observables and initial states (reference src/Observables.jl, src/InitialStates.jl) ---- */
/* magnetization_per_site   src/Observables.jl:14-36 : mags_out[L] = <S^z_i> */
int sd_magnetization(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi_host, int64_t n, double *mags_out);
int sd_magnetization_dev(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi_dev, int64_t n, double *mags_out);
/* connected_correlations   src/Observables.jl:44-94 : C_out[L], C_r = (1/L) sum_i (<S_i S_j> - <S_i><S_j>), j = mod1(i+r,L) */
int sd_connected_correlations(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi_host, int64_t n, double *C_out);
int sd_connected_correlations_dev(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi_dev, int64_t n, double *C_out);
/* structure_factor_Sq   src/Observables.jl:100-109 : q_out[k] = 2 pi k / L, S_out[k] = real(fft(C_r))[k] */
int sd_structure_factor(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi_host, int64_t n, double *q_out, double *S_out);
int sd_structure_factor_dev(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi_dev, int64_t n, double *q_out, double *S_out);
/* Equal-time pair correlations of one state, all L x L site pairs from one call (sites 1-based; nothing is divided by <psi|psi>,
 * as in the observables above):
 *   SD_PAIR_PM: G_ij = <psi| S^+_i S^-_j |psi> = sum over rows s with site j up and site i down of conj(psi[s']) psi[s], s' = s with
 *               the up spin moved from j to i.  Hermitian; G_ii = sum_s |psi[s]|^2 [site i up] = <psi|psi>/2 + <S^z_i>; complex for
 *               a ComplexF64 psi, imaginary parts exactly 0 for a Float64 psi.  <S^-_i S^+_j> = conj(G_ij) for i != j and
 *               <psi|psi>/2 - <S^z_i> for i == j, in a sector and in the full basis alike.
 *   SD_PAIR_ZZ: Z_ij = <psi| S^z_i S^z_j |psi>; real symmetric, Z_ii = <psi|psi>/4, imaginary parts 0.
 * M_out: 2 L L host doubles, (re, im) of M[i-1][j-1] row-major, both triangles and the diagonal.  Fixed-nup sectors and the full
 * basis; unsharded models only (SD_EARG), a wrong n is SD_EDIM.  Sums in a fixed order: the same call gives the same bits.
 * _dev: psi is a device pointer; the call synchronises the stream. */
#define SD_PAIR_ZZ 0
#define SD_PAIR_PM 1
int sd_pair_correlations(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi_host, int64_t n, int component, double *M_out);
int sd_pair_correlations_dev(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi_dev, int64_t n, int component, double *M_out);
/* Bond operators and dimer correlations of one state (sites 1-based; nothing is divided by <psi|psi>).  For a bond b = (i, j), i != j,
 * and two real weights
 *   D_b = xy/2 (S^+_i S^-_j + S^-_i S^+_j) + zz S^z_i S^z_j          (xy = zz = 1: S_i . S_j; symmetric in i, j):
 *   (D_b psi)(s) = +-(zz/4) psi(s), + when the two sites agree in s, plus (xy/2) psi(s') when they differ, s' = s with the two sites
 *   exchanged.  D_b conserves S^z: fixed-nup sectors and the full basis alike.
 * sd_bond_apply: out (n elements of psi's dtype) = D_b psi, every row written.  _dev: device pointers, out_dev must not alias
 *   psi_dev (SD_EARG).
 * sd_dimer_correlations: for the B bonds (i_0, j_0, i_1, j_1, ...) of `bonds` (2 B host ints; a bond may appear twice or reversed),
 *   D_out: 2 B B host doubles, (re, im) of D[a][b] = <psi| D_a D_b |psi> = sum_s conj((D_a psi)(s)) (D_b psi)(s) row-major, both
 *          triangles and the diagonal.  Hermitian to the bit (one triangle is summed), the diagonal's imaginary parts exactly 0;
 *          complex for a ComplexF64 psi when bonds overlap (D_a and D_b do not commute then), imaginary parts exactly 0 for a Float64 psi.
 *   e_out: B host doubles, e[b] = <psi| D_b |psi>.
 *   One pass of a Gram-accumulating gather kernel: no vector D_b psi is stored.  Sums in a fixed order: the same call gives the
 *   same bits.  _dev: psi is a device pointer; the call synchronises the stream.
 * SD_EARG: i == j, a site outside 1..L, B < 1 or B > SD_DIMER_MAX_BONDS, a dtype other than SD_F64 / SD_C128, weights that are not
 * finite, a sharded model, a model without device tables.  SD_EDIM: n is not the basis dimension.  A model with no rows gives zeros. */
#define SD_DIMER_MAX_BONDS 128
int sd_bond_apply(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi_host, int64_t n, int i, int j, double xy, double zz,
                  void *out_host);
int sd_bond_apply_dev(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi_dev, int64_t n, int i, int j, double xy, double zz,
                      void *out_dev);
int sd_dimer_correlations(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi_host, int64_t n, const int *bonds, int B,
                          double xy, double zz, double *D_out, double *e_out);
int sd_dimer_correlations_dev(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi_dev, int64_t n, const int *bonds, int B,
                              double xy, double zz, double *D_out, double *e_out);
/* ---- lattice symmetry operators: translation, reflection, spin flip ---------------------------------------------------------
 * Site i is bit i - 1 of a configuration s; L-bit masks implied.
 *   T moves the spin of site i to site i + 1 (mod L):  T s = ((s << 1) | (s >> (L - 1))) & mask;
 *   R exchanges site i with site L + 1 - i: bit reversal over L bits;
 *   Z flips every spin: ~s & mask -- defined on the full basis and on sectors with 2 nup = L only (SD_EARG elsewhere).
 * A group element g = (r, refl, flip) is U_g = T^r R^refl Z^flip, U_g |s> = |T^r R^refl Z^flip s>, so
 *   (U_g psi)[idx(s)] = psi[idx(Z^flip R^refl T^-r s)];   its CODE is r | refl << 8 | flip << 9 with 0 <= r < L.
 * Nothing is divided by <psi|psi>.  Fixed-nup sectors and the full basis; unsharded models only.
 *
 * sd_model_symmetric: *yes = 1 when the hop, zz and field lists are invariant under U_g, else 0 (host only; works on a model created
 *   without a context).  Bond tables are summed per unordered site pair, i == j and exact zeros dropped, and compared exactly after
 *   the site permutation of T^r R^refl; the field must be invariant under that permutation, and all zero for flip = 1.
 * sd_symmetry_apply: out (n elements of psi's dtype, every row written) = U_g psi -- a permutation, every output is bit for bit one
 *   input -- or, with y != NULL, the fused out = U_g psi + (c_re + i c_im) y (y of psi's dtype, read row by row; a Float64 psi takes
 *   c_im = 0).  _dev: device pointers; out_dev must not share a byte with psi_dev (SD_EARG: identity and partial overlap alike); it
 *   may be y_dev itself, not a range that overlaps y_dev partly.
 * sd_symmetry_overlaps: out[2k .. +1] (host) = (re, im) of <bra|U_g|ket> = sum_s conj(bra[s]) (U_g ket)[s] for element k of `codes`
 *   (n_codes host ints, 1 .. SD_SYM_MAX_ELEMENTS), all in one pass over the rows; bra and ket of `dtype`, bra NULL: ket itself.  Sums
 *   in a fixed order: the same call gives the same bits.
 * sd_symmetry_project: out = sum_k c_k U_{g_k} psi, c_k = (coef[2k], coef[2k + 1]), in one pass; per row the terms are added in list
 *   order from zero, each product formed first, no fused multiply-add.  dtype_out is SD_C128, or SD_F64 for an SD_F64 psi when every
 *   coefficient is real (SD_EARG otherwise).  out_dev must not share a byte with psi_dev.
 * _dev: the vectors are device pointers; sd_symmetry_apply_dev is queued on the context's stream, the other two synchronise it.
 * SD_EARG: r outside 0..L-1 or other bits set in a code, Z in a sector with 2 nup != L, n_codes out of range, a NULL pointer, a dtype
 * other than SD_F64 / SD_C128, coefficients that are not finite, out aliasing psi, a sharded model, a model without device tables.
 * SD_EDIM: n is not the basis dimension.  A model with no rows gives empty vectors / zero overlaps. */
#define SD_SYM_REFLECT 256
#define SD_SYM_FLIP 512
#define SD_SYM_MAX_ELEMENTS 252
int sd_model_symmetric(const sd_model *m, int code, int *yes);
int sd_symmetry_apply(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi_host, int64_t n, int code, const void *y_host,
                      double c_re, double c_im, void *out_host);
int sd_symmetry_apply_dev(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi_dev, int64_t n, int code, const void *y_dev,
                          double c_re, double c_im, void *out_dev);
int sd_symmetry_overlaps(sd_ctx *ctx, const sd_model *m, int dtype, const void *bra_host, const void *ket_host, int64_t n,
                         const int *codes, int n_codes, double *out);
int sd_symmetry_overlaps_dev(sd_ctx *ctx, const sd_model *m, int dtype, const void *bra_dev, const void *ket_dev, int64_t n,
                             const int *codes, int n_codes, double *out);
int sd_symmetry_project(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi_host, int64_t n, const int *codes,
                        const double *coef, int n_codes, int dtype_out, void *out_host);
int sd_symmetry_project_dev(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi_dev, int64_t n, const int *codes,
                            const double *coef, int n_codes, int dtype_out, void *out_dev);
/* ---- operator strings: any product of S^+, S^-, S^z, and sums of such products ------------------------------------------------
 * Site i is bit i - 1 of a configuration s.  A TERM is (plus P, minus M, z Z, c, op): P, M, Z are 64-bit site masks, pairwise disjoint,
 * with no bit at or above L; c = (c_re, c_im) is a complex coefficient; op >= 0 is the index of the operator the term belongs to:
 *   O_k = sum_{t : op_t = k}  c_t  prod_{i in P_t} S^+_i  prod_{j in M_t} S^-_j  prod_{l in Z_t} S^z_l.
 * All factors of a term sit on distinct sites, so their order does not matter.  In a fixed-nup sector every term must have
 * |P| = |M| (SD_EARG otherwise); on the full basis any term is allowed (rows are configurations there).  A source sector different
 * from the destination sector (as in sd_spm_q) is not covered.  Consecutive terms with equal (P, M, op) form a GROUP and share one
 * gather.  Row form, as computed, nothing contracted:
 *   (O psi)[s] = sum_groups [(s & P) == P and (s & M) == 0] co_g(s) psi[row(s ^ (P | M))]
 *   co_g(s)    = sum over the group's terms, in list order from (0.0, 0.0), of sigma_t(s) ch_t,
 *                sigma_t(s) = +1 when popcount(~s & Z_t) is even, else -1;  ch_t = c_t 2^-|Z_t| (scaled on the host, exact)
 *   product:     t_re = co_re v_re - co_im v_im, t_im = co_re v_im + co_im v_re, both products first, then the add or subtract;
 *                a Float64 psi: t_re = co_re v, t_im = co_im v
 *   (re, im) accumulated from (0.0, 0.0) in group order.  A group with P = M = 0 is diagonal: its source is the row itself.
 * Nothing is divided by <psi|psi>.  Fixed-nup sectors and the full basis; unsharded models only.
 *
 * sd_opstring_check: host only (works on a model created without a context).  Validates the list against the model, sets
 *   *n_ops = K = 1 + the largest op (0 for an empty list) and *hermitian = 1 when, for every op, the list equals its own adjoint
 *   (the adjoint of a term swaps P and M and conjugates c; coefficients of equal (P, M, Z) are summed first and compared exactly).
 * sd_hamiltonian_terms: host only; the model's hop, zz and field lists as strings with op = 0, in list order: a hop (i, j, t) gives the
 *   two terms t S^+_i S^-_j then t S^-_i S^+_j (none when i == j), a zz term (i, j, v) gives v with Z = {i, j} (v/4 with Z empty when
 *   i == j), field entry i gives B_i with Z = {i}.  That order is part of the interface.  cap = 0: only *n_terms is set; SD_EARG for
 *   0 < cap < *n_terms or more than SD_OPTERM_MAX terms.
 * sd_opstring_apply: out (n elements of dtype_out, every row written) = O_0 psi, or with y != NULL the fused
 *   out = O_0 psi + (b_re + i b_im) y: t = b y formed as the complex product above (a Float64 output: b_re y), then one add per
 *   component; y has dtype_out.  Every term must have op = 0.  dtype_out is SD_C128, or SD_F64 for an SD_F64 psi when every c_im and
 *   b_im is exactly 0.  _dev: device pointers, queued on the context's stream (a call with a non-empty list returns after the stream has
 *   drained: its tables go back to the context's pool); out_dev must not share a byte with psi_dev (identity and partial overlap
 *   alike); it may be y_dev itself, not a range that overlaps y_dev partly.
 * sd_opstring_expect: out[2k .. +1] (host, 2 K doubles) = (re, im) of sum_s conj(bra[s]) (O_k ket)[s] for k = 0 .. K-1, all in one pass
 *   over the rows, no vector O_k ket stored; bra and ket of `dtype`, bra NULL: ket itself.  Sums in a fixed order: the same call gives
 *   the same bits.  Both forms synchronise the stream.
 * SD_EARG: overlapping masks, a bit at or above L, |P| != |M| in a sector, a coefficient that is not finite, op < 0 or op >=
 * SD_OPSTRING_MAX_OPS, n_terms outside 0..SD_OPTERM_MAX, op != 0 in the write form, an SD_F64 output with an imaginary coefficient or
 * a ComplexF64 psi, another dtype, a NULL vector, out aliasing psi, a sharded model, a model without device tables.  SD_EDIM: n is not
 * the basis dimension.  An empty list or a model with no rows gives a zero vector (b y with y) / zero expectations; the empty list has
 * K = 0 and writes nothing to out of sd_opstring_expect. */
#define SD_OPTERM_MAX 4096
#define SD_OPSTRING_MAX_OPS 256
typedef struct sd_opterm { uint64_t plus, minus, z; double c_re, c_im; int32_t op; int32_t reserved; } sd_opterm;
int sd_opstring_check(const sd_model *m, const sd_opterm *terms, int n_terms, int *n_ops, int *hermitian);
int sd_hamiltonian_terms(const sd_model *m, sd_opterm *out, int cap, int *n_terms);
int sd_opstring_apply(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi_host, int64_t n, const sd_opterm *terms, int n_terms,
                      const void *y_host, double b_re, double b_im, int dtype_out, void *out_host);
int sd_opstring_apply_dev(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi_dev, int64_t n, const sd_opterm *terms,
                          int n_terms, const void *y_dev, double b_re, double b_im, int dtype_out, void *out_dev);
int sd_opstring_expect(sd_ctx *ctx, const sd_model *m, int dtype, const void *bra_host, const void *ket_host, int64_t n,
                       const sd_opterm *terms, int n_terms, double *out);
int sd_opstring_expect_dev(sd_ctx *ctx, const sd_model *m, int dtype, const void *bra_dev, const void *ket_dev, int64_t n,
                           const sd_opterm *terms, int n_terms, double *out);
/* ---- S^z-basis statistics: participation moments, counting statistics, projective snapshots -------------------------------------
 * Everything here reads the weights w_s = |psi_s|^2 of the basis configurations s (site i is bit i - 1) in one streaming pass over
 * psi.  Nothing is divided by <psi|psi>.  Rows are in the basis order of sd_model_states, so "row r" means the same on every plan.
 * Fixed-nup sectors and the full basis; unsharded models only.
 *
 * sd_basis_moments: out (host, 5 + nq doubles) = sum_s w_s, sum_s w_s ln w_s (a term is 0 where w_s = 0), max_s w_s, the lowest row
 *   that attains the maximum (stored as a double, exact below 2^53), a reserved 0, then sum_s w_s^q for the nq exponents of `q`
 *   (0 .. SD_MOMENT_MAX_Q host doubles, each finite, > 0 and != 1: q = 1 is the Shannon term above).  q = 2, 3, 4 are formed by
 *   multiplication, other exponents by pow.  The maximum is compared as (w, -row) pairs, so ties go to the lowest row whatever the
 *   order of the comparisons.
 * sd_counting_range: host only (works on a model created without a context).  The values popcount(s & mask) takes on the basis:
 *   *m_min .. *m_min + *n_bins - 1.  In a sector, with a = popcount(mask): max(0, nup - (L - a)) .. min(a, nup); in the full basis
 *   0 .. a.  SD_EARG for a mask bit at or above L or a NULL pointer.
 * sd_counting_statistics: P_out (host, K (L + 1) doubles, every entry written) with P_out[k (L + 1) + m] = sum_s w_s [popcount(s &
 *   masks[k]) = m], m = 0 .. L, for the K masks (1 .. SD_COUNT_MAX_MASKS host uint64) of `masks`: the distribution of the number of
 *   up spins in subsystem k.  Bins outside a mask's range (sd_counting_range) are exact zeros.  A mask with more than
 *   SD_COUNT_MAX_BINS reachable values is SD_EARG (full basis, a subsystem of 33 or more sites).  All masks in one pass over psi.
 * sd_sample_uniforms_host: host only.  u_out[i] = the uniform of shot first + i of stream `seed`,
 *   (double)(mix64((seed ^ SALT) ^ mix64(k)) >> 11) * 2^-53 in [0, 1), mix64 the hash of the normal stream (sd_fill_randn_host) and SALT a
 *   fixed constant, exact in IEEE arithmetic: host and device agree to the bit.
 * sd_sample_configurations: `shots` rows drawn independently from w_s / sum w: rows_out[k] (host int64, may be NULL) and
 *   configs_out[k] (host uint64, the configuration of that row), k = 0 .. shots - 1.  Shot k has the target t_k = u_k W, W the
 *   library's own sum of the weights, and is the row at which the running sum of the weights, rows in basis order, first exceeds
 *   t_k: the rows are cut into fixed chunks of 1024 consecutive rows, the chunk weights are scanned (monotone non-decreasing), the
 *   chunk is found by bisection and walked in row order.  The result is a function of (psi, seed, shots) alone, not of the tile plan,
 *   and shot k does not depend on `shots`.  Every returned row lies in [0, N) and has w > 0.  shots = 0 writes nothing.
 * Sums in a fixed order: the same call gives the same bits.  _dev: psi is a device pointer; results go to host pointers and the call
 * synchronises the stream.
 * SD_EARG: an exponent <= 0, equal to 1 or not finite, nq outside 0..SD_MOMENT_MAX_Q, K outside 1..SD_COUNT_MAX_MASKS, a mask bit at or
 * above L, a mask with too many bins, shots < 0, a NULL pointer (rows_out excepted), a dtype other than SD_F64 / SD_C128, a sharded
 * model, a model without device tables.  SD_EDIM: n is not the basis dimension.  SD_EZERO: sd_sample_configurations of a vector
 * whose weights sum to zero (or to something not finite).  A model with no rows gives zeros. */
#define SD_MOMENT_MAX_Q 8
#define SD_COUNT_MAX_MASKS 256
#define SD_COUNT_MAX_BINS 33
int sd_basis_moments(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi_host, int64_t n, const double *q, int nq, double *out);
int sd_basis_moments_dev(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi_dev, int64_t n, const double *q, int nq, double *out);
int sd_counting_range(const sd_model *m, uint64_t mask, int *m_min, int *n_bins);
int sd_counting_statistics(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi_host, int64_t n, const uint64_t *masks, int K,
                           double *P_out);
int sd_counting_statistics_dev(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi_dev, int64_t n, const uint64_t *masks, int K,
                               double *P_out);
int sd_sample_uniforms_host(uint64_t seed, uint64_t first, int64_t n, double *u_out);
int sd_sample_configurations(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi_host, int64_t n, int64_t shots, uint64_t seed,
                             int64_t *rows_out, uint64_t *configs_out);
int sd_sample_configurations_dev(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi_dev, int64_t n, int64_t shots,
                                 uint64_t seed, int64_t *rows_out, uint64_t *configs_out);
/* ---- entanglement across a chain cut: the blocks of the reduced density matrix as Gram matrices ---------------------------------
 * The cut k (1 .. L-1) separates sites 1..k (part A, the low k bits of a configuration) from sites k+1..L (part B).  Write a
 * configuration s = (P, S) with the prefix P = s & (2^k - 1) and the suffix S = s >> k.  In a fixed-nup sector psi is, without a
 * copy, one dense matrix per number m of up spins in A:
 *     Psi_m[a, j] = psi[off_m[a] + j],   a < dA(m) = C(k, m),   j < dB(m) = C(L - k, nup - m),
 * off_m[a] the first row of the a-th prefix of popcount m: the rows that share a prefix are one contiguous run of the basis, the runs
 * of one m have the same length and the same internal order.  In the full basis there is one block, reported with m = -1:
 * Psi[a, j] = psi[j 2^k + a], dA = 2^k, dB = 2^(L-k).  The reduced density matrices are block diagonal,
 *     side A (SD_CUT_A): G_m[a][a'] = sum_j Psi_m[a, j] conj(Psi_m[a', j])      (rho_A = (+)_m G_m, dimension d = dA),
 *     side B (SD_CUT_B): G_m[j][j'] = sum_a Psi_m[a, j] conj(Psi_m[a, j'])      (rho_B = (+)_m G_m, dimension d = dB),
 * and both sides of a block have the same non-zero spectrum.  SD_CUT_AUTO takes, block by block, the side of the smaller dimension
 * (a tie goes to A).  The row order of a block is the order of first appearance in the basis: prefixes for A, suffix configurations
 * for B; in the full basis that is the integer value.  Nothing is divided by <psi|psi>.
 *
 * sd_cut_blocks: host only (works on a model created without a context).  *n_blocks = the number of blocks -- m = max(0, nup - (L -
 *   k)) .. min(k, nup) in a sector, one in the full basis -- and *n_elems = the matrix elements of the packed output, sum d^2.  With
 *   cap >= *n_blocks the records go to `out` in ascending m: m, the side in effect, dA, dB, d and the offset (in matrix elements) of
 *   the block in the packed output.  cap = 0: only the two counts.
 * sd_cut_plan_info: host only.  The launch plan of (model, cut, side): *n_items work items, the largest number of pieces *max_ns the
 *   summation range of a tile pair is cut into, and the bytes of the partial-sum workspace a call with `dtype` takes from the
 *   context's pool.  sd_cut_plan_items: the items themselves (cap = 0: only *n_items), sd_cut_segments: the start rows of the
 *   segments of block `block` (cap = 0: only *n_seg and *seg_len).  A segment is a run of rows with one prefix (sector; seg_len =
 *   dB) or one suffix (full basis; seg_len = 2^k).  An item is one (block, tile row ti, tile column tj >= ti, range [k0, k1) of the
 *   summation index) of the upper triangle of tile x tile output tiles, `slot` the offset (matrix elements) of its tile x tile
 *   partial sums in the workspace; piece `piece` of `ns`.  form 0 (ACROSS): the Gram index counts segments, the summation index runs
 *   inside a segment; form 1 (INSIDE): the Gram index runs inside a segment, the summation index counts segments.
 * sd_cut_gram: G_out (host) = the blocks packed at the offsets of sd_cut_blocks, each row-major d x d: SD_C128 as (re, im) pairs,
 *   exactly Hermitian with the diagonal's imaginary parts exactly 0; SD_F64 as d x d doubles, exactly symmetric.  Sums in a fixed
 *   order, no atomics: the same call gives the same bits.  _dev: psi is a device pointer; G_out is a host pointer and the call
 *   synchronises the stream.  sd_cut_gram_time_dev: the same launches on a device psi with the blocks left on the device and dropped;
 *   *kernel_ms = the device time of the Gram kernels and the reduction alone, between two events (profiles/entanglement_bench.py).
 * SD_EARG: a cut outside 1..L-1, a side other than the three, a dtype other than SD_F64 / SD_C128, a NULL pointer, 0 < cap < the
 * count, a block index outside the list, a sharded model, a model without device tables (sd_cut_gram), a block with d >
 * SD_CUT_MAX_DIM.  SD_EDIM: n is not the basis dimension.  SD_ENOMEM: the workspace does not fit; the context stays usable.  A
 * model with no rows gives zeros. */
#define SD_CUT_A 0
#define SD_CUT_B 1
#define SD_CUT_AUTO 2
#define SD_CUT_MAX_DIM 16384
typedef struct sd_cut_block { int32_t m, side; int64_t dA, dB, d, offset; } sd_cut_block;
typedef struct sd_cut_item { int32_t block, ti, tj, tile, form, piece, ns, reserved; int64_t k0, k1, slot; } sd_cut_item;
int sd_cut_blocks(const sd_model *m, int cut, int side, sd_cut_block *out, int cap, int *n_blocks, int64_t *n_elems);
int sd_cut_plan_info(const sd_model *m, int cut, int side, int dtype, int64_t *n_items, int *max_ns, int64_t *workspace_bytes);
int sd_cut_plan_items(const sd_model *m, int cut, int side, sd_cut_item *out, int64_t cap, int64_t *n_items);
int sd_cut_segments(const sd_model *m, int cut, int side, int block, int64_t *starts, int64_t cap, int64_t *n_seg, int64_t *seg_len);
int sd_cut_gram(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi_host, int64_t n, int cut, int side, void *G_out);
int sd_cut_gram_dev(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi_dev, int64_t n, int cut, int side, void *G_out);
int sd_cut_gram_time_dev(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi_dev, int64_t n, int cut, int side, double *kernel_ms);
/* ---- site permutations, and the entanglement of any set of sites ------------------------------------------------------------------
 * A site permutation pi is given as perm[0 .. L-1]: perm[i] is the 1-based site to which the spin of site i + 1 moves, a bijection of
 * 1..L.  U_pi |s> = |pi s>, so
 *     (U_pi psi)[idx(s)] = psi[idx(src(s))],   bit i of src(s) = bit (perm[i] - 1) of s.
 * perm[i] = (i + 1) mod L + 1 is the translation T, perm[i] = L - i the reflection R.  The number of up spins is preserved, so source
 * and target are the same model; fixed-nup sectors and the full basis; unsharded models only.  Every output element is bit for bit one
 * input element.
 *
 * sd_site_permute: out (n elements of psi's dtype, every row written) = U_pi psi.  out must not share a byte with psi (SD_EARG: identity
 *   and partial overlap alike).  _dev: device pointers, queued on the context's stream.
 * sd_site_permute_sources: host only (works on a model created without a context).  rows_out[k] = the row of psi that row start + k of
 *   the output copies, k < count, from the same byte table the kernel builds.
 * sd_subsystem_permutation: host only.  The permutation that brings a list of n_sites distinct sites to the front: sites[j] goes to
 *   site j + 1, in the order given, and the remaining sites go to n_sites + 1 .. L in ascending order.  perm_out: L ints.
 * sd_subsystem_gram: the blocks of the reduced density matrix of the listed sites (side SD_CUT_A), of the other sites (SD_CUT_B), or
 *   block by block of the smaller of the two (SD_CUT_AUTO): psi is permuted with sd_subsystem_permutation into one n-element vector
 *   taken from the context's pool, and the result goes through sd_cut_gram at cut = n_sites.  The block records and the packed layout of
 *   G_out are exactly those of sd_cut_blocks(m, n_sites, side, ...), with sites[j] playing site j + 1; sums, structure and determinism
 *   are sd_cut_gram's.  sites = 1..k in order: no copy is made and the result is sd_cut_gram's bit for bit.  _dev: psi is a device
 *   pointer; G_out is a host pointer and the call synchronises the stream.  The copy is a second vector: where two vectors do not fit
 *   (ComplexF64 at L = 36 on one card) the call returns SD_ENOMEM and the context stays usable.
 * SD_EARG: perm not a bijection of 1..L, sites not distinct or outside 1..L, n_sites outside 1..L-1, rows outside the basis, a NULL
 * pointer, a dtype other than SD_F64 / SD_C128, out sharing a byte with psi, a sharded model, a model without device tables, and what
 * sd_cut_gram refuses at cut = n_sites.  SD_EDIM: n is not the basis dimension.  A model with no rows gives empty vectors / zeros. */
int sd_site_permute(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi_host, int64_t n, const int *perm, void *out_host);
int sd_site_permute_dev(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi_dev, int64_t n, const int *perm, void *out_dev);
int sd_site_permute_sources(const sd_model *m, const int *perm, int64_t start, int64_t count, int64_t *rows_out);
int sd_subsystem_permutation(int L, const int *sites, int n_sites, int *perm_out);
int sd_subsystem_gram(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi_host, int64_t n, const int *sites, int n_sites, int side,
                      void *G_out);
int sd_subsystem_gram_dev(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi_dev, int64_t n, const int *sites, int n_sites,
                          int side, void *G_out);
/* create_spin_operator(site, op)(psi, model)   src/Hamiltonian.jl:49-136.  site is 1-based.  S^z is diagonal and works
 * in any basis; S^+, S^-, S^x, S^y change the magnetisation and are rejected in a fixed-nup sector (SD_EARG), as the
 * reference does.  out has psi's element type; S^y needs a ComplexF64 psi (SD_EARG otherwise: the reference's
 * accumulation of +-0.5im*psi into a Float64 result raises InexactError). */
#define SD_SPIN_Z 0
#define SD_SPIN_PLUS 1
#define SD_SPIN_MINUS 2
#define SD_SPIN_X 3
#define SD_SPIN_Y 4
int sd_spin_operator(sd_ctx *ctx, const sd_model *m, int dtype, int site, int op, const void *psi_host, int64_t n,
                     void *out_host);
/* InitialStates (src/InitialStates.jl:9-130): 0-based basis index of the one-hot state; SD_EARG when the
 * configuration is not in the basis.  flips: 1-based sites for SD_STATE_POLARIZED_FLIPS. */
#define SD_STATE_DOMAIN_WALL 0
#define SD_STATE_NEEL 1
#define SD_STATE_POLARIZED_UP 2
#define SD_STATE_POLARIZED_DOWN 3
#define SD_STATE_POLARIZED_FLIPS 4
int sd_initial_state_index(const sd_model *m, int kind, const int *flips, int nflips, int64_t *idx0_out);

/* ---- host utilities ------------------------------------------------------ */
/* eigen(SymTridiagonal(d, e)): ascending eigenvalues w[n]; z (n*n column-major) may be NULL */
int sd_symtridiag_eig(int n, const double *d, const double *e, double *w, double *z);
/* eigen(Symmetric(A)) by cyclic Jacobi rotations, n <= 128: A is n*n (column-major; the lower triangle is read), ascending
 * eigenvalues w[n], eigenvectors in the columns of Z (n*n column-major).  The projected matrix of a restarted Lanczos basis is
 * arrowhead plus tridiagonal, which sd_symtridiag_eig cannot take.  SD_EARG: n outside 1..128 or a NULL pointer. */
int sd_sym_eig(int n, const double *A, double *w, double *Z);
/* Chebyshev expansion coefficients c_k = (2 - delta_k0) (-i)^k J_k(a dt) exp(-i b dt), k < cheb_n (src/TimeEvolution/Chebyshev.jl:
 * 74-79); c_out has 2*cheb_n doubles (re, im).  The contract every real-time Chebyshev entry point inherits:
 *   accuracy  J_k is the Bessel function of the Float64 product a * dt, all orders from one backward recurrence in extended
 *             precision, rounded once: |c_k - exact| <= 4 * 2^-53 at b = 0, <= 8 * 2^-53 with the phase (cos, sin of the Float64
 *             product b * dt), at every |a dt| <= 1e6 and every k.  The call is O(|a dt| + cheb_n).
 *   sign      dt < 0 evolves backwards: J_k(-z) = (-1)^k J_k(z), and c(-dt) is the complex conjugate of c(dt) bit for bit.
 *   cap       SD_EARG for |a dt| > 1e6, a, b or dt not finite, cheb_n < 1 or c_out NULL; nothing else fails but allocation.
 * sd_chebyshev_terms: *n_terms = the first k with k > |z| and |J_k(z)| < 2^-53 -- the term count that cheb_n = 0 stands for in
 * sd_dqt_correlations, exact at every |z| <= 1e6 (the rule is read off the same recurrence, with no search cap); SD_EARG for
 * |z| > 1e6, a NaN or n_terms NULL. */
int sd_chebyshev_coeffs(int cheb_n, double a, double b, double dt, double *c_out);
int sd_chebyshev_terms(double z, int *n_terms);
/* counter-based N(0,1) generator used for synthetic vectors: element k of the
 * stream (seed) -- identical on host and device, independent of sharding. */
int sd_fill_randn_dev(sd_ctx *ctx, void *x_dev, int64_t n_doubles, uint64_t seed, uint64_t first_index);
int sd_fill_randn_host(double *x, int64_t n_doubles, uint64_t seed, uint64_t first_index);
/* dot(x, y) = sum conj(x_k) y_k and sum |x_k|^2 over n elements of device vectors (LinearAlgebra.dot / norm^2 as the
 * recursions use them, e.g. src/Lanczos.jl:40,55,59), reduced in a fixed order (same inputs -> same bits, any n up to
 * 2^62).  out_re_im[2] / out[1] are host doubles; the call synchronises the stream. */
int sd_dot_dev(sd_ctx *ctx, int dtype, const void *x_dev, const void *y_dev, int64_t n, double *out_re_im);
int sd_nrm2sq_dev(sd_ctx *ctx, int dtype, const void *x_dev, int64_t n, double *out);

/* ---- index-range sharding (multi-GPU; one process per GPU) -------------- */
/* A shard owns the contiguous basis-index range [row_lo, row_hi) (aligned to
 * tile boundaries).  Vectors of a sharded model are device arrays of
 * n_local + n_halo elements: the first n_local are the owned rows, the tail is
 * the halo filled by the exchange (RCCL send/recv driven by the host layer)
 * before each apply.  The plan lists contiguous slabs to send / receive. */
typedef struct sd_shard_info {
  int rank, nranks;
  int64_t row_lo, row_hi;   /* owned global rows */
  int64_t n_local, n_halo;  /* elements */
  int64_t n_recv_slabs, n_send_slabs;
  int mode;                 /* 0 index ranges (send slabs are slices of psi), 1 popcount cells (send slabs are slices
                               of the packed send buffer filled by sd_shard_pack_dev) */
  int64_t n_send;           /* elements of the packed send buffer (mode 1), else 0 */
  int64_t n_local_tiles;
  int64_t n_pack;           /* entries of the pack list (mode 1) */
  int64_t n_interior_tiles; /* tiles whose hop partners are all owned (sd_apply_sharded_dev part 1) */
  int64_t n_interior_rows;  /* rows of those tiles (the rest of n_local waits for the halo) */
  int64_t packed;           /* mode 1: 1 = the send slabs index the packed send buffer (sd_shard_pack_dev, n_send elements); 0 = they index the
                               vector itself -- the tiles a peer needs form long contiguous runs, one slab per run, no pack, no send buffer */
} sd_shard_info;
typedef struct sd_slab {
  int peer;                 /* rank on the other side */
  int64_t local_offset;     /* element offset in THIS rank's vector (send: within owned rows; recv: >= n_local) */
  int64_t count;            /* elements */
  int64_t global_row;       /* global basis index of the slab's first element */
} sd_slab;
/* Re-plans the model as shard `rank` of `nranks` (nranks == 1 restores the
 * unsharded plan).  Must be called before any apply on that model.  On failure
 * (SD_ENOMEM, SD_EHIP, ...) the model is left WITHOUT a plan: every later call
 * that needs one returns SD_EARG; destroy the model (or call set_shard again). */
int sd_model_set_shard(sd_model *m, int rank, int nranks);
/* One KPM moment step on a shard (src/KPM_Sqw.jl:106-117), ComplexF64 device vectors of n_local elements:
 * first != 0: v_next = (H v_curr - b v_curr)/a; else v_next = 2 (H v_curr - b v_curr)/a - v_prev.
 * sums_out[0..1] = this rank's { Re<phi|v_next>, |v_next|^2 }: all-reduce over the ranks for mu_n and the norm. */
int sd_kpm_step_sharded_dev(sd_ctx *ctx, const sd_model *m, void *v_next_dev, const void *v_curr_dev, const void *halo_dev,
                            const void *v_prev_dev, const void *phi_dev, int64_t n_local, double a, double b, int first,
                            double *sums_out);
/* mode: -1 auto (env SD_SHARD_MODE=range|class, default class when the model allows it), 0 index ranges, 1 popcount cells */
int sd_model_set_shard_mode(sd_model *m, int rank, int nranks, int mode);
/* local tiles in natural order: offset in the local vector, GLOBAL basis index of the first row, rows (arrays of
 * sd_shard_info.n_local_tiles entries; any may be NULL).  local row = local_base + i  <->  global row = global_base + i */
int sd_model_local_tiles(const sd_model *m, int64_t *local_base, int64_t *global_base, int32_t *len);
/* mode 1: the pack list -- tile k of it is psi[src[k] .. src[k]+len[k]) -> sendbuf[dst[k] ..) (n_pack entries each) */
int sd_model_shard_pack_list(const sd_model *m, int64_t *src, int64_t *dst, int32_t *len);
/* mode 1: gather the tiles the peers need into the contiguous send buffer (n_send elements) */
int sd_shard_pack_dev(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi_dev, void *sendbuf_dev);
/* counter-based N(0,1) keyed by the GLOBAL element index into this shard's local vector (any sharding gives the same state) */
int sd_fill_randn_local_dev(sd_ctx *ctx, const sd_model *m, int dtype, void *x_dev, uint64_t seed);
/* Sharded apply with the imported partner tiles in a SEPARATE halo buffer (n_halo elements, filled by the exchange):
 * vectors then hold exactly n_local elements and one halo buffer serves every vector of a recursion.
 * epilogue: 0 out = H psi; 1 out = (H psi - b psi)/a; 2 fused Chebyshev term (ComplexF64; phi_prev, psi_t as in
 * sd_cheb_step_dev); 3 recurrence only, out = 2 (H psi - b psi)/a - phi_prev (psi_t untouched).  part: 0 all tiles; 1 only the interior tiles (every hop partner owned: reads no halo, so it
 * can run while the exchange is in flight); 2 only the boundary tiles.  All pointers are device pointers. */
int sd_apply_sharded_dev(sd_ctx *ctx, const sd_model *m, int dtype, void *out_dev, const void *psi_dev,
                         const void *halo_dev, int64_t n_local, int epilogue, double a, double b,
                         double c_re, double c_im, const void *phi_prev_dev, void *psi_t_dev, int part);
/* The pair form of the Chebyshev term (src/TimeEvolution/Chebyshev.jl:110-121): sd_apply_sharded_dev with epilogue 3
 * computes phi_k = 2 H~ phi_{k-1} - phi_{k-2} without touching psi_t; this call then computes
 * out = phi_{k+1} = 2 H~ psi - phi_prev (psi = phi_k) and psi_t += c0*phi_k; psi_t += c*phi_{k+1}, in that order --
 * the same bits as one accumulation per term, with psi_t read and written once per two terms. */
int sd_apply_sharded_cheb2_dev(sd_ctx *ctx, const sd_model *m, void *out, const void *psi, const void *halo, int64_t n_local,
                               double a, double b, double c0_re, double c0_im, double c_re, double c_im,
                               const void *phi_prev, void *psi_t, int part);
int sd_model_shard_info(const sd_model *m, sd_shard_info *out);
int sd_model_shard_slabs(const sd_model *m, sd_slab *recv_out, sd_slab *send_out);

/* ---- sharded recursions (one process per GPU) ------------------------------------------------------------------
 * The reference has no distributed layer (its only parallel construct above apply_H! is the thread loop over the momenta,
 * src/KPM_Sqw.jl:218).  These are the recursion-level entry points of above for a model re-planned with
 * sd_model_set_shard[_mode]: every vector argument is this rank's OWNED part (n_local elements, device pointer), every
 * rank makes the same call, scalars come back identical on all ranks.  A sd_comm says how halos travel and scalars are
 * summed; with the RCCL communicator a recursion step (pack, grouped send/recv beside the interior tiles, boundary tiles,
 * BLAS-1 passes, ncclAllReduce of the device scalars) is queued without touching the host.  Halo and send buffers come
 * from the context's pool: per rank a recursion holds its vectors (n_local elements each) + n_halo + n_send elements. */
typedef struct sd_comm sd_comm;
typedef struct sd_comm_callbacks {
  void *user;
  /* Post the halo exchange: for every send slab of this rank (sd_model_shard_slabs) send src_dev[local_offset ..
   * local_offset+count) to slab.peer, for every recv slab receive into halo_dev[local_offset - n_local ..).  src_dev is the
   * vector itself (mode 0) or the packed send buffer (mode 1); elements are dtype-sized; both are device pointers whose
   * producers are queued on the context's stream.  May return before the bytes have moved. */
  int (*exchange_start)(void *user, int dtype, const void *src_dev, void *halo_dev);
  /* Return once work queued on the context's stream after this call is ordered behind the completed exchange. */
  int (*exchange_wait)(void *user);
  /* vals[0..count) <- sum over all ranks (host memory; count <= 16). */
  int (*allreduce_sum)(void *user, double *vals, int count);
} sd_comm_callbacks;
/* nonzero return of a callback aborts the call with SD_ECOMM */
int sd_comm_from_callbacks(const sd_comm_callbacks *cb, int rank, int nranks, sd_comm **out);
/* RCCL over xGMI.  Rank 0 obtains a 128-byte id (ncclGetUniqueId) and hands it to the other ranks by any means (the
 * Julia front-end: Distributed / MPI; the Python mirror: torch.distributed broadcast); every rank then creates its
 * communicator on its context's device.  Collective: all nranks must call. */
int sd_comm_rccl_unique_id(void *id128);
int sd_comm_rccl_create(sd_ctx *ctx, int rank, int nranks, const void *id128, sd_comm **out);
void sd_comm_destroy(sd_comm *comm);
/* Routed halo exchange (RCCL communicator).  By default an exchange is one grouped ncclSend / ncclRecv of the model's slab lists
 * (sd_model_shard_slabs): every (owner, receiver) pair's bytes ride the one xGMI link that joins the pair, and the busiest pair
 * carries two to three times the mean.  This installs an explicit list instead: operations in ascending `batch` order, one RCCL
 * group per batch on the exchange stream, `buf` naming what `offset` (in elements) counts from -- 0 the vector handed to the
 * exchange (sends only), 1 the halo buffer (receives only), 2 this rank's relay buffer of `relay_elems` elements (a piece
 * received in batch b is forwarded in batch b + 1).  Every rank must install lists that pair up (the Python mirror builds them
 * from one routing plan: dist.relay_routes / dist.relay_ops).  n_ops == 0 restores the default. */
typedef struct sd_xop {
  int batch;        /* ascending through the list */
  int peer;
  int kind;         /* 0 send, 1 receive */
  int buf;          /* 0 vector, 1 halo, 2 relay buffer */
  int64_t offset;   /* elements from the start of that buffer */
  int64_t count;    /* elements */
} sd_xop;
int sd_comm_set_exchange_ops(sd_comm *comm, const sd_xop *ops, int64_t n_ops, int64_t relay_elems);
/* Diagnostic (RCCL communicator): ncclAllReduce of two device doubles and a grouped ncclSend/ncclRecv round the ring of ranks
 * (rank -> rank+1; to itself with nranks == 1), bytes checked.  Collective: with more than one rank all of them must call it. */
int sd_comm_selftest(sd_ctx *ctx, sd_comm *comm);

/* out = H psi on the owned rows, halo exchange included (overlapped with the interior tiles when overlap != 0). */
int sd_apply_sharded(sd_ctx *ctx, const sd_model *m, sd_comm *comm, int dtype, void *out_dev, const void *psi_dev,
                     int64_t n_local, int overlap);
/* lanczos_extremal / estimate_energy_bounds (src/Lanczos.jl:27-84, 255-271); psi0_dev NULL: counter-based N(0,1) start
 * vector keyed by the global row index (the same state for every sharding). */
int sd_lanczos_extremal_sharded(sd_ctx *ctx, const sd_model *m, sd_comm *comm, int lanc_m, double tol, const void *psi0_dev,
                                uint64_t seed, int negate, double *emin, double *emax);
int sd_energy_bounds_sharded(sd_ctx *ctx, const sd_model *m, sd_comm *comm, int lanc_m, uint64_t seed, double *Emin,
                             double *Emax);
/* chebyshev_time_evolve (src/TimeEvolution/Chebyshev.jl:61-124) on ComplexF64 shards; psit_dev may alias psi0_dev. */
int sd_chebyshev_evolve_sharded(sd_ctx *ctx, const sd_model *m, sd_comm *comm, const void *psi0_dev, int64_t n_local,
                                double dt, int cheb_n, double Emin, double Emax, void *psit_dev);
/* krylov_time_evolve (src/TimeEvolution/Krylov.jl:136-192) on shards (psit ComplexF64). */
int sd_krylov_evolve_sharded(sd_ctx *ctx, const sd_model *m, sd_comm *comm, int dtype, const void *psi0_dev,
                             int64_t n_local, double dt, int kry_m, void *psit_dev);
/* compute_chebyshev_moments (src/KPM_Sqw.jl:95-128): phi_dev normalised over all ranks; mu (host, M entries) on every rank. */
int sd_kpm_moments_sharded(sd_ctx *ctx, const sd_model *m, sd_comm *comm, const void *phi_dev, int64_t n_local, int M,
                           double a, double b, double *mu);
/* kpm_sqw (src/KPM_Sqw.jl:191-256) on a sharded psi0 (BASELINE config 5); Smat (host, Qn x W row-major) on every rank. */
int sd_kpm_sqw_sharded(sd_ctx *ctx, const sd_model *m, sd_comm *comm, int dtype, const void *psi0_dev, int64_t n_local,
                       const double *q, int Qn, const double *omega, int W, int have_ab, double a, double b, int kpm_m,
                       int kernel, uint64_t seed, double *Smat);
/* <x|y> (re, im) and |x|^2 over all ranks */
int sd_dot_sharded(sd_ctx *ctx, sd_comm *comm, int dtype, const void *x_dev, const void *y_dev, int64_t n_local,
                   double *out2);

#ifdef __cplusplus
}
#endif
#endif /* SPINDYN_H */
