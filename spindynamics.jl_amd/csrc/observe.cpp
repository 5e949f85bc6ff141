// One-pass observables: the host side of the calls that read a state once and need no operator loop -- spin current and energy
// current, pair correlations (15), bond operators and dimer correlations (16), lattice symmetry operators (18),
// operator strings (19), S^z-basis statistics (20).  Every core is the same few steps on the helpers of host_calls.hpp: the
// model check, the entry's own argument checks in the order its contract (include/spindyn.h) states them, the vectors staged, one
// launch, the result delivered.  The recursions are in recur.cpp.
#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "host_calls.hpp"

int current_weights(sd_ctx *ctx, const sd_model *m, const double *w, DBuf &wt) {
  const size_t nh = m->hop_J.size();
  std::vector<double> h(std::max<size_t>(nh, 1), 0.0);
  for (size_t b = 0; b < nh; ++b) {
    if (w && !std::isfinite(w[b])) return sd_set_err(ctx, SD_EARG, "current weights must be finite");
    h[b] = w ? w[b] * m->hop_J[b] : m->hop_J[b];
  }
  RC(wt.alloc(ctx, (int64_t)h.size()));
  return h2d(ctx, wt.p, h.data(), (int64_t)h.size());
}

int DList::init(sd_ctx *ctx, const sd_model *m, const sd_dterm *list, int n_terms) {
  if (n_terms < 0 || n_terms > SD_DTERM_MAX) return sd_set_err(ctx, SD_EARG, "the number of terms must be in 0..SD_DTERM_MAX");
  if (n_terms > 0 && !list) return sd_set_err(ctx, SD_EARG, "null argument");
  std::vector<sd_dgroup> g;
  std::vector<sd_dterm_dev> t((size_t)n_terms);
  for (int n = 0; n < n_terms; ++n) {
    const sd_dterm &T = list[n];
    if (T.i < 1 || T.i > m->L || T.j < 1 || T.j > m->L || T.k < 0 || T.k > m->L) return sd_set_err(ctx, SD_EARG, "a site of a term is outside 1..L (k may also be 0)");
    if (T.i == T.j) return sd_set_err(ctx, SD_EARG, "the two sites of a bond current must differ");
    if (T.k == T.i || T.k == T.j) return sd_set_err(ctx, SD_EARG, "the S^z site of a term must not be one of its bond's sites");
    if (!std::isfinite(T.c)) return sd_set_err(ctx, SD_EARG, "the coefficients must be finite");
    if (n == 0 || T.i != list[n - 1].i || T.j != list[n - 1].j) {
      const int lo = std::min(T.i, T.j) - 1, hi = std::max(T.i, T.j) - 1;
      g.push_back(sd_dgroup{lo | (hi << 8) | ((T.i > T.j ? 1 : 0) << 16), n, 0, 0});
    }
    ++g.back().count;
    t[(size_t)n] = sd_dterm_dev{T.k == 0 ? T.c : 0.5 * T.c, T.k - 1, 0};
  }
  n_groups = (int)g.size();
  if (n_groups == 0) return SD_OK;
  const int ig = tab.add(g.data(), g.size()), it = tab.add(t.data(), t.size());
  RC(tab.upload(ctx));
  groups = tab.at<sd_dgroup>(ig);
  terms = tab.at<sd_dterm_dev>(it);
  return SD_OK;
}

namespace {

// write form (bra == null): out (ComplexF64, n) = J_w vec; bracket form: out[0..1] (host) = <bra|J_w|vec>, vec ComplexF64
int current_core(sd_ctx *ctx, const sd_model *m, int dtype, const void *vec, const void *bra, bool bracket, int64_t n, const double *w,
                 void *out, bool on_dev) {
  RC(check_unsharded_model(ctx, m));
  if (n != m->N) return sd_set_err(ctx, SD_EDIM, "vector length does not match the basis dimension");
  if (!out) return sd_set_err(ctx, SD_EARG, "null argument");
  if (!bracket && on_dev && out == vec) return sd_set_err(ctx, SD_EARG, "out must not alias psi");
  DBuf wt, res;
  DevIn v, b;
  RC(current_weights(ctx, m, w, wt));
  RC(v.stage(ctx, bracket ? SD_C128 : dtype, vec, on_dev, n));
  if (bracket) {
    RC(b.stage(ctx, dtype, bra, on_dev, n));
    RC(res.alloc(ctx, 2));
    RC(sd_launch_current(ctx, m, dtype, v.p, b.p, wt.p, nullptr, res.p));
    return read_back(ctx, out, res.p, 2 * sizeof(double));
  }
  DevOut o;
  RC(o.open(ctx, out, on_dev, 2 * n));
  RC(sd_launch_current(ctx, m, dtype, v.p, nullptr, wt.p, o.p, nullptr));
  return o.close(true);                                    // the weights go back to the pool
}

// write form (bra == null): out (ComplexF64, n) = J vec; bracket form: out[0..1] (host) = <bra|J|vec>, vec ComplexF64
int dcurrent_core(sd_ctx *ctx, const sd_model *m, int dtype, const void *vec, const void *bra, bool bracket, int64_t n,
                  const sd_dterm *list, int n_terms, void *out, bool on_dev) {
  RC(check_unsharded_model(ctx, m));
  if (dtype != SD_F64 && dtype != SD_C128) return sd_set_err(ctx, SD_EARG, "dtype must be SD_F64 or SD_C128");
  if (n != m->N) return sd_set_err(ctx, SD_EDIM, "vector length does not match the basis dimension");
  if (!out || !vec) return sd_set_err(ctx, SD_EARG, "null argument");
  if (!bracket && on_dev && out == vec) return sd_set_err(ctx, SD_EARG, "out must not alias psi");
  DList dl;
  RC(dl.init(ctx, m, list, n_terms));
  DBuf res;
  DevIn v, b;
  RC(v.stage(ctx, bracket ? SD_C128 : dtype, vec, on_dev, n));
  if (bracket) {
    RC(b.stage(ctx, dtype, bra, on_dev, n));
    RC(res.alloc(ctx, 2));
    RC(sd_launch_dcurrent(ctx, m, dtype, v.p, b.p, dl.groups, dl.n_groups, dl.terms, nullptr, res.p));
    return read_back(ctx, out, res.p, 2 * sizeof(double));
  }
  DevOut o;
  RC(o.open(ctx, out, on_dev, 2 * n));
  RC(sd_launch_dcurrent(ctx, m, dtype, v.p, nullptr, dl.groups, dl.n_groups, dl.terms, o.p, nullptr));
  return o.close(true);                                    // the tables go back to the pool
}

// M_out (host, 2 L L doubles) = the L x L pair-correlation matrix of psi: the kernel sums the pairs i <= j, the other triangle is
// the conjugate
int pair_correlations_core(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi, int64_t n, int component, double *M_out,
                           bool on_dev) {
  RC(check_unsharded_model(ctx, m));
  if (component != SD_PAIR_ZZ && component != SD_PAIR_PM) return sd_set_err(ctx, SD_EARG, "component must be SD_PAIR_ZZ or SD_PAIR_PM");
  if (n != m->N) return sd_set_err(ctx, SD_EDIM, "vector length does not match the basis dimension");
  if (!M_out) return sd_set_err(ctx, SD_EARG, "null argument");
  DevIn in;
  TableBlock plist;
  DBuf res;
  RC(in.stage(ctx, dtype, psi, on_dev, n));
  const int L = m->L;
  std::vector<int> pairs;
  for (int i = 0; i < L; ++i)
    for (int j = i; j < L; ++j) pairs.push_back(i | (j << 8));
  const int np = (int)pairs.size();
  plist.add(pairs.data(), pairs.size());
  RC(plist.upload(ctx));
  RC(res.alloc(ctx, 2 * (int64_t)np));
  RC(sd_launch_pair_correlations(ctx, m, dtype, in.p, component, plist.at<int>(0), np, res.p));
  std::vector<double> h(2 * (size_t)np);
  RC(read_back(ctx, h.data(), res.p, sizeof(double) * h.size()));
  for (int k = 0; k < np; ++k) {
    const int i = pairs[k] & 255, j = pairs[k] >> 8;
    const double re = h[2 * (size_t)k], im = h[2 * (size_t)k + 1];
    double *a = M_out + 2 * ((size_t)i * L + j), *b = M_out + 2 * ((size_t)j * L + i);
    b[0] = re; b[1] = im == 0.0 ? 0.0 : -im;
    a[0] = re; a[1] = im;
  }
  return SD_OK;
}

// ---- S^z-basis statistics (kernels_basis_stats.hip) ----
int basis_moments_core(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi, int64_t n, const double *q, int nq, double *out,
                       bool on_dev) {
  RC(check_unsharded_model(ctx, m));
  if (n != m->N) return sd_set_err(ctx, SD_EDIM, "vector length does not match the basis dimension");
  if (!out || (nq > 0 && !q)) return sd_set_err(ctx, SD_EARG, "null argument");
  if (nq < 0 || nq > SD_MOMENT_MAX_Q) return sd_set_err(ctx, SD_EARG, "basis moments: between 0 and SD_MOMENT_MAX_Q exponents");
  DevIn in;
  DBuf res;
  RC(in.stage(ctx, dtype, psi, on_dev, n));
  RC(res.alloc(ctx, 5 + SD_MOMENT_MAX_Q));
  RC(sd_launch_basis_moments(ctx, m, dtype, in.p, q, nq, res.p));
  return read_back(ctx, out, res.p, sizeof(double) * (size_t)(5 + nq));
}

int counting_statistics_core(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi, int64_t n, const uint64_t *masks, int K,
                             double *P_out, bool on_dev) {
  RC(check_unsharded_model(ctx, m));
  if (n != m->N) return sd_set_err(ctx, SD_EDIM, "vector length does not match the basis dimension");
  if (!P_out || !masks) return sd_set_err(ctx, SD_EARG, "null argument");
  if (K < 1 || K > SD_COUNT_MAX_MASKS) return sd_set_err(ctx, SD_EARG, "counting statistics: between 1 and SD_COUNT_MAX_MASKS masks");
  DevIn in;
  DBuf res;
  RC(in.stage(ctx, dtype, psi, on_dev, n));
  const int64_t np = (int64_t)K * (m->L + 1);
  RC(res.alloc(ctx, np));
  RC(sd_launch_counting_statistics(ctx, m, dtype, in.p, masks, K, res.p));
  return read_back(ctx, P_out, res.p, sizeof(double) * (size_t)np);
}

int sample_configurations_core(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi, int64_t n, int64_t shots, uint64_t seed,
                               int64_t *rows_out, uint64_t *configs_out, bool on_dev) {
  RC(check_unsharded_model(ctx, m));
  if (n != m->N) return sd_set_err(ctx, SD_EDIM, "vector length does not match the basis dimension");
  if (shots < 0) return sd_set_err(ctx, SD_EARG, "snapshots: a negative number of shots");
  if (shots > 0 && !configs_out) return sd_set_err(ctx, SD_EARG, "null argument");
  DevIn in;
  DBuf res;
  RC(in.stage(ctx, dtype, psi, on_dev, n));
  RC(res.alloc(ctx, 2 * std::max<int64_t>(shots, 1)));     // rows, then configurations: 8 bytes each
  int64_t *rows_dev = (int64_t *)res.p;
  uint64_t *cfg_dev = (uint64_t *)(res.p + std::max<int64_t>(shots, 1));
  RC(sd_launch_sample_configurations(ctx, m, dtype, in.p, shots, seed, rows_dev, cfg_dev));
  if (shots == 0) return SD_OK;
  if (rows_out) SD_HIP(ctx, hipMemcpyAsync(rows_out, rows_dev, sizeof(int64_t) * (size_t)shots, hipMemcpyDeviceToHost, ctx->stream));
  return read_back(ctx, configs_out, cfg_dev, sizeof(uint64_t) * (size_t)shots);
}

// the 0-based bits lo < hi of the bond of the 1-based sites (i, j): D_b is symmetric in its two sites
int bond_bits(sd_ctx *ctx, const sd_model *m, int i, int j, int *lo, int *hi) {
  if (i < 1 || i > m->L || j < 1 || j > m->L) return sd_set_err(ctx, SD_EARG, "a bond site is outside 1..L");
  if (i == j) return sd_set_err(ctx, SD_EARG, "the two sites of a bond must differ");
  *lo = std::min(i, j) - 1; *hi = std::max(i, j) - 1;
  return SD_OK;
}

// out (n elements of psi's dtype) = D_b psi, b = (i, j)
int bond_apply_core(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi, int64_t n, int i, int j, double xy, double zz, void *out,
                    bool on_dev) {
  RC(check_unsharded_model(ctx, m));
  if (dtype != SD_F64 && dtype != SD_C128) return sd_set_err(ctx, SD_EARG, "dtype must be SD_F64 or SD_C128");
  int lo = 0, hi = 0;
  RC(bond_bits(ctx, m, i, j, &lo, &hi));
  if (!std::isfinite(xy) || !std::isfinite(zz)) return sd_set_err(ctx, SD_EARG, "the bond weights must be finite");
  if (n != m->N) return sd_set_err(ctx, SD_EDIM, "vector length does not match the basis dimension");
  if (!out) return sd_set_err(ctx, SD_EARG, "null argument");
  if (on_dev && out == psi) return sd_set_err(ctx, SD_EARG, "out must not alias psi");
  DevIn in;
  DevOut o;
  RC(in.stage(ctx, dtype, psi, on_dev, n));
  RC(o.open(ctx, out, on_dev, vec_doubles(dtype, n)));
  RC(sd_launch_bond_apply(ctx, m, dtype, in.p, lo, hi, xy, zz, o.p));
  return o.close(true);                                    // no pool block is in flight: see the table of DESIGN.md 4.5
}

// D_out (host, 2 B B doubles) = the B x B dimer matrix of psi, e_out (host, B doubles) the bond expectation values: the kernel sums
// the tiles of the upper triangle of 4-bond chunks (inside a diagonal tile a <= b is used), the other triangle is the conjugate
int dimer_correlations_core(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi, int64_t n, const int *bonds, int B, double xy,
                            double zz, double *D_out, double *e_out, bool on_dev) {
  RC(check_unsharded_model(ctx, m));
  if (dtype != SD_F64 && dtype != SD_C128) return sd_set_err(ctx, SD_EARG, "dtype must be SD_F64 or SD_C128");
  if (B < 1 || B > SD_DIMER_MAX_BONDS) return sd_set_err(ctx, SD_EARG, "the number of bonds must be in 1..SD_DIMER_MAX_BONDS");
  if (!bonds || !D_out || !e_out) return sd_set_err(ctx, SD_EARG, "null argument");
  std::vector<int> packed((size_t)B);
  for (int b = 0; b < B; ++b) {
    int lo = 0, hi = 0;
    RC(bond_bits(ctx, m, bonds[2 * b], bonds[2 * b + 1], &lo, &hi));
    packed[(size_t)b] = lo | (hi << 8);
  }
  if (!std::isfinite(xy) || !std::isfinite(zz)) return sd_set_err(ctx, SD_EARG, "the bond weights must be finite");
  if (n != m->N) return sd_set_err(ctx, SD_EDIM, "vector length does not match the basis dimension");
  DevIn in;
  TableBlock blist;
  DBuf res;
  RC(in.stage(ctx, dtype, psi, on_dev, n));
  blist.add(packed.data(), packed.size());
  RC(blist.upload(ctx));
  const int ntiles = sd_dimer_tiles(B), nch = (B + 3) / 4;
  RC(res.alloc(ctx, (int64_t)ntiles * SD_DIMER_TILE_ROW));
  RC(sd_launch_dimer_gram(ctx, m, dtype, in.p, blist.at<int>(0), B, xy, zz, res.p));
  std::vector<double> h((size_t)ntiles * SD_DIMER_TILE_ROW);
  RC(read_back(ctx, h.data(), res.p, sizeof(double) * h.size()));
  size_t t = 0;
  for (int ca = 0; ca < nch; ++ca)
    for (int cb = ca; cb < nch; ++cb, ++t) {
      const double *row = h.data() + t * SD_DIMER_TILE_ROW;
      for (int ka = 0; ka < 4 && 4 * ca + ka < B; ++ka) {
        const int a = 4 * ca + ka;
        if (ca == cb) e_out[a] = row[32 + ka];
        for (int kb = (ca == cb ? ka : 0); kb < 4 && 4 * cb + kb < B; ++kb) {
          const int b = 4 * cb + kb;
          const double re = row[2 * (4 * ka + kb)], im = row[2 * (4 * ka + kb) + 1];
          double *up = D_out + 2 * ((size_t)a * B + b), *dn = D_out + 2 * ((size_t)b * B + a);
          dn[0] = re; dn[1] = im == 0.0 ? 0.0 : -im;
          up[0] = re; up[1] = im;
        }
      }
    }
  return SD_OK;
}

// ---- lattice symmetry operators (kernels_symmetry.hip) ----
int sym_code(sd_ctx *ctx, const sd_model *m, int code) {
  std::string err;
  const int rc = sd_symmetry_check_code(m, code, err);
  return rc ? sd_set_err(ctx, rc, err) : SD_OK;
}

// a validated element list on the device: the coefficients (2 n doubles, when given) first, then the n codes
struct SymList {
  TableBlock tab;
  const int *codes = nullptr;
  const double *coef = nullptr;
  bool all_real = true;
  int init(sd_ctx *ctx, const sd_model *m, const int *list, const double *c, int n) {
    if (n < 1 || n > SD_SYM_MAX_ELEMENTS) return sd_set_err(ctx, SD_EARG, "the number of elements must be in 1..SD_SYM_MAX_ELEMENTS");
    if (!list) return sd_set_err(ctx, SD_EARG, "null argument");
    for (int k = 0; k < n; ++k) {
      RC(sym_code(ctx, m, list[k]));
      if (c && (!std::isfinite(c[2 * k]) || !std::isfinite(c[2 * k + 1]))) return sd_set_err(ctx, SD_EARG, "the coefficients must be finite");
      if (c && c[2 * k + 1] != 0.0) all_real = false;
    }
    const int ic = c ? tab.add(c, 2 * (size_t)n) : -1, il = tab.add(list, (size_t)n);
    RC(tab.upload(ctx));
    coef = c ? tab.at<double>(ic) : nullptr;
    codes = tab.at<int>(il);
    return SD_OK;
  }
};

// out (n elements of psi's dtype) = U_g psi (+ c y)
int symmetry_apply_core(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi, int64_t n, int code, const void *y, double cr,
                        double ci, void *out, bool on_dev) {
  RC(check_unsharded_model(ctx, m));
  if (dtype != SD_F64 && dtype != SD_C128) return sd_set_err(ctx, SD_EARG, "dtype must be SD_F64 or SD_C128");
  RC(sym_code(ctx, m, code));
  if (y && (!std::isfinite(cr) || !std::isfinite(ci))) return sd_set_err(ctx, SD_EARG, "the coefficient must be finite");
  if (y && dtype == SD_F64 && ci != 0.0) return sd_set_err(ctx, SD_EARG, "a Float64 vector takes a real coefficient (c_im = 0)");
  if (n != m->N) return sd_set_err(ctx, SD_EDIM, "vector length does not match the basis dimension");
  if (!out || !psi) return sd_set_err(ctx, SD_EARG, "null argument");
  const size_t vbytes = (size_t)n * (dtype == SD_C128 ? 16 : 8);
  if (on_dev && ranges_overlap(out, vbytes, psi, vbytes)) return sd_set_err(ctx, SD_EARG, "out must not alias or overlap psi");
  if (on_dev && y && y != out && ranges_overlap(out, vbytes, y, vbytes)) return sd_set_err(ctx, SD_EARG, "out may be y itself but must not overlap it partly");
  DevIn in, yin;
  DevOut o;
  RC(in.stage(ctx, dtype, psi, on_dev, n));
  if (y) RC(yin.stage(ctx, dtype, y, on_dev, n));
  RC(o.open(ctx, out, on_dev, vec_doubles(dtype, n)));
  RC(sd_launch_symmetry_apply(ctx, m, dtype, code, in.p, yin.p, cr, ci, o.p));
  return o.close(false);                                   // the device form takes nothing from the pool
}

// out (host, 2 n_codes doubles) = <bra|U_g|ket> for the elements of the list
int symmetry_overlaps_core(sd_ctx *ctx, const sd_model *m, int dtype, const void *bra, const void *ket, int64_t n, const int *codes,
                           int n_codes, double *out, bool on_dev) {
  RC(check_unsharded_model(ctx, m));
  if (dtype != SD_F64 && dtype != SD_C128) return sd_set_err(ctx, SD_EARG, "dtype must be SD_F64 or SD_C128");
  if (!ket || !out) return sd_set_err(ctx, SD_EARG, "null argument");
  SymList sl;
  RC(sl.init(ctx, m, codes, nullptr, n_codes));
  if (n != m->N) return sd_set_err(ctx, SD_EDIM, "vector length does not match the basis dimension");
  DevIn bin, kin;
  DBuf res;
  RC(kin.stage(ctx, dtype, ket, on_dev, n));
  if (bra && bra != ket) RC(bin.stage(ctx, dtype, bra, on_dev, n));
  RC(res.alloc(ctx, 2 * (int64_t)n_codes));
  RC(sd_launch_symmetry_overlaps(ctx, m, dtype, bin.p ? bin.p : kin.p, kin.p, sl.codes, n_codes, res.p));
  return read_back(ctx, out, res.p, sizeof(double) * 2 * (size_t)n_codes);
}

// out (n elements of dtype_out) = sum_k c_k U_{g_k} psi
int symmetry_project_core(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi, int64_t n, const int *codes, const double *coef,
                          int n_codes, int dtype_out, void *out, bool on_dev) {
  RC(check_unsharded_model(ctx, m));
  if (dtype != SD_F64 && dtype != SD_C128) return sd_set_err(ctx, SD_EARG, "dtype must be SD_F64 or SD_C128");
  if (dtype_out != SD_F64 && dtype_out != SD_C128) return sd_set_err(ctx, SD_EARG, "dtype_out must be SD_F64 or SD_C128");
  if (!coef || !out || !psi) return sd_set_err(ctx, SD_EARG, "null argument");
  SymList sl;
  RC(sl.init(ctx, m, codes, coef, n_codes));
  if (dtype_out == SD_F64 && dtype != SD_F64) return sd_set_err(ctx, SD_EARG, "an SD_F64 result needs an SD_F64 psi");
  if (dtype_out == SD_F64 && !sl.all_real) return sd_set_err(ctx, SD_EARG, "an SD_F64 result needs real coefficients");
  if (n != m->N) return sd_set_err(ctx, SD_EDIM, "vector length does not match the basis dimension");
  if (on_dev && ranges_overlap(out, (size_t)n * (dtype_out == SD_C128 ? 16 : 8), psi, (size_t)n * (dtype == SD_C128 ? 16 : 8))) return sd_set_err(ctx, SD_EARG, "out must not alias or overlap psi");
  DevIn in;
  DevOut o;
  RC(in.stage(ctx, dtype, psi, on_dev, n));
  RC(o.open(ctx, out, on_dev, vec_doubles(dtype_out, n)));
  RC(sd_launch_symmetry_project(ctx, m, dtype, in.p, sl.codes, sl.coef, n_codes, dtype_out, o.p));
  return o.close(true);                                    // the list goes back to the pool
}

// ---- operator strings (kernels_opstring.hip) ----
// A caller's list validated, cut into groups and put on the device: the three tables in one block from the context's pool (groups,
// terms, op_first).  n_groups == 0: the empty list.
struct OpList {
  TableBlock dev;
  sd_opstring_tables tab;
  int n_groups = 0;
  const sd_opgroup *groups = nullptr;
  const sd_opterm_dev *terms = nullptr;
  const int32_t *op_first = nullptr;
  int init(sd_ctx *ctx, const sd_model *m, const sd_opterm *list, int n_terms) {
    std::string err;
    const int rc = sd_opstring_build(m, list, n_terms, tab, err);
    if (rc) return sd_set_err(ctx, rc, err);
    n_groups = (int)tab.groups.size();
    if (n_groups == 0) return SD_OK;
    const int ig = dev.add(tab.groups.data(), tab.groups.size()), it = dev.add(tab.terms.data(), tab.terms.size()),
              io = dev.add(tab.op_first.data(), tab.op_first.size());
    RC(dev.upload(ctx));
    groups = dev.at<sd_opgroup>(ig);
    terms = dev.at<sd_opterm_dev>(it);
    op_first = dev.at<int32_t>(io);
    return SD_OK;
  }
};

// out (n elements of dtype_out) = O_0 psi (+ (b_re + i b_im) y, y of dtype_out)
int opstring_apply_core(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi, int64_t n, const sd_opterm *list, int n_terms,
                        const void *y, double b_re, double b_im, int dtype_out, void *out, bool on_dev) {
  RC(check_unsharded_model(ctx, m));
  if (dtype != SD_F64 && dtype != SD_C128) return sd_set_err(ctx, SD_EARG, "dtype must be SD_F64 or SD_C128");
  if (dtype_out != SD_F64 && dtype_out != SD_C128) return sd_set_err(ctx, SD_EARG, "dtype_out must be SD_F64 or SD_C128");
  OpList ol;
  RC(ol.init(ctx, m, list, n_terms));
  for (int k = 0; k < n_terms; ++k)
    if (list[k].op != 0) return sd_set_err(ctx, SD_EARG, "the write form takes one operator: every term must have op = 0");
  if (y && (!std::isfinite(b_re) || !std::isfinite(b_im))) return sd_set_err(ctx, SD_EARG, "the coefficient b must be finite");
  if (dtype_out == SD_F64 && dtype != SD_F64) return sd_set_err(ctx, SD_EARG, "an SD_F64 output needs an SD_F64 psi");
  if (dtype_out == SD_F64 && !ol.tab.all_real) return sd_set_err(ctx, SD_EARG, "an SD_F64 output needs real coefficients (every c_im = 0)");
  if (dtype_out == SD_F64 && y && b_im != 0.0) return sd_set_err(ctx, SD_EARG, "an SD_F64 output takes a real b (b_im = 0)");
  if (n != m->N) return sd_set_err(ctx, SD_EDIM, "vector length does not match the basis dimension");
  if (!out || !psi) return sd_set_err(ctx, SD_EARG, "null argument");
  const size_t obytes = (size_t)n * (dtype_out == SD_C128 ? 16 : 8), pbytes = (size_t)n * (dtype == SD_C128 ? 16 : 8);
  if (on_dev && ranges_overlap(out, obytes, psi, pbytes)) return sd_set_err(ctx, SD_EARG, "out must not alias or overlap psi");
  if (on_dev && y && y != out && ranges_overlap(out, obytes, y, obytes)) return sd_set_err(ctx, SD_EARG, "out may be y itself but must not overlap it partly");
  DevIn in, yin;
  DevOut o;
  RC(in.stage(ctx, dtype, psi, on_dev, n));
  if (y) RC(yin.stage(ctx, dtype_out, y, on_dev, n));
  RC(o.open(ctx, out, on_dev, vec_doubles(dtype_out, n)));
  RC(sd_launch_opstring(ctx, m, dtype, in.p, ol.groups, ol.n_groups, ol.terms, yin.p, b_re, b_im, dtype_out, o.p));
  return o.close(ol.n_groups > 0);                         // the tables go back to the pool; the empty list has none
}

// out (host, 2 K doubles, K = 1 + max op) = <bra|O_k|ket>
int opstring_expect_core(sd_ctx *ctx, const sd_model *m, int dtype, const void *bra, const void *ket, int64_t n, const sd_opterm *list,
                         int n_terms, double *out, bool on_dev) {
  RC(check_unsharded_model(ctx, m));
  if (dtype != SD_F64 && dtype != SD_C128) return sd_set_err(ctx, SD_EARG, "dtype must be SD_F64 or SD_C128");
  OpList ol;
  RC(ol.init(ctx, m, list, n_terms));
  if (n != m->N) return sd_set_err(ctx, SD_EDIM, "vector length does not match the basis dimension");
  if (!ket) return sd_set_err(ctx, SD_EARG, "null argument");
  const int K = ol.tab.n_ops;
  if (K == 0) return SD_OK;                                  // the empty list: no operator, nothing to write
  if (!out) return sd_set_err(ctx, SD_EARG, "null argument");
  DevIn bin, kin;
  DBuf res;
  RC(kin.stage(ctx, dtype, ket, on_dev, n));
  if (bra && bra != ket) RC(bin.stage(ctx, dtype, bra, on_dev, n));
  RC(res.alloc(ctx, 2 * (int64_t)K));
  RC(sd_launch_opstring_expect(ctx, m, dtype, bin.p ? bin.p : kin.p, kin.p, ol.groups, ol.op_first, ol.terms, K, res.p));
  return read_back(ctx, out, res.p, sizeof(double) * 2 * (size_t)K);
}

}  // namespace

extern "C" int sd_current_apply(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi_host, int64_t n, const double *w,
                                void *out_host) {
  return abi_guard(ctx, [&]() -> int { return current_core(ctx, m, dtype, psi_host, nullptr, false, n, w, out_host, false); });
}
extern "C" int sd_current_apply_dev(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi_dev, int64_t n, const double *w,
                                    void *out_dev) {
  return abi_guard(ctx, [&]() -> int { return current_core(ctx, m, dtype, psi_dev, nullptr, false, n, w, out_dev, true); });
}
extern "C" int sd_current_bracket(sd_ctx *ctx, const sd_model *m, int dtype_bra, const void *bra_host, const void *ket_host, int64_t n,
                                  const double *w, double *out) {
  return abi_guard(ctx, [&]() -> int {
    if (!bra_host) return sd_set_err(ctx, SD_EARG, "null argument");
    return current_core(ctx, m, dtype_bra, ket_host, bra_host, true, n, w, out, false);
  });
}
extern "C" int sd_current_bracket_dev(sd_ctx *ctx, const sd_model *m, int dtype_bra, const void *bra_dev, const void *ket_dev, int64_t n,
                                      const double *w, double *out) {
  return abi_guard(ctx, [&]() -> int {
    if (!bra_dev) return sd_set_err(ctx, SD_EARG, "null argument");
    return current_core(ctx, m, dtype_bra, ket_dev, bra_dev, true, n, w, out, true);
  });
}

extern "C" int sd_energy_current_terms(const sd_model *m, int periodic, sd_dterm *out, int cap, int *n_terms) {
  return abi_guard(nullptr, [&]() -> int {
    if (!m || !n_terms || cap < 0 || (cap > 0 && !out) || (periodic != 0 && periodic != 1)) return SD_EARG;
    std::vector<sd_dterm> list;
    std::string err;
    const int rc = sd_build_energy_current(m, periodic, list, err);
    if (rc) return m->ctx ? sd_set_err(m->ctx, rc, err) : rc;
    *n_terms = (int)list.size();
    if (cap == 0) return SD_OK;
    if ((size_t)cap < list.size()) return m->ctx ? sd_set_err(m->ctx, SD_EARG, "cap is smaller than the number of terms") : SD_EARG;
    std::copy(list.begin(), list.end(), out);
    return SD_OK;
  });
}
extern "C" int sd_dcurrent_apply(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi_host, int64_t n, const sd_dterm *terms,
                                 int n_terms, void *out_host) {
  return abi_guard(ctx, [&]() -> int { return dcurrent_core(ctx, m, dtype, psi_host, nullptr, false, n, terms, n_terms, out_host, false); });
}
extern "C" int sd_dcurrent_apply_dev(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi_dev, int64_t n, const sd_dterm *terms,
                                     int n_terms, void *out_dev) {
  return abi_guard(ctx, [&]() -> int { return dcurrent_core(ctx, m, dtype, psi_dev, nullptr, false, n, terms, n_terms, out_dev, true); });
}
extern "C" int sd_dcurrent_bracket(sd_ctx *ctx, const sd_model *m, int dtype_bra, const void *bra_host, const void *ket_host, int64_t n,
                                   const sd_dterm *terms, int n_terms, double *out) {
  return abi_guard(ctx, [&]() -> int {
    if (!bra_host) return sd_set_err(ctx, SD_EARG, "null argument");
    return dcurrent_core(ctx, m, dtype_bra, ket_host, bra_host, true, n, terms, n_terms, out, false);
  });
}
extern "C" int sd_dcurrent_bracket_dev(sd_ctx *ctx, const sd_model *m, int dtype_bra, const void *bra_dev, const void *ket_dev, int64_t n,
                                       const sd_dterm *terms, int n_terms, double *out) {
  return abi_guard(ctx, [&]() -> int {
    if (!bra_dev) return sd_set_err(ctx, SD_EARG, "null argument");
    return dcurrent_core(ctx, m, dtype_bra, ket_dev, bra_dev, true, n, terms, n_terms, out, true);
  });
}

extern "C" int sd_pair_correlations(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi_host, int64_t n, int component,
                                    double *M_out) {
  return abi_guard(ctx, [&]() -> int { return pair_correlations_core(ctx, m, dtype, psi_host, n, component, M_out, false); });
}
extern "C" int sd_pair_correlations_dev(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi_dev, int64_t n, int component,
                                        double *M_out) {
  return abi_guard(ctx, [&]() -> int { return pair_correlations_core(ctx, m, dtype, psi_dev, n, component, M_out, true); });
}

extern "C" int sd_basis_moments(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi_host, int64_t n, const double *q, int nq,
                                double *out) {
  return abi_guard(ctx, [&]() -> int { return basis_moments_core(ctx, m, dtype, psi_host, n, q, nq, out, false); });
}
extern "C" int sd_basis_moments_dev(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi_dev, int64_t n, const double *q, int nq,
                                    double *out) {
  return abi_guard(ctx, [&]() -> int { return basis_moments_core(ctx, m, dtype, psi_dev, n, q, nq, out, true); });
}
extern "C" int sd_counting_range(const sd_model *m, uint64_t mask, int *m_min, int *n_bins) {
  if (!m || !m_min || !n_bins) return SD_EARG;
  return sd_counting_range_host(m, mask, m_min, n_bins);
}
extern "C" int sd_counting_statistics(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi_host, int64_t n, const uint64_t *masks,
                                      int K, double *P_out) {
  return abi_guard(ctx, [&]() -> int { return counting_statistics_core(ctx, m, dtype, psi_host, n, masks, K, P_out, false); });
}
extern "C" int sd_counting_statistics_dev(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi_dev, int64_t n,
                                          const uint64_t *masks, int K, double *P_out) {
  return abi_guard(ctx, [&]() -> int { return counting_statistics_core(ctx, m, dtype, psi_dev, n, masks, K, P_out, true); });
}
extern "C" int sd_sample_uniforms_host(uint64_t seed, uint64_t first, int64_t n, double *u_out) {
  if (!u_out || n < 0) return SD_EARG;
  for (int64_t i = 0; i < n; ++i) u_out[i] = sd_sample_uniform_host(seed, first + (uint64_t)i);
  return SD_OK;
}
extern "C" int sd_sample_configurations(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi_host, int64_t n, int64_t shots,
                                        uint64_t seed, int64_t *rows_out, uint64_t *configs_out) {
  return abi_guard(ctx, [&]() -> int {
    return sample_configurations_core(ctx, m, dtype, psi_host, n, shots, seed, rows_out, configs_out, false);
  });
}
extern "C" int sd_sample_configurations_dev(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi_dev, int64_t n, int64_t shots,
                                            uint64_t seed, int64_t *rows_out, uint64_t *configs_out) {
  return abi_guard(ctx, [&]() -> int {
    return sample_configurations_core(ctx, m, dtype, psi_dev, n, shots, seed, rows_out, configs_out, true);
  });
}

extern "C" int sd_bond_apply(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi_host, int64_t n, int i, int j, double xy,
                             double zz, void *out_host) {
  return abi_guard(ctx, [&]() -> int { return bond_apply_core(ctx, m, dtype, psi_host, n, i, j, xy, zz, out_host, false); });
}
extern "C" int sd_bond_apply_dev(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi_dev, int64_t n, int i, int j, double xy,
                                 double zz, void *out_dev) {
  return abi_guard(ctx, [&]() -> int { return bond_apply_core(ctx, m, dtype, psi_dev, n, i, j, xy, zz, out_dev, true); });
}
extern "C" int sd_dimer_correlations(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi_host, int64_t n, const int *bonds,
                                     int B, double xy, double zz, double *D_out, double *e_out) {
  return abi_guard(ctx, [&]() -> int { return dimer_correlations_core(ctx, m, dtype, psi_host, n, bonds, B, xy, zz, D_out, e_out, false); });
}
extern "C" int sd_dimer_correlations_dev(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi_dev, int64_t n, const int *bonds,
                                         int B, double xy, double zz, double *D_out, double *e_out) {
  return abi_guard(ctx, [&]() -> int { return dimer_correlations_core(ctx, m, dtype, psi_dev, n, bonds, B, xy, zz, D_out, e_out, true); });
}

extern "C" int sd_symmetry_apply(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi_host, int64_t n, int code, const void *y_host,
                                 double c_re, double c_im, void *out_host) {
  return abi_guard(ctx, [&]() -> int { return symmetry_apply_core(ctx, m, dtype, psi_host, n, code, y_host, c_re, c_im, out_host, false); });
}
extern "C" int sd_symmetry_apply_dev(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi_dev, int64_t n, int code,
                                     const void *y_dev, double c_re, double c_im, void *out_dev) {
  return abi_guard(ctx, [&]() -> int { return symmetry_apply_core(ctx, m, dtype, psi_dev, n, code, y_dev, c_re, c_im, out_dev, true); });
}
extern "C" int sd_symmetry_overlaps(sd_ctx *ctx, const sd_model *m, int dtype, const void *bra_host, const void *ket_host, int64_t n,
                                    const int *codes, int n_codes, double *out) {
  return abi_guard(ctx, [&]() -> int { return symmetry_overlaps_core(ctx, m, dtype, bra_host, ket_host, n, codes, n_codes, out, false); });
}
extern "C" int sd_symmetry_overlaps_dev(sd_ctx *ctx, const sd_model *m, int dtype, const void *bra_dev, const void *ket_dev, int64_t n,
                                        const int *codes, int n_codes, double *out) {
  return abi_guard(ctx, [&]() -> int { return symmetry_overlaps_core(ctx, m, dtype, bra_dev, ket_dev, n, codes, n_codes, out, true); });
}
extern "C" int sd_symmetry_project(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi_host, int64_t n, const int *codes,
                                   const double *coef, int n_codes, int dtype_out, void *out_host) {
  return abi_guard(ctx, [&]() -> int { return symmetry_project_core(ctx, m, dtype, psi_host, n, codes, coef, n_codes, dtype_out, out_host, false); });
}
extern "C" int sd_symmetry_project_dev(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi_dev, int64_t n, const int *codes,
                                       const double *coef, int n_codes, int dtype_out, void *out_dev) {
  return abi_guard(ctx, [&]() -> int { return symmetry_project_core(ctx, m, dtype, psi_dev, n, codes, coef, n_codes, dtype_out, out_dev, true); });
}

extern "C" int sd_opstring_check(const sd_model *m, const sd_opterm *terms, int n_terms, int *n_ops, int *hermitian) {
  return abi_guard(nullptr, [&]() -> int {
    if (!m || !n_ops || !hermitian) return SD_EARG;
    sd_opstring_tables tab;
    std::string err;
    const int rc = sd_opstring_build(m, terms, n_terms, tab, err);
    if (rc) return m->ctx ? sd_set_err(m->ctx, rc, err) : rc;
    *n_ops = tab.n_ops;
    *hermitian = sd_opstring_hermitian(terms, n_terms) ? 1 : 0;
    return SD_OK;
  });
}
extern "C" int sd_hamiltonian_terms(const sd_model *m, sd_opterm *out, int cap, int *n_terms) {
  return abi_guard(nullptr, [&]() -> int {
    if (!m || !n_terms || cap < 0 || (cap > 0 && !out)) return SD_EARG;
    auto fail = [&](const char *msg) { return m->ctx ? sd_set_err(m->ctx, SD_EARG, msg) : SD_EARG; };
    if (m->L < 1 || m->L > SD_MAX_L) return fail("operator strings need 1 <= L <= 63");
    auto bit = [](int site) { return (uint64_t)1 << (site - 1); };
    std::vector<sd_opterm> list;
    for (size_t b = 0; b < m->hop_J.size(); ++b) {           // t (S^+_i S^-_j + S^-_i S^+_j); i == j never flips
      const int i = m->hop_i[b], j = m->hop_j[b];
      if (i == j) continue;
      list.push_back(sd_opterm{bit(i), bit(j), 0, m->hop_J[b], 0.0, 0, 0});
      list.push_back(sd_opterm{bit(j), bit(i), 0, m->hop_J[b], 0.0, 0, 0});
    }
    for (size_t b = 0; b < m->zz_J.size(); ++b) {            // v S^z_i S^z_j; i == j: (S^z_i)^2 = 1/4
      const int i = m->zz_i[b], j = m->zz_j[b];
      if (i == j) list.push_back(sd_opterm{0, 0, 0, 0.25 * m->zz_J[b], 0.0, 0, 0});
      else list.push_back(sd_opterm{0, 0, bit(i) | bit(j), m->zz_J[b], 0.0, 0, 0});
    }
    for (int i = 1; i <= m->L && i <= (int)m->field.size(); ++i) list.push_back(sd_opterm{0, 0, bit(i), m->field[(size_t)i - 1], 0.0, 0, 0});
    if (list.size() > SD_OPTERM_MAX) return fail("the model's lists give more than SD_OPTERM_MAX terms");
    *n_terms = (int)list.size();
    if (cap == 0) return SD_OK;
    if ((size_t)cap < list.size()) return fail("cap is smaller than the number of terms");
    std::copy(list.begin(), list.end(), out);
    return SD_OK;
  });
}
extern "C" int sd_opstring_apply(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi_host, int64_t n, const sd_opterm *terms,
                                 int n_terms, const void *y_host, double b_re, double b_im, int dtype_out, void *out_host) {
  return abi_guard(ctx, [&]() -> int { return opstring_apply_core(ctx, m, dtype, psi_host, n, terms, n_terms, y_host, b_re, b_im, dtype_out, out_host, false); });
}
extern "C" int sd_opstring_apply_dev(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi_dev, int64_t n, const sd_opterm *terms,
                                     int n_terms, const void *y_dev, double b_re, double b_im, int dtype_out, void *out_dev) {
  return abi_guard(ctx, [&]() -> int { return opstring_apply_core(ctx, m, dtype, psi_dev, n, terms, n_terms, y_dev, b_re, b_im, dtype_out, out_dev, true); });
}
extern "C" int sd_opstring_expect(sd_ctx *ctx, const sd_model *m, int dtype, const void *bra_host, const void *ket_host, int64_t n,
                                  const sd_opterm *terms, int n_terms, double *out) {
  return abi_guard(ctx, [&]() -> int { return opstring_expect_core(ctx, m, dtype, bra_host, ket_host, n, terms, n_terms, out, false); });
}
extern "C" int sd_opstring_expect_dev(sd_ctx *ctx, const sd_model *m, int dtype, const void *bra_dev, const void *ket_dev, int64_t n,
                                      const sd_opterm *terms, int n_terms, double *out) {
  return abi_guard(ctx, [&]() -> int { return opstring_expect_core(ctx, m, dtype, bra_dev, ket_dev, n, terms, n_terms, out, true); });
}
