// C ABI: contexts, models, operator-level entry points (include/spindyn.h).
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <new>
#include <string>
#include <utility>
#include <vector>

#include "host_calls.hpp"
#include "site_perm.hpp"

int sd_set_err(sd_ctx *ctx, int code, const std::string &msg) {
  if (ctx) ctx->err = msg;
  return code;
}

int sd_pool_take(sd_ctx *ctx, size_t bytes, void **out, size_t *got) {
  if (bytes == 0) bytes = 8;
  int best = -1;
  for (int i = 0; i < (int)ctx->pool_free.size(); ++i) {
    const size_t sz = ctx->pool_free[i].second;
    if (sz >= bytes && sz <= 2 * bytes && (best < 0 || sz < ctx->pool_free[best].second)) best = i;
  }
  if (best >= 0) {
    *out = ctx->pool_free[best].first; *got = ctx->pool_free[best].second;
    ctx->pool_free.erase(ctx->pool_free.begin() + best);
    return SD_OK;
  }
  static const bool dbg = getenv("SD_POOL_DEBUG") != nullptr;     // stderr trace of every allocation the pool could not serve
  const auto t0 = std::chrono::steady_clock::now();
  hipError_t e = hipMalloc(out, bytes);
  bool retried = false;
  if (e != hipSuccess) {                       // make room: drop what the pool still holds, then try once more
    (void)hipGetLastError();
    sd_pool_release(ctx);
    e = hipMalloc(out, bytes);
    retried = true;
  }
  if (dbg) {
    size_t held = 0, fr = 0, tot = 0;
    for (auto &b : ctx->pool_free) held += b.second;
    (void)hipMemGetInfo(&fr, &tot);
    fprintf(stderr, "[sd pool] hipMalloc %.3f GB took %.1f ms%s; pool holds %zu blocks / %.2f GB; device free %.1f of %.1f GB\n",
            bytes / 1e9, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(),
            retried ? " (after dropping the pool: first attempt failed)" : "", ctx->pool_free.size(), held / 1e9, fr / 1e9, tot / 1e9);
  }
  if (e != hipSuccess) { *out = nullptr; return sd_set_err(ctx, SD_ENOMEM, std::string("hipMalloc: ") + hipGetErrorString(e)); }
  *got = bytes;
  return SD_OK;
}

void sd_pool_give(sd_ctx *ctx, void *p, size_t bytes) {
  if (!p) return;
  static const size_t cap = [] {               // bytes the pool may hold (SD_POOL_MAX_GB, default 96; 0 disables the pool)
    const char *e = getenv("SD_POOL_MAX_GB");
    return (size_t)((e ? atof(e) : 96.0) * 1e9);
  }();
  if (bytes > cap) { (void)hipFree(p); return; }
  // every block is kept (a hipMalloc/hipFree pair costs ~0.1 ms even for a few KB: hipFree waits for the device -- more than
  // three Lanczos steps of a small system); the oldest blocks make room when the pool is full
  ctx->pool_free.emplace_back(p, bytes);
  size_t held = 0;
  for (auto &b : ctx->pool_free) held += b.second;
  while (!ctx->pool_free.empty() && (held > cap || ctx->pool_free.size() > 256)) {
    held -= ctx->pool_free.front().second;
    (void)hipFree(ctx->pool_free.front().first);
    ctx->pool_free.erase(ctx->pool_free.begin());
  }
}

void sd_pool_release(sd_ctx *ctx) {
  for (auto &b : ctx->pool_free) (void)hipFree(b.first);
  ctx->pool_free.clear();
}

int sd_ensure_partials(sd_ctx *ctx, size_t doubles) {
  if (ctx->partials_cap >= doubles) return SD_OK;
  if (ctx->d_partials) (void)hipFree(ctx->d_partials);   // hipFree waits for the kernels still using it
  ctx->d_partials = nullptr; ctx->partials_cap = 0;
  SD_HIP(ctx, hipMalloc((void **)&ctx->d_partials, doubles * sizeof(double)));
  ctx->partials_cap = doubles;
  return SD_OK;
}

namespace {
thread_local std::string g_err;  // errors raised without a context

int fail(sd_ctx *ctx, int code, const std::string &msg) {
  g_err = msg;
  return sd_set_err(ctx, code, msg);
}

struct TmpDev {
  sd_ctx *ctx;
  void *p = nullptr;
  explicit TmpDev(sd_ctx *c) : ctx(c) {}
  ~TmpDev() { if (p) (void)hipFree(p); }
  int alloc(size_t bytes) {
    hipError_t e = hipMalloc(&p, bytes ? bytes : 1);
    if (e != hipSuccess) return sd_set_err(ctx, SD_ENOMEM, std::string("hipMalloc: ") + hipGetErrorString(e));
    return SD_OK;
  }
};

// grow-only device staging buffers of a context: a solver that calls sd_apply in a loop pays hipMalloc/hipFree once
int stage_buf(sd_ctx *ctx, int which, size_t bytes, void **out) {
  if (ctx->stage_cap[which] < bytes) {
    if (ctx->stage[which]) (void)hipFree(ctx->stage[which]);
    ctx->stage[which] = nullptr; ctx->stage_cap[which] = 0;
    hipError_t e = hipMalloc(&ctx->stage[which], bytes ? bytes : 1);
    if (e != hipSuccess) return sd_set_err(ctx, SD_ENOMEM, std::string("hipMalloc: ") + hipGetErrorString(e));
    ctx->stage_cap[which] = bytes;
  }
  *out = ctx->stage[which];
  return SD_OK;
}

int check_apply_args(sd_ctx *ctx, const sd_model *m, int dtype, const void *out, const void *psi, int64_t n) {
  if (!ctx) return SD_EARG;
  if (!m) return sd_set_err(ctx, SD_EARG, "null model");
  if (!m->dev_ready) return sd_set_err(ctx, SD_EARG, "model has no device tables (created without a context)");
  if (dtype != SD_F64 && dtype != SD_C128) return sd_set_err(ctx, SD_EARG, "dtype must be SD_F64 or SD_C128");
  if (!out || !psi) return sd_set_err(ctx, SD_EARG, "null vector");
  if (out == psi) return sd_set_err(ctx, SD_EARG, "out must not alias psi");
  SD_HIP(ctx, hipSetDevice(ctx->device));   // the caller's thread may have another device current (several contexts per process)
  return SD_OK;
}
// the site pairs of a bond list as a table: J summed per unordered pair in list order, i == j and exact zeros dropped, each pair
// sent through the site permutation `perm` (1-based)
std::map<std::pair<int, int>, double> bond_table(const std::vector<int> &bi, const std::vector<int> &bj, const std::vector<double> &J,
                                                 const std::vector<int> &perm) {
  std::map<std::pair<int, int>, double> sum, out;
  for (size_t k = 0; k < J.size(); ++k) {
    if (bi[k] == bj[k]) continue;
    sum[{std::min(bi[k], bj[k]), std::max(bi[k], bj[k])}] += J[k];
  }
  for (const auto &e : sum) {
    if (e.second == 0.0) continue;
    const int a = perm[(size_t)e.first.first], b = perm[(size_t)e.first.second];
    out[{std::min(a, b), std::max(a, b)}] = e.second;
  }
  return out;
}
}  // namespace

int sd_symmetry_check_code(const sd_model *m, int code, std::string &err) {
  const int r = code & 255;
  if (code < 0 || (code >> 10) != 0 || r >= m->L) { err = "element code: the shift must be in 0..L-1 and no bit above bit 9 set"; return SD_EARG; }
  if ((code & SD_SYM_FLIP) && m->nup >= 0 && 2 * m->nup != m->L) {
    err = "the spin flip Z is defined on the full basis and on sectors with 2 nup = L only";
    return SD_EARG;
  }
  return SD_OK;
}

// ---- operator strings: a caller's list against a model, cut into the device tables ----
int sd_opstring_build(const sd_model *m, const sd_opterm *list, int n_terms, sd_opstring_tables &out, std::string &err) {
  if (n_terms < 0 || n_terms > SD_OPTERM_MAX) { err = "the number of terms must be in 0..SD_OPTERM_MAX"; return SD_EARG; }
  if (n_terms > 0 && !list) { err = "null argument"; return SD_EARG; }
  if (m->L < 1 || m->L > SD_MAX_L) { err = "operator strings need 1 <= L <= 63"; return SD_EARG; }
  const uint64_t outside = ~(~(uint64_t)0 >> (64 - m->L));
  out = sd_opstring_tables();
  out.terms.resize((size_t)n_terms);
  std::vector<sd_opgroup> g;
  int max_op = -1;
  for (int n = 0; n < n_terms; ++n) {
    const sd_opterm &T = list[n];
    if ((T.plus & T.minus) || (T.plus & T.z) || (T.minus & T.z)) { err = "the plus, minus and z masks of a term must be pairwise disjoint"; return SD_EARG; }
    if ((T.plus | T.minus | T.z) & outside) { err = "a mask of a term has a bit at or above L"; return SD_EARG; }
    if (m->nup >= 0 && __builtin_popcountll(T.plus) != __builtin_popcountll(T.minus)) {
      err = "in a fixed-nup sector every term needs as many S^+ as S^- factors";
      return SD_EARG;
    }
    if (!std::isfinite(T.c_re) || !std::isfinite(T.c_im)) { err = "the coefficients must be finite"; return SD_EARG; }
    if (T.op < 0 || T.op >= SD_OPSTRING_MAX_OPS) { err = "op must be in 0..SD_OPSTRING_MAX_OPS-1"; return SD_EARG; }
    if (T.c_im != 0.0) out.all_real = false;
    max_op = std::max(max_op, (int)T.op);
    if (n == 0 || T.plus != list[n - 1].plus || T.minus != list[n - 1].minus || T.op != list[n - 1].op)
      g.push_back(sd_opgroup{T.plus, T.minus, n, 0, T.op, 0});
    ++g.back().count;
    const double sc = std::ldexp(1.0, -__builtin_popcountll(T.z));      // 2^-|Z|: exact
    out.terms[(size_t)n] = sd_opterm_dev{T.z, T.c_re * sc, T.c_im * sc};
  }
  out.n_ops = max_op + 1;
  std::stable_sort(g.begin(), g.end(), [](const sd_opgroup &a, const sd_opgroup &b) { return a.op < b.op; });
  out.op_first.assign((size_t)out.n_ops + 1, 0);
  for (const sd_opgroup &G : g) ++out.op_first[(size_t)G.op + 1];
  for (int k = 0; k < out.n_ops; ++k) out.op_first[(size_t)k + 1] += out.op_first[(size_t)k];
  out.groups = std::move(g);
  return SD_OK;
}

bool sd_opstring_hermitian(const sd_opterm *list, int n_terms) {
  struct Key {
    int32_t op; uint64_t p, m, z;
    bool operator<(const Key &o) const { return op != o.op ? op < o.op : p != o.p ? p < o.p : m != o.m ? m < o.m : z < o.z; }
  };
  std::map<Key, std::pair<double, double>> sum;
  for (int n = 0; n < n_terms; ++n) {
    auto &s = sum[Key{list[n].op, list[n].plus, list[n].minus, list[n].z}];
    s.first += list[n].c_re; s.second += list[n].c_im;
  }
  for (const auto &e : sum) {
    const double re = e.second.first, im = e.second.second;
    const auto it = sum.find(Key{e.first.op, e.first.m, e.first.p, e.first.z});      // the adjoint term: P <-> M, conj(c)
    const double are = it == sum.end() ? 0.0 : it->second.first, aim = it == sum.end() ? 0.0 : it->second.second;
    if (re != are || im != -aim) return false;
  }
  return true;
}

extern "C" {

int sd_model_symmetric(const sd_model *m, int code, int *yes) {
  if (!m || !yes) return SD_EARG;
  try {
    std::string err;
    const int rc = sd_symmetry_check_code(m, code, err);
    if (rc) return m->ctx ? sd_set_err(m->ctx, rc, err) : rc;
    const int L = m->L, r = code & 255;
    std::vector<int> id((size_t)L + 1), perm((size_t)L + 1);       // site i -> the site T^r R^refl moves its spin to
    for (int i = 1; i <= L; ++i) {
      id[(size_t)i] = i;
      const int j = (code & SD_SYM_REFLECT) ? L + 1 - i : i;
      perm[(size_t)i] = (j - 1 + r) % L + 1;
    }
    bool ok = bond_table(m->hop_i, m->hop_j, m->hop_J, perm) == bond_table(m->hop_i, m->hop_j, m->hop_J, id) &&
              bond_table(m->zz_i, m->zz_j, m->zz_J, perm) == bond_table(m->zz_i, m->zz_j, m->zz_J, id);
    for (int i = 1; i <= L && ok; ++i) {
      const double f = m->field[(size_t)i - 1];
      ok = f == m->field[(size_t)perm[(size_t)i] - 1] && !((code & SD_SYM_FLIP) && f != 0.0);
    }
    *yes = ok ? 1 : 0;
    return SD_OK;
  } catch (...) {
    return m->ctx ? sd_set_err(m->ctx, SD_ENOMEM, "out of host memory inside the call") : SD_ENOMEM;
  }
}

const char *sd_version(void) { return "spindyn-mi355x 0.1 (gfx950)"; }

int sd_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

const char *sd_status_string(int status) {
  switch (status) {
    case SD_OK: return "ok";
    case SD_EARG: return "invalid argument";
    case SD_EDIM: return "dimension mismatch";
    case SD_EZERO: return "starting vector has zero norm";
    case SD_ENOMEM: return "out of memory";
    case SD_EHIP: return "HIP error";
    case SD_ENODEV: return "no HIP device";
    case SD_EINTERNAL: return "internal error";
    case SD_ECOMM: return "communication error";
    default: return "unknown status";
  }
}

int sd_ctx_create(int device, sd_ctx **out) {
  if (!out) return SD_EARG;
  *out = nullptr;
  int n = sd_device_count();
  if (n <= 0) return fail(nullptr, SD_ENODEV, "no HIP device: libspindyn has no CPU fallback");
  if (device < 0 || device >= n) return fail(nullptr, SD_EARG, "device index out of range");
  sd_ctx *c = new (std::nothrow) sd_ctx();
  if (!c) return SD_ENOMEM;
  c->device = device;
  if (hipSetDevice(device) != hipSuccess || hipStreamCreate(&c->own_stream) != hipSuccess) {
    delete c;
    return fail(nullptr, SD_EHIP, "hipSetDevice/hipStreamCreate failed");
  }
  c->stream = c->own_stream;
  if (hipMalloc((void **)&c->d_scalars, 16 * sizeof(double)) != hipSuccess ||
      hipHostMalloc((void **)&c->h_scalars, 16 * sizeof(double)) != hipSuccess ||
      hipEventCreate(&c->ev0) != hipSuccess || hipEventCreate(&c->ev1) != hipSuccess) {
    sd_ctx_destroy(c);
    return fail(nullptr, SD_EHIP, "context allocation failed");
  }
  (void)hipMemset(c->d_scalars, 0, 16 * sizeof(double));
  if (const char *e = getenv("SD_Q_BATCH")) c->q_batch = atoi(e) ? 1 : 0;
  *out = c;
  return SD_OK;
}

void sd_ctx_destroy(sd_ctx *c) {
  if (!c) return;
  if (c->own_stream) (void)hipStreamSynchronize(c->own_stream);
  if (c->d_partials) (void)hipFree(c->d_partials);
  for (void *b : c->stage) if (b) (void)hipFree(b);
  sd_xfer_release(c);
  sd_pool_release(c);
  if (c->d_scalars) (void)hipFree(c->d_scalars);
  if (c->h_scalars) (void)hipHostFree(c->h_scalars);
  if (c->ev0) (void)hipEventDestroy(c->ev0);
  if (c->ev1) (void)hipEventDestroy(c->ev1);
  if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
  delete c;
}

int sd_ctx_set_stream(sd_ctx *ctx, void *hip_stream) {
  if (!ctx) return SD_EARG;
  ctx->stream = hip_stream ? (hipStream_t)hip_stream : ctx->own_stream;
  SD_HIP(ctx, hipSetDevice(ctx->device));
  return SD_OK;
}

int sd_ctx_set_kpm_doubling(sd_ctx *ctx, int on) {
  if (!ctx) return SD_EARG;
  ctx->kpm_doubling = on ? 1 : 0;
  return SD_OK;
}

int64_t sd_ctx_apply_count(const sd_ctx *ctx) { return ctx ? ctx->n_applies : -1; }

int sd_ctx_set_gs_blocked(sd_ctx *ctx, int on) {
  if (!ctx) return SD_EARG;
  ctx->gs_blocked = on ? 1 : 0;
  return SD_OK;
}

int sd_ctx_set_kpm_pair_q(sd_ctx *ctx, int on) {
  if (!ctx) return SD_EARG;
  ctx->kpm_pair_q = on ? 1 : 0;
  return SD_OK;
}

int sd_ctx_set_q_batch(sd_ctx *ctx, int on) {
  if (!ctx) return SD_EARG;
  ctx->q_batch = on ? 1 : 0;
  return SD_OK;
}

int sd_ctx_release_scratch(sd_ctx *ctx) {
  if (!ctx) return SD_EARG;
  SD_HIP(ctx, hipStreamSynchronize(ctx->stream));
  for (int k = 0; k < 2; ++k) {
    if (ctx->stage[k]) (void)hipFree(ctx->stage[k]);
    ctx->stage[k] = nullptr; ctx->stage_cap[k] = 0;
  }
  if (ctx->d_partials) (void)hipFree(ctx->d_partials);
  ctx->d_partials = nullptr; ctx->partials_cap = 0;
  sd_xfer_release(ctx);
  sd_pool_release(ctx);
  return SD_OK;
}

int sd_ctx_synchronize(sd_ctx *ctx) {
  if (!ctx) return SD_EARG;
  SD_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return SD_OK;
}

const char *sd_last_error(const sd_ctx *ctx) { return ctx ? ctx->err.c_str() : g_err.c_str(); }

// Plan + device tables of a model.  The plan's host tables grow with the number of tiles (up to 2^26 prefixes x p entries): a
// failed host allocation must come back as a status, never unwind through the C ABI.
static int plan_and_upload(sd_model *m, int rank, int nranks, std::string &err) {
  try {
    int rc = sd_build_plan(m, rank, nranks, err);
    if (!rc && m->ctx) {
      if (hipSetDevice(m->ctx->device) != hipSuccess) { rc = SD_EHIP; err = "hipSetDevice failed"; }
      else rc = sd_upload_model(m, err);
    }
    return rc;
  } catch (const std::bad_alloc &) {
    err = "out of host memory while building the plan tables of this model";
    return SD_ENOMEM;
  } catch (const std::exception &e) {
    err = std::string("plan construction failed: ") + e.what();
    return SD_EINTERNAL;
  }
}

int sd_model_create(sd_ctx *ctx, int L, int nup, int n_hop, const int *hop_i, const int *hop_j, const double *hop_J,
                    int n_zz, const int *zz_i, const int *zz_j, const double *zz_J, const double *field,
                    sd_model **out) {
  if (!out) return SD_EARG;
  *out = nullptr;
  // src/Basis.jl:9-20 _validate_basis_args
  if (L < 1) return fail(ctx, SD_EARG, "L must be at least 1");
  if (L > SD_MAX_L) return fail(ctx, SD_EARG, "L must be at most 63 when using UInt64 basis states");
  if (nup < -1 || nup > L) return fail(ctx, SD_EARG, "nup must satisfy 0 <= nup <= L");
  if (n_hop < 0 || n_zz < 0 || n_hop > SD_MAX_BONDS || n_zz > SD_MAX_BONDS) return fail(ctx, SD_EARG, "bad bond count");
  if ((n_hop && (!hop_i || !hop_j || !hop_J)) || (n_zz && (!zz_i || !zz_j || !zz_J))) return fail(ctx, SD_EARG, "null bond list");
  for (int k = 0; k < n_hop; ++k)
    if (hop_i[k] < 1 || hop_i[k] > L || hop_j[k] < 1 || hop_j[k] > L)
      return fail(ctx, SD_EARG, "hopping bond site out of range");
  for (int k = 0; k < n_zz; ++k)
    if (zz_i[k] < 1 || zz_i[k] > L || zz_j[k] < 1 || zz_j[k] > L) return fail(ctx, SD_EARG, "zz bond site out of range");
  sd_model *m = new (std::nothrow) sd_model();
  if (!m) return SD_ENOMEM;
  m->ctx = ctx; m->L = L; m->nup = nup;
  // a hop (i, i, J) is accepted as the reference accepts it (build_model takes any pair; in apply_H! bit_i != bit_j is
  // never true for i == j, src/Hamiltonian.jl:248-252): the term does nothing and is dropped here, the order of the rest kept
  for (int k = 0; k < n_hop; ++k) {
    if (hop_i[k] == hop_j[k]) continue;
    m->hop_i.push_back(hop_i[k]); m->hop_j.push_back(hop_j[k]); m->hop_J.push_back(hop_J[k]);
  }
  m->zz_i.assign(zz_i, zz_i + n_zz); m->zz_j.assign(zz_j, zz_j + n_zz); m->zz_J.assign(zz_J, zz_J + n_zz);
  m->field.assign(L, 0.0);
  if (field) m->field.assign(field, field + L);
  sd_fill_binom(m->binom);
  m->N = nup < 0 ? ((int64_t)1 << L) : sd_binom(L, nup);
  std::string err;
  int rc = plan_and_upload(m, 0, 1, err);
  if (rc) { sd_model_destroy(m); return fail(ctx, rc, err); }
  *out = m;
  return SD_OK;
}

int sd_xxz_chain(sd_ctx *ctx, int L, double Jxy, double Jz, double hz, int nup, int boundary, sd_model **out) {
  if (!out) return SD_EARG;
  *out = nullptr;
  if (boundary != 0 && boundary != 1) return fail(ctx, SD_EARG, "boundary must be :open or :periodic");
  if (L < 1 || L > SD_MAX_L) return fail(ctx, SD_EARG, "L must satisfy 1 <= L <= 63");
  int hi[SD_MAX_L + 1], hj[SD_MAX_L + 1];
  double hJ[SD_MAX_L + 1], zJ[SD_MAX_L + 1], f[SD_MAX_L + 1];
  int nb = 0;
  for (int i = 1; i <= L - 1; ++i) { hi[nb] = i; hj[nb] = i + 1; hJ[nb] = Jxy / 2; zJ[nb] = Jz; ++nb; }   // src/SpinModel.jl:71-72
  if (boundary == 1 && L > 2) { hi[nb] = L; hj[nb] = 1; hJ[nb] = Jxy / 2; zJ[nb] = Jz; ++nb; }           // :74-78
  for (int i = 0; i < L; ++i) f[i] = hz;                                                              // :87
  return sd_model_create(ctx, L, nup, nb, hi, hj, hJ, nb, hi, hj, zJ, f, out);
}

void sd_model_destroy(sd_model *m) {
  if (!m) return;
  sd_free_device_tables(m);
  delete m;
}

int64_t sd_model_dim(const sd_model *m) { return m ? m->N : -1; }
int sd_model_L(const sd_model *m) { return m ? m->L : -1; }
int sd_model_nup(const sd_model *m) { return m ? m->nup : -2; }
int sd_ctx_set_apply_callback(sd_ctx *ctx, sd_apply_fn fn, void *user) {
  if (!ctx) return SD_EARG;
  ctx->user_apply = fn;
  ctx->user_apply_data = fn ? user : nullptr;
  return SD_OK;
}
int sd_model_path(const sd_model *m) { return !m ? 0 : m->p >= 0 ? 1 : m->full_ls > 0 ? 2 : 0; }

int sd_model_states(const sd_model *m, int64_t start, int64_t count, uint64_t *out) {
  if (!m || !out || start < 0 || count < 0 || start + count > m->N) return SD_EARG;
  for (int64_t i = 0; i < count; ++i) out[i] = sd_unrank_host(m, start + i);
  return SD_OK;
}

int sd_model_rank(const sd_model *m, const uint64_t *states, int64_t n, int64_t *idx) {
  if (!m || !states || !idx || n < 0) return SD_EARG;
  for (int64_t i = 0; i < n; ++i) idx[i] = sd_rank_host(m, states[i]);
  return SD_OK;
}

int sd_model_set_shard_mode(sd_model *m, int rank, int nranks, int mode) {
  if (!m || mode < -1 || mode > 1) return SD_EARG;
  m->shard_mode_req = mode;
  return sd_model_set_shard(m, rank, nranks);
}

int sd_model_set_shard(sd_model *m, int rank, int nranks) {
  if (!m) return SD_EARG;
  std::string err;
  int rc = plan_and_upload(m, rank, nranks, err);
  if (rc) {
    // The host tables may be partly those of the new (rank, nranks) while the device tables still describe the old plan:
    // no kernel may run on that mixture.  The model is left without a plan -- every later call that needs one fails with
    // SD_EARG ("model has no device tables") -- until a set_shard succeeds; the caller is expected to destroy it.
    sd_free_device_tables(m);
    m->dev_ready = false;
    m->n_local = 0; m->n_halo = 0; m->n_send = 0; m->n_interior = 0;
    m->tile_prefix.clear(); m->tile_base.clear();
    m->recv_slabs.clear(); m->send_slabs.clear();
    m->pack_len.clear();
    return fail(m->ctx, rc, err);
  }
  return SD_OK;
}

int sd_model_shard_info(const sd_model *m, sd_shard_info *out) {
  if (!m || !out) return SD_EARG;
  out->rank = m->rank; out->nranks = m->nranks;
  out->row_lo = m->row_lo; out->row_hi = m->row_hi;
  out->n_local = m->n_local; out->n_halo = m->n_halo;
  out->n_recv_slabs = (int64_t)m->recv_slabs.size(); out->n_send_slabs = (int64_t)m->send_slabs.size();
  out->mode = m->shard_mode; out->n_send = m->n_send; out->n_local_tiles = (int64_t)m->tile_prefix.size();
  out->n_pack = (int64_t)m->pack_len.size();
  out->n_interior_tiles = m->n_interior;
  out->n_interior_rows = 0;
  if (m->p >= 0)
    for (int k = 0; k < m->n_interior && k < (int)m->single_prefix.size(); ++k)
      out->n_interior_rows += sd_binom(m->LS, m->nup - __builtin_popcount(m->single_prefix[k]));
  out->packed = m->packed;
  return SD_OK;
}

int sd_model_shard_slabs(const sd_model *m, sd_slab *recv_out, sd_slab *send_out) {
  if (!m) return SD_EARG;
  if (recv_out) for (size_t i = 0; i < m->recv_slabs.size(); ++i) recv_out[i] = m->recv_slabs[i];
  if (send_out) for (size_t i = 0; i < m->send_slabs.size(); ++i) send_out[i] = m->send_slabs[i];
  return SD_OK;
}

int sd_model_local_tiles(const sd_model *m, int64_t *local_base, int64_t *global_base, int32_t *len) {
  if (!m || m->p < 0) return SD_EARG;
  for (size_t k = 0; k < m->tile_prefix.size(); ++k) {
    if (local_base) local_base[k] = m->tile_base[k];
    if (global_base) global_base[k] = m->tile_gbase.size() == m->tile_prefix.size() ? m->tile_gbase[k] : -1;
    if (len) len[k] = (int32_t)sd_binom(m->LS, m->nup - __builtin_popcount(m->tile_prefix[k]));
  }
  return SD_OK;
}

int sd_model_shard_pack_list(const sd_model *m, int64_t *src, int64_t *dst, int32_t *len) {
  if (!m) return SD_EARG;
  for (size_t k = 0; k < m->pack_len.size(); ++k) {
    if (src) src[k] = m->pack_src[k];
    if (dst) dst[k] = m->pack_dst[k];
    if (len) len[k] = m->pack_len[k];
  }
  return SD_OK;
}

int sd_shard_pack_dev(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi_dev, void *sendbuf_dev) {
  if (!ctx) return SD_EARG;
  if (!m || !psi_dev) return sd_set_err(ctx, SD_EARG, "null argument");
  if (dtype != SD_F64 && dtype != SD_C128) return sd_set_err(ctx, SD_EARG, "bad dtype");
  if (m->n_send > 0 && !sendbuf_dev) return sd_set_err(ctx, SD_EARG, "this shard needs a send buffer");
  return sd_launch_pack(ctx, m, dtype, psi_dev, sendbuf_dev);
}

int sd_fill_randn_local_dev(sd_ctx *ctx, const sd_model *m, int dtype, void *x_dev, uint64_t seed) {
  if (!ctx) return SD_EARG;
  if (!m || !x_dev) return sd_set_err(ctx, SD_EARG, "null argument");
  if (dtype != SD_F64 && dtype != SD_C128) return sd_set_err(ctx, SD_EARG, "bad dtype");
  return sd_launch_fill_randn_local(ctx, m, dtype, x_dev, seed);
}

// ---- operator level ----

int sd_apply_dev(sd_ctx *ctx, const sd_model *m, int dtype, void *out, const void *psi, int64_t n) {
  int rc = check_apply_args(ctx, m, dtype, out, psi, n);
  if (rc) return rc;
  if (n != m->n_local) return sd_set_err(ctx, SD_EDIM, "vector length does not match the (local) basis dimension");
  sd_epi_args ea;
  return sd_launch_apply(ctx, m, dtype, out, psi, SD_EPI_PLAIN, ea);
}

int sd_kpm_step_sharded_dev(sd_ctx *ctx, const sd_model *m, void *v_next, const void *v_curr, const void *halo,
                            const void *v_prev, const void *phi, int64_t n_local, double a, double b, int first,
                            double *sums_out) {
  // one KPM recursion step on this shard (src/KPM_Sqw.jl:106-117): first != 0: v_next = H~ v_curr; else
  // v_next = 2 H~ v_curr - v_prev.  sums_out = local { Re<phi|v_next>, |v_next|^2 } (all-reduce them over the ranks);
  // phi == NULL: Re<v_curr|v_next> instead (moment doubling, no extra vector read).
  int rc = check_apply_args(ctx, m, SD_C128, v_next, v_curr, n_local);
  if (rc) return rc;
  if (n_local != m->n_local) return sd_set_err(ctx, SD_EDIM, "vector length does not match the local basis dimension");
  if (!sums_out || (!first && !v_prev)) return sd_set_err(ctx, SD_EARG, "null argument");   // phi may be null: <v_curr|v_next>
  if (m->n_halo > 0 && !halo) return sd_set_err(ctx, SD_EARG, "this shard needs a halo buffer");
  sd_epi_args ea; ea.a = a; ea.b = b; ea.prev = v_prev; ea.phi = phi; ea.halo = halo;
  rc = sd_launch_apply(ctx, m, SD_C128, v_next, v_curr, first ? SD_EPI_RESCALE_DOT : SD_EPI_KPM, ea, 0);
  if (rc) return rc;
  return sd_read_scalars(ctx, 0, 2, sums_out);
}

int sd_apply_sharded_dev(sd_ctx *ctx, const sd_model *m, int dtype, void *out, const void *psi, const void *halo,
                         int64_t n_local, int epilogue, double a, double b, double c_re, double c_im,
                         const void *phi_prev, void *psi_t, int part) {
  int rc = check_apply_args(ctx, m, dtype, out, psi, n_local);
  if (rc) return rc;
  if (n_local != m->n_local) return sd_set_err(ctx, SD_EDIM, "vector length does not match the local basis dimension");
  if (part < 0 || part > 2) return sd_set_err(ctx, SD_EARG, "part must be 0 (all), 1 (interior) or 2 (boundary)");
  if (m->n_halo > 0 && !halo && part != 1) return sd_set_err(ctx, SD_EARG, "this shard needs a halo buffer");
  sd_epi_args ea; ea.a = a; ea.b = b; ea.c_re = c_re; ea.c_im = c_im; ea.prev = phi_prev; ea.accv = psi_t; ea.halo = halo;
  int epi;
  switch (epilogue) {
    case 0: epi = SD_EPI_PLAIN; break;
    case 1: epi = SD_EPI_RESCALE; break;
    case 2:
      if (dtype != SD_C128 || !phi_prev || !psi_t) return sd_set_err(ctx, SD_EARG, "Chebyshev epilogue needs ComplexF64 phi_prev and psi_t");
      epi = SD_EPI_CHEB; break;
    case 3:
      if (!phi_prev) return sd_set_err(ctx, SD_EARG, "recurrence epilogue needs phi_prev");
      epi = SD_EPI_RECUR; break;
    default: return sd_set_err(ctx, SD_EARG, "unknown epilogue");
  }
  return sd_launch_apply(ctx, m, dtype, out, psi, epi, ea, part);
}

int sd_apply_sharded_cheb2_dev(sd_ctx *ctx, const sd_model *m, void *out, const void *psi, const void *halo, int64_t n_local,
                               double a, double b, double c0_re, double c0_im, double c_re, double c_im,
                               const void *phi_prev, void *psi_t, int part) {
  int rc = check_apply_args(ctx, m, SD_C128, out, psi, n_local);
  if (rc) return rc;
  if (n_local != m->n_local) return sd_set_err(ctx, SD_EDIM, "vector length does not match the local basis dimension");
  if (part < 0 || part > 2) return sd_set_err(ctx, SD_EARG, "part must be 0 (all), 1 (interior) or 2 (boundary)");
  if (m->n_halo > 0 && !halo && part != 1) return sd_set_err(ctx, SD_EARG, "this shard needs a halo buffer");
  if (!phi_prev || !psi_t) return sd_set_err(ctx, SD_EARG, "null vector");
  sd_epi_args ea; ea.a = a; ea.b = b; ea.c0_re = c0_re; ea.c0_im = c0_im; ea.c_re = c_re; ea.c_im = c_im;
  ea.prev = phi_prev; ea.accv = psi_t; ea.halo = halo;
  return sd_launch_apply(ctx, m, SD_C128, out, psi, SD_EPI_CHEB2, ea, part);
}

int sd_apply_rescaled_dev(sd_ctx *ctx, const sd_model *m, int dtype, void *out, const void *psi, int64_t n, double a,
                          double b) {
  int rc = check_apply_args(ctx, m, dtype, out, psi, n);
  if (rc) return rc;
  if (n != m->n_local) return sd_set_err(ctx, SD_EDIM, "vector length does not match the (local) basis dimension");
  sd_epi_args ea; ea.a = a; ea.b = b;
  return sd_launch_apply(ctx, m, dtype, out, psi, SD_EPI_RESCALE, ea);
}

int sd_cheb_step_dev(sd_ctx *ctx, const sd_model *m, void *phi_next, const void *phi_curr, const void *phi_prev,
                     void *psi_t, int64_t n, double a, double b, double c_re, double c_im) {
  int rc = check_apply_args(ctx, m, SD_C128, phi_next, phi_curr, n);
  if (rc) return rc;
  if (!phi_prev || !psi_t) return sd_set_err(ctx, SD_EARG, "null vector");
  if (n != m->n_local) return sd_set_err(ctx, SD_EDIM, "vector length does not match the (local) basis dimension");
  sd_epi_args ea; ea.a = a; ea.b = b; ea.c_re = c_re; ea.c_im = c_im; ea.prev = phi_prev; ea.accv = psi_t;
  return sd_launch_apply(ctx, m, SD_C128, phi_next, phi_curr, SD_EPI_CHEB, ea);
}

static int apply_host(sd_ctx *ctx, const sd_model *m, int dtype, void *out, const void *psi, int64_t n, int epi,
                      double a, double b) {
  int rc = check_apply_args(ctx, m, dtype, out, psi, n);
  if (rc) return rc;
  if (m->nranks != 1) return sd_set_err(ctx, SD_EARG, "host-pointer applies need an unsharded model");
  if (n != m->N) return sd_set_err(ctx, SD_EDIM, "vector length does not match the basis dimension");
  const size_t bytes = (size_t)n * (dtype == SD_C128 ? 16 : 8);
  void *din, *dout;
  if ((rc = stage_buf(ctx, 0, bytes, &din)) || (rc = stage_buf(ctx, 1, bytes, &dout))) return rc;
  if ((rc = sd_xfer_h2d(ctx, din, psi, bytes))) return rc;
  sd_epi_args ea; ea.a = a; ea.b = b;
  rc = sd_launch_apply(ctx, m, dtype, dout, din, epi, ea);
  if (rc) return rc;
  return sd_xfer_d2h(ctx, out, dout, bytes);
}

int sd_apply(sd_ctx *ctx, const sd_model *m, int dtype, void *out, const void *psi, int64_t n) {
  return apply_host(ctx, m, dtype, out, psi, n, SD_EPI_PLAIN, 1.0, 0.0);
}

int sd_apply_rescaled(sd_ctx *ctx, const sd_model *m, int dtype, void *out, const void *psi, int64_t n, double a, double b) {
  return apply_host(ctx, m, dtype, out, psi, n, SD_EPI_RESCALE, a, b);
}

int sd_szq_dev(sd_ctx *ctx, const sd_model *m, int dtype_in, const void *psi0, int64_t n, double q, void *phi) {
  if (!ctx) return SD_EARG;
  if (!m || !psi0 || !phi) return sd_set_err(ctx, SD_EARG, "null argument");
  if (n != m->n_local) return sd_set_err(ctx, SD_EDIM, "vector length does not match the (local) basis dimension");
  return sd_launch_szq(ctx, m, dtype_in, psi0, q, phi);
}

int sd_szq(sd_ctx *ctx, const sd_model *m, int dtype_in, const void *psi0, int64_t n, double q, void *phi) {
  if (!ctx) return SD_EARG;
  if (!m || !psi0 || !phi) return sd_set_err(ctx, SD_EARG, "null argument");
  if (dtype_in != SD_F64 && dtype_in != SD_C128) return sd_set_err(ctx, SD_EARG, "bad dtype");
  if (m->nranks != 1) return sd_set_err(ctx, SD_EARG, "host-pointer entry points need an unsharded model");
  if (n != m->N) return sd_set_err(ctx, SD_EDIM, "vector length does not match the basis dimension");
  const size_t bin = (size_t)n * (dtype_in == SD_C128 ? 16 : 8), bout = (size_t)n * 16;
  TmpDev din(ctx), dout(ctx);
  int rc;
  if ((rc = din.alloc(bin)) || (rc = dout.alloc(bout))) return rc;
  if ((rc = sd_xfer_h2d(ctx, din.p, psi0, bin))) return rc;
  rc = sd_launch_szq(ctx, m, dtype_in, din.p, q, dout.p);
  if (rc) return rc;
  return sd_xfer_d2h(ctx, phi, dout.p, bout);
}

int sd_bench_apply_dev(sd_ctx *ctx, const sd_model *m, int dtype, void *buf_a, void *buf_b, int64_t n, int reps,
                       float *ms_per_apply) {
  int rc = check_apply_args(ctx, m, dtype, buf_a, buf_b, n);
  if (rc) return rc;
  if (n != m->n_local) return sd_set_err(ctx, SD_EDIM, "vector length does not match the (local) basis dimension");
  if (reps < 1 || !ms_per_apply) return sd_set_err(ctx, SD_EARG, "bad reps");
  sd_epi_args ea;
  void *src = buf_a, *dst = buf_b;
  SD_HIP(ctx, hipEventRecord(ctx->ev0, ctx->stream));
  for (int r = 0; r < reps; ++r) {
    rc = sd_launch_apply(ctx, m, dtype, dst, src, SD_EPI_PLAIN, ea);
    if (rc) return rc;
    void *t = src; src = dst; dst = t;
  }
  SD_HIP(ctx, hipEventRecord(ctx->ev1, ctx->stream));
  SD_HIP(ctx, hipEventSynchronize(ctx->ev1));
  float ms = 0.f;
  SD_HIP(ctx, hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
  *ms_per_apply = ms / reps;
  return SD_OK;
}

// ---- observables / initial states ("next" rows f2, f3) ----

static int obs_dev(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi, int64_t n, int what, double *out, double *q_out) {
  if (!ctx) return SD_EARG;
  if (!m || !psi || !out) return sd_set_err(ctx, SD_EARG, "null argument");
  if (m->nranks != 1) return sd_set_err(ctx, SD_EARG, "observables need an unsharded model");
  if (n != m->N) return sd_set_err(ctx, SD_EDIM, "vector length does not match the basis dimension");
  const int L = m->L;
  if (what == 0) return sd_launch_observable(ctx, m, dtype, psi, 0, out);       // magnetization_per_site
  std::vector<double> S(L), R(L), Cr(L);
  RC(sd_launch_observable(ctx, m, dtype, psi, 0, S.data()));
  RC(sd_launch_observable(ctx, m, dtype, psi, 1, R.data()));
  for (int r = 0; r < L; ++r) {                                                   // src/Observables.jl:83-91
    double prod = 0.0;
    for (int i = 1; i <= L; ++i) { const int j = ((i + r - 1) % L) + 1; prod += S[i - 1] * S[j - 1]; }
    Cr[r] = (R[r] - prod) / L;
  }
  if (what == 1) { for (int r = 0; r < L; ++r) out[r] = Cr[r]; return SD_OK; }
  const double PI = 3.14159265358979323846;                                      // :100-109, plain DFT of C_r
  for (int k = 0; k < L; ++k) {
    double s = 0.0;
    for (int r = 0; r < L; ++r) s += Cr[r] * std::cos(2 * PI * k * r / L);
    out[k] = s;
    if (q_out) q_out[k] = 2 * PI * k / L;
  }
  return SD_OK;
}

static int obs_host(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi, int64_t n, int what, double *out, double *q_out) {
  if (!ctx) return SD_EARG;
  if (!m || !psi || !out) return sd_set_err(ctx, SD_EARG, "null argument");
  if (dtype != SD_F64 && dtype != SD_C128) return sd_set_err(ctx, SD_EARG, "bad dtype");
  if (n != m->N) return sd_set_err(ctx, SD_EDIM, "vector length does not match the basis dimension");
  const size_t bytes = (size_t)n * (dtype == SD_C128 ? 16 : 8);
  TmpDev d(ctx);
  RC(d.alloc(bytes));
  RC(sd_xfer_h2d(ctx, d.p, psi, bytes));
  return obs_dev(ctx, m, dtype, d.p, n, what, out, q_out);
}

int sd_magnetization(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi_host, int64_t n, double *mags_out) {
  return abi_guard(ctx, [&]() -> int { return obs_host(ctx, m, dtype, psi_host, n, 0, mags_out, nullptr); });
}
int sd_magnetization_dev(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi_dev, int64_t n, double *mags_out) {
  return abi_guard(ctx, [&]() -> int { return obs_dev(ctx, m, dtype, psi_dev, n, 0, mags_out, nullptr); });
}
int sd_connected_correlations(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi_host, int64_t n, double *C_out) {
  return abi_guard(ctx, [&]() -> int { return obs_host(ctx, m, dtype, psi_host, n, 1, C_out, nullptr); });
}
int sd_connected_correlations_dev(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi_dev, int64_t n, double *C_out) {
  return abi_guard(ctx, [&]() -> int { return obs_dev(ctx, m, dtype, psi_dev, n, 1, C_out, nullptr); });
}
int sd_structure_factor(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi_host, int64_t n, double *q_out, double *S_out) {
  return abi_guard(ctx, [&]() -> int { return obs_host(ctx, m, dtype, psi_host, n, 2, S_out, q_out); });
}
int sd_structure_factor_dev(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi_dev, int64_t n, double *q_out, double *S_out) {
  return abi_guard(ctx, [&]() -> int { return obs_dev(ctx, m, dtype, psi_dev, n, 2, S_out, q_out); });
}

int sd_spin_operator(sd_ctx *ctx, const sd_model *m, int dtype, int site, int op, const void *psi_host, int64_t n,
                     void *out_host) {
  // create_spin_operator(site, op)(psi, model)  -- src/Hamiltonian.jl:49-136
  if (!ctx) return SD_EARG;
  if (!m || !psi_host || !out_host) return sd_set_err(ctx, SD_EARG, "null argument");
  if (site < 1) return sd_set_err(ctx, SD_EARG, "site must be at least 1");                                    // :50
  if (op < SD_SPIN_Z || op > SD_SPIN_Y) return sd_set_err(ctx, SD_EARG, "unsupported spin operator");        // :52-55
  if (site > m->L) return sd_set_err(ctx, SD_EARG, "site is outside the model");                             // :60-61
  if (dtype != SD_F64 && dtype != SD_C128) return sd_set_err(ctx, SD_EARG, "bad dtype");
  if (n != m->N) return sd_set_err(ctx, SD_EDIM, "state vector length does not match the basis");             // :63-66
  if (m->nup >= 0 && op != SD_SPIN_Z)                                                                          // :68-73
    return sd_set_err(ctx, SD_EARG, "operator changes total magnetization and cannot be applied within a fixed-nup sector");
  if (op == SD_SPIN_Y && dtype != SD_C128)   // result[...] += ±0.5im*psi into zeros(Float64) is an InexactError upstream (:118-127)
    return sd_set_err(ctx, SD_EARG, "S^y of a Float64 vector is complex: pass ComplexF64");
  if (m->nranks != 1) return sd_set_err(ctx, SD_EARG, "needs an unsharded model");
  const size_t bin = (size_t)n * (dtype == SD_C128 ? 16 : 8), bout = bin;
  TmpDev din(ctx), dout(ctx);
  int rc;
  if ((rc = din.alloc(bin)) || (rc = dout.alloc(bout))) return rc;
  if ((rc = sd_xfer_h2d(ctx, din.p, psi_host, bin))) return rc;
  rc = sd_launch_spin_op(ctx, m, dtype, site, op, din.p, dout.p);
  if (rc) return rc;
  return sd_xfer_d2h(ctx, out_host, dout.p, bout);
}

int sd_initial_state_index(const sd_model *m, int kind, const int *flips, int nflips, int64_t *idx0_out) {
  if (!m || !idx0_out || nflips < 0 || (nflips && !flips)) return SD_EARG;
  const int L = m->L;
  uint64_t s = 0;
  if (kind == SD_STATE_DOMAIN_WALL) {                          // src/InitialStates.jl:9-34
    const int nup = m->nup >= 0 ? m->nup : (L + 1) / 2;
    for (int i = 0; i < nup; ++i) s |= (uint64_t)1 << i;
  } else if (kind == SD_STATE_NEEL) {                          // :40-63
    for (int i = 0; i < L; i += 2) s |= (uint64_t)1 << i;
  } else if (kind == SD_STATE_POLARIZED_UP) {                  // :70-89
    s = ((uint64_t)1 << L) - 1;
  } else if (kind == SD_STATE_POLARIZED_DOWN) {
    s = 0;
  } else if (kind == SD_STATE_POLARIZED_FLIPS) {               // :97-130
    for (int k = 0; k < nflips; ++k) if (flips[k] < 1 || flips[k] > L) return fail(m->ctx, SD_EARG, "flip site is outside the model");
    s = ((uint64_t)1 << L) - 1;
    for (int k = 0; k < nflips; ++k) s ^= (uint64_t)1 << (flips[k] - 1);
  } else return fail(m->ctx, SD_EARG, "unknown initial-state kind");
  const int64_t idx = sd_rank_host(m, s);
  if (idx < 0) return fail(m->ctx, SD_EARG, "requested state is not contained in the model basis");
  *idx0_out = idx;
  return SD_OK;
}

int sd_fill_randn_dev(sd_ctx *ctx, void *x, int64_t n, uint64_t seed, uint64_t first) {
  if (!ctx) return SD_EARG;
  if (!x || n < 0) return sd_set_err(ctx, SD_EARG, "bad argument");
  return sd_k_fill_randn(ctx, (double *)x, n, seed, first);
}

int sd_dot_dev(sd_ctx *ctx, int dtype, const void *x, const void *y, int64_t n, double *out) {
  if (!ctx) return SD_EARG;
  if (!out || n < 0 || (n > 0 && (!x || !y))) return sd_set_err(ctx, SD_EARG, "bad argument");
  if (dtype != SD_F64 && dtype != SD_C128) return sd_set_err(ctx, SD_EARG, "bad dtype");
  out[0] = out[1] = 0.0;
  if (n == 0) return SD_OK;
  int rc = sd_k_dot(ctx, dtype == SD_C128 ? 2 : 1, (const double *)x, (const double *)y, n, 4);
  if (rc) return rc;
  return sd_read_scalars(ctx, 4, dtype == SD_C128 ? 2 : 1, out);
}

int sd_nrm2sq_dev(sd_ctx *ctx, int dtype, const void *x, int64_t n, double *out) {
  if (!ctx) return SD_EARG;
  if (!out || n < 0 || (n > 0 && !x)) return sd_set_err(ctx, SD_EARG, "bad argument");
  if (dtype != SD_F64 && dtype != SD_C128) return sd_set_err(ctx, SD_EARG, "bad dtype");
  *out = 0.0;
  if (n == 0) return SD_OK;
  int rc = sd_k_nrm2sq(ctx, (const double *)x, n * (dtype == SD_C128 ? 2 : 1), 4);
  if (rc) return rc;
  return sd_read_scalars(ctx, 4, 1, out);
}

int sd_fill_randn_host(double *x, int64_t n, uint64_t seed, uint64_t first) {
  if (!x || n < 0) return SD_EARG;
  for (int64_t i = 0; i < n; ++i) x[i] = sd_randn_host(seed, first + (uint64_t)i);
  return SD_OK;
}

}  // extern "C"

// ---- entanglement across a chain cut (cut_plan.cpp, kernels_cut.hip) ----
namespace {
int cut_gram_core(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi, int64_t n, int cut, int side, void *G_out, bool on_dev,
                  double *kernel_ms = nullptr) {
  if (!ctx) return SD_EARG;
  if (!m || !psi || (!G_out && !kernel_ms)) return sd_set_err(ctx, SD_EARG, "null argument");
  if (!m->dev_ready) return sd_set_err(ctx, SD_EARG, "model has no device tables (created without a context)");
  if (dtype != SD_F64 && dtype != SD_C128) return sd_set_err(ctx, SD_EARG, "dtype must be SD_F64 or SD_C128");
  sd_cut_plan plan;
  std::string err;
  if (int rc = sd_cut_build_plan(m, cut, side, true, plan, err)) return sd_set_err(ctx, rc, err);
  if (n != m->N) return sd_set_err(ctx, SD_EDIM, "vector length does not match the basis dimension");
  const size_t el = dtype == SD_C128 ? 16 : 8, out_bytes = (size_t)plan.n_out * el;
  if (kernel_ms) *kernel_ms = 0.0;
  if (m->N == 0) { if (G_out) memset(G_out, 0, out_bytes); return SD_OK; }
  SD_HIP(ctx, hipSetDevice(ctx->device));
  DevIn in;
  DBuf res;
  RC(in.stage(ctx, dtype, psi, on_dev, n));
  RC(res.alloc_bytes(ctx, out_bytes));
  float ms = 0.0f;
  RC(sd_launch_cut_gram(ctx, m, dtype, in.p, plan, res.p, kernel_ms ? &ms : nullptr));
  if (kernel_ms) *kernel_ms = ms;
  return G_out ? sd_xfer_d2h(ctx, G_out, res.p, out_bytes) : SD_OK;
}
}  // namespace

extern "C" {

int sd_cut_blocks(const sd_model *m, int cut, int side, sd_cut_block *out, int cap, int *n_blocks, int64_t *n_elems) {
  if (!m || !n_blocks || !n_elems || cap < 0 || (cap > 0 && !out)) return SD_EARG;
  return abi_guard(m->ctx, [&]() -> int {
    std::vector<sd_cut_blk> blks;
    std::string err;
    int64_t total = 0;
    const int rc = sd_cut_layout(m, cut, side, blks, &total, err);
    if (rc) return sd_set_err(m->ctx, rc, err);
    *n_blocks = (int)blks.size();
    *n_elems = total;
    if (cap == 0) return SD_OK;
    if (cap < (int)blks.size()) return sd_set_err(m->ctx, SD_EARG, "sd_cut_blocks: cap is below the number of blocks");
    for (size_t i = 0; i < blks.size(); ++i) out[i] = sd_cut_block{blks[i].m, blks[i].side, blks[i].dA, blks[i].dB, blks[i].d, blks[i].out_off};
    return SD_OK;
  });
}

int sd_cut_plan_info(const sd_model *m, int cut, int side, int dtype, int64_t *n_items, int *max_ns, int64_t *workspace_bytes) {
  if (!m || !n_items || !max_ns || !workspace_bytes) return SD_EARG;
  return abi_guard(m->ctx, [&]() -> int {
    if (dtype != SD_F64 && dtype != SD_C128) return sd_set_err(m->ctx, SD_EARG, "dtype must be SD_F64 or SD_C128");
    sd_cut_plan plan;
    std::string err;
    const int rc = sd_cut_build_plan(m, cut, side, false, plan, err);
    if (rc) return sd_set_err(m->ctx, rc, err);
    *n_items = (int64_t)plan.items.size();
    *max_ns = plan.max_ns;
    *workspace_bytes = plan.ws_elems * (dtype == SD_C128 ? 16 : 8);
    return SD_OK;
  });
}

int sd_cut_plan_items(const sd_model *m, int cut, int side, sd_cut_item *out, int64_t cap, int64_t *n_items) {
  if (!m || !n_items || cap < 0 || (cap > 0 && !out)) return SD_EARG;
  return abi_guard(m->ctx, [&]() -> int {
    sd_cut_plan plan;
    std::string err;
    const int rc = sd_cut_build_plan(m, cut, side, false, plan, err);
    if (rc) return sd_set_err(m->ctx, rc, err);
    *n_items = (int64_t)plan.items.size();
    if (cap == 0) return SD_OK;
    if (cap < *n_items) return sd_set_err(m->ctx, SD_EARG, "sd_cut_plan_items: cap is below the number of items");
    std::copy(plan.items.begin(), plan.items.end(), out);
    return SD_OK;
  });
}

int sd_cut_segments(const sd_model *m, int cut, int side, int block, int64_t *starts, int64_t cap, int64_t *n_seg, int64_t *seg_len) {
  if (!m || !n_seg || !seg_len || cap < 0 || (cap > 0 && !starts)) return SD_EARG;
  return abi_guard(m->ctx, [&]() -> int {
    std::vector<sd_cut_blk> blks;
    std::string err;
    const int rc = sd_cut_layout(m, cut, side, blks, nullptr, err);
    if (rc) return sd_set_err(m->ctx, rc, err);
    if (block < 0 || block >= (int)blks.size()) return sd_set_err(m->ctx, SD_EARG, "sd_cut_segments: no such block");
    const sd_cut_blk &b = blks[(size_t)block];
    *n_seg = b.nseg;
    *seg_len = b.seglen;
    if (cap == 0) return SD_OK;
    if (cap < b.nseg) return sd_set_err(m->ctx, SD_EARG, "sd_cut_segments: cap is below the number of segments");
    std::vector<int64_t> segs;
    sd_cut_fill_segments(m, cut, b, segs);
    std::copy(segs.begin(), segs.end(), starts);
    return SD_OK;
  });
}

int sd_cut_gram(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi_host, int64_t n, int cut, int side, void *G_out) {
  return abi_guard(ctx, [&]() -> int { return cut_gram_core(ctx, m, dtype, psi_host, n, cut, side, G_out, false); });
}

int sd_cut_gram_dev(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi_dev, int64_t n, int cut, int side, void *G_out) {
  return abi_guard(ctx, [&]() -> int { return cut_gram_core(ctx, m, dtype, psi_dev, n, cut, side, G_out, true); });
}

int sd_cut_gram_time_dev(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi_dev, int64_t n, int cut, int side, double *kernel_ms) {
  if (ctx && !kernel_ms) return sd_set_err(ctx, SD_EARG, "null argument");
  return abi_guard(ctx, [&]() -> int { return cut_gram_core(ctx, m, dtype, psi_dev, n, cut, side, nullptr, true, kernel_ms); });
}

}  // extern "C"

// ---- site permutations and the entanglement of any set of sites (site_perm.hpp, kernels_permute.hip) ----
namespace {
// what every vector call checks before anything is queued; pm receives the permutation
int permute_args(sd_ctx *ctx, const sd_model *m, int dtype, const int *perm, sd_site_perm &pm, int *identity) {
  if (!m->dev_ready) return sd_set_err(ctx, SD_EARG, "model has no device tables (created without a context)");
  if (dtype != SD_F64 && dtype != SD_C128) return sd_set_err(ctx, SD_EARG, "dtype must be SD_F64 or SD_C128");
  if (m->nranks != 1) return sd_set_err(ctx, SD_EARG, "site permutations need an unsharded model");
  if (!sd_site_perm_make(perm, m->L, &pm, identity)) return sd_set_err(ctx, SD_EARG, "perm must be a bijection of 1..L");
  return SD_OK;
}

int site_permute_core(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi, int64_t n, const int *perm, void *out, bool on_dev) {
  if (!ctx) return SD_EARG;
  if (!m || !psi || !perm || !out) return sd_set_err(ctx, SD_EARG, "null argument");
  sd_site_perm pm;
  RC(permute_args(ctx, m, dtype, perm, pm, nullptr));
  if (n != m->N) return sd_set_err(ctx, SD_EDIM, "vector length does not match the basis dimension");
  const size_t bytes = (size_t)n * (dtype == SD_C128 ? 16 : 8);
  if (ranges_overlap(out, bytes, psi, bytes)) return sd_set_err(ctx, SD_EARG, "out must not alias or overlap psi");
  if (n == 0) return SD_OK;
  SD_HIP(ctx, hipSetDevice(ctx->device));
  DevIn in;
  DevOut o;
  RC(in.stage(ctx, dtype, psi, on_dev, n));
  RC(o.open(ctx, out, on_dev, vec_doubles(dtype, n)));
  RC(sd_launch_site_permute(ctx, m, dtype, pm, in.p, o.p));
  return o.close(false);                                   // the device form takes nothing from the pool
}

int subsystem_perm(int L, const int *sites, int n_sites, int *perm_out) {
  if (L < 2 || L > SD_MAX_L || !sites || !perm_out || n_sites < 1 || n_sites > L - 1) return SD_EARG;
  uint64_t seen = 0;
  for (int j = 0; j < n_sites; ++j) {
    const int s = sites[j];
    if (s < 1 || s > L || ((seen >> (s - 1)) & 1)) return SD_EARG;
    seen |= (uint64_t)1 << (s - 1);
    perm_out[s - 1] = j + 1;
  }
  int next = n_sites + 1;
  for (int i = 0; i < L; ++i)
    if (!((seen >> i) & 1)) perm_out[i] = next++;
  return SD_OK;
}

int subsystem_gram_core(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi, int64_t n, const int *sites, int n_sites, int side,
                        void *G_out, bool on_dev) {
  if (!ctx) return SD_EARG;
  if (!m || !psi || !sites || !G_out) return sd_set_err(ctx, SD_EARG, "null argument");
  int perm[SD_MAX_L + 1];
  if (subsystem_perm(m->L, sites, n_sites, perm))
    return sd_set_err(ctx, SD_EARG, "the sites must be distinct, in 1..L, and 1 <= n_sites <= L - 1");
  sd_site_perm pm;
  int identity = 0;
  RC(permute_args(ctx, m, dtype, perm, pm, &identity));
  std::vector<sd_cut_blk> blks;         // the cut's own refusals (side, block dimension) before anything is queued
  std::string err;
  if (int rc = sd_cut_layout(m, n_sites, side, blks, nullptr, err)) return sd_set_err(ctx, rc, err);
  if (n != m->N) return sd_set_err(ctx, SD_EDIM, "vector length does not match the basis dimension");
  if (identity || n == 0) return cut_gram_core(ctx, m, dtype, psi, n, n_sites, side, G_out, on_dev);
  SD_HIP(ctx, hipSetDevice(ctx->device));
  DevIn in;
  DBuf tmp;
  RC(in.stage(ctx, dtype, psi, on_dev, n));
  RC(tmp.alloc(ctx, vec_doubles(dtype, n)));
  RC(sd_launch_site_permute(ctx, m, dtype, pm, in.p, tmp.p));
  return cut_gram_core(ctx, m, dtype, tmp.p, n, n_sites, side, G_out, true);   // returns after the stream has drained
}
}  // namespace

extern "C" {

int sd_site_permute(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi_host, int64_t n, const int *perm, void *out_host) {
  return abi_guard(ctx, [&]() -> int { return site_permute_core(ctx, m, dtype, psi_host, n, perm, out_host, false); });
}

int sd_site_permute_dev(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi_dev, int64_t n, const int *perm, void *out_dev) {
  return abi_guard(ctx, [&]() -> int { return site_permute_core(ctx, m, dtype, psi_dev, n, perm, out_dev, true); });
}

int sd_site_permute_sources(const sd_model *m, const int *perm, int64_t start, int64_t count, int64_t *rows_out) {
  if (!m) return SD_EARG;
  if (!perm || start < 0 || count < 0 || start > m->N - count || (count > 0 && !rows_out))
    return sd_set_err(m->ctx, SD_EARG, "sd_site_permute_sources: null argument or rows outside the basis");
  return abi_guard(m->ctx, [&]() -> int {
    sd_site_perm pm;
    if (!sd_site_perm_make(perm, m->L, &pm, nullptr)) return sd_set_err(m->ctx, SD_EARG, "perm must be a bijection of 1..L");
    const int ntab = (m->L + 7) / 8;
    std::vector<uint64_t> lut((size_t)256 * ntab);
    sd_site_perm_fill(lut.data(), pm, m->L, 0, ntab, 0, 1);
    for (int64_t k = 0; k < count; ++k)
      rows_out[k] = sd_rank_host(m, sd_site_perm_source(lut.data(), ntab, sd_unrank_host(m, start + k)));
    return SD_OK;
  });
}

int sd_subsystem_permutation(int L, const int *sites, int n_sites, int *perm_out) { return subsystem_perm(L, sites, n_sites, perm_out); }

int sd_subsystem_gram(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi_host, int64_t n, const int *sites, int n_sites, int side,
                      void *G_out) {
  return abi_guard(ctx, [&]() -> int { return subsystem_gram_core(ctx, m, dtype, psi_host, n, sites, n_sites, side, G_out, false); });
}

int sd_subsystem_gram_dev(sd_ctx *ctx, const sd_model *m, int dtype, const void *psi_dev, int64_t n, const int *sites, int n_sites, int side,
                          void *G_out) {
  return abi_guard(ctx, [&]() -> int { return subsystem_gram_core(ctx, m, dtype, psi_dev, n, sites, n_sites, side, G_out, true); });
}

}  // extern "C"

// ---- diagonal drives: the limits of a drive list and the table of one stage's effective operator ----
// coef == null: the limits alone, nothing is written to `out`.
int sd_drive_build(const sd_model *m, const sd_drive *drives, int K, const double *coef, sd_drive_table &out, std::string &err) {
  if (!m) { err = "null model"; return SD_EARG; }
  if (K < 0 || K > SD_DRIVE_MAX) { err = "the number of drives must be 0.." + std::to_string(SD_DRIVE_MAX); return SD_EARG; }
  if (K > 0 && !drives) { err = "null drive list"; return SD_EARG; }
  if (m->L < 1 || m->L > SD_MAX_L) { err = "diagonal drives need 1 <= L <= 63"; return SD_EARG; }
  if (m->nranks != 1) { err = "diagonal drives need an unsharded model"; return SD_EARG; }
  const int L = m->L;
  int nb = 0;
  bool sites = false;
  for (int k = 0; k < K; ++k) {
    const sd_drive &d = drives[k];
    if (coef && !std::isfinite(coef[k])) { err = "drive coefficient " + std::to_string(k) + " is not finite"; return SD_EARG; }
    if (d.site_w) {
      sites = true;
      for (int i = 0; i < L; ++i)
        if (!std::isfinite(d.site_w[i])) { err = "drive " + std::to_string(k) + ": a site weight is not finite"; return SD_EARG; }
    }
    if (d.n_zz < 0) { err = "drive " + std::to_string(k) + ": negative bond count"; return SD_EARG; }
    if (d.n_zz > 0 && (!d.zz_i || !d.zz_j || !d.zz_w)) { err = "drive " + std::to_string(k) + ": null bond list"; return SD_EARG; }
    if (d.n_zz > SD_DRIVE_MAX_BONDS - nb) {
      err = "more than " + std::to_string(SD_DRIVE_MAX_BONDS) + " zz terms in the drives together";
      return SD_EARG;
    }
    for (int b = 0; b < d.n_zz; ++b) {
      const int i = d.zz_i[b], j = d.zz_j[b];
      if (i < 1 || i > L || j < 1 || j > L) { err = "drive " + std::to_string(k) + ": a bond site is outside 1..L"; return SD_EARG; }
      if (i == j) { err = "drive " + std::to_string(k) + ": the two sites of a bond must differ"; return SD_EARG; }
      if (!std::isfinite(d.zz_w[b])) { err = "drive " + std::to_string(k) + ": a bond weight is not finite"; return SD_EARG; }
    }
    nb += d.n_zz;
  }
  if (!coef) return SD_OK;
  std::memset(&out, 0, sizeof(out));
  out.has_sites = sites ? 1 : 0;
  out.n_bonds = nb;
  for (int i = 0; i < L; ++i) {
    double W = 0.0;
    for (int k = 0; k < K; ++k)
      if (drives[k].site_w) { const double t = coef[k] * drives[k].site_w[i]; W = W + t; }
    out.wh[i] = W * 0.5;
  }
  int at = 0;
  for (int k = 0; k < K; ++k)
    for (int b = 0; b < drives[k].n_zz; ++b, ++at) {
      out.vq[at] = (coef[k] * drives[k].zz_w[b]) * 0.25;
      out.bits[at] = (uint32_t)((drives[k].zz_i[b] - 1) | ((drives[k].zz_j[b] - 1) << 8));
    }
  return SD_OK;
}

extern "C" int sd_drive_check(const sd_model *m, const sd_drive *drives, int K) {
  if (!m) return SD_EARG;
  return abi_guard(m->ctx, [&]() -> int {
    std::string err;
    sd_drive_table none;
    const int rc = sd_drive_build(m, drives, K, nullptr, none, err);
    return rc ? sd_set_err(m->ctx, rc, "sd_drive_check: " + err) : SD_OK;
  });
}

// ---- hopping drives: the limits of a hopping-drive list, its form, and the effective list of one stage ----
// coef == null: the limits and the form alone (out.n = the terms of all drives, nothing else written).  coef: KH coefficients.
int sd_hop_build(const sd_model *m, const sd_hop_drive *hops, int KH, int K_diag, const double *coef, sd_hop_table &out, std::string &err) {
  if (!m) { err = "null model"; return SD_EARG; }
  if (KH < 0 || K_diag < 0 || KH > SD_DRIVE_MAX - K_diag) {
    err = "diagonal and hopping drives together must be 0.." + std::to_string(SD_DRIVE_MAX);
    return SD_EARG;
  }
  if (KH > 0 && !hops) { err = "null hopping-drive list"; return SD_EARG; }
  if (m->L < 1 || m->L > SD_MAX_L) { err = "hopping drives need 1 <= L <= 63"; return SD_EARG; }
  if (m->nranks != 1) { err = "hopping drives need an unsharded model"; return SD_EARG; }
  const int L = m->L;
  int nb = 0;
  bool cplx = false;
  for (int k = 0; k < KH; ++k) {
    const sd_hop_drive &d = hops[k];
    const std::string who = "hopping drive " + std::to_string(k);
    if (coef && !std::isfinite(coef[k])) { err = who + ": the coefficient is not finite"; return SD_EARG; }
    if (d.n < 0) { err = who + ": negative bond count"; return SD_EARG; }
    if (d.n > 0 && (!d.i || !d.j || !d.re)) { err = who + ": null bond list"; return SD_EARG; }
    if (d.n > SD_HOP_MAX_BONDS - nb) {
      err = "more than " + std::to_string(SD_HOP_MAX_BONDS) + " hop terms in the drives together";
      return SD_EARG;
    }
    for (int b = 0; b < d.n; ++b) {
      const int i = d.i[b], j = d.j[b];
      if (i < 1 || i > L || j < 1 || j > L) { err = who + ": a bond site is outside 1..L"; return SD_EARG; }
      if (i == j) { err = who + ": the two sites of a bond must differ"; return SD_EARG; }
      if (!std::isfinite(d.re[b]) || (d.im && !std::isfinite(d.im[b]))) { err = who + ": a bond weight is not finite"; return SD_EARG; }
      if (d.im && d.im[b] != 0.0) cplx = true;
    }
    nb += d.n;
  }
  out.complex_form = cplx ? 1 : 0;
  out.n = nb;
  if (!coef) return SD_OK;
  int at = 0;
  for (int k = 0; k < KH; ++k) {
    if (coef[k] == 0.0) continue;                            // a switched-off drive gathers nothing
    const sd_hop_drive &d = hops[k];
    for (int b = 0; b < d.n; ++b, ++at) {
      const int bi = d.i[b] - 1, bj = d.j[b] - 1;
      const int lo = bi < bj ? bi : bj, hi = bi < bj ? bj : bi;
      out.bits[at] = (uint32_t)(lo | (hi << 8) | ((bi > bj ? 1 : 0) << 16));
      out.xy[2 * at] = coef[k] * d.re[b];
      out.xy[2 * at + 1] = d.im ? coef[k] * d.im[b] : 0.0;
    }
  }
  out.n = at;
  return SD_OK;
}

extern "C" int sd_hop_drive_check(const sd_model *m, const sd_hop_drive *hops, int KH) {
  if (!m) return SD_EARG;
  return abi_guard(m->ctx, [&]() -> int {
    std::string err;
    sd_hop_table none;
    const int rc = sd_hop_build(m, hops, KH, 0, nullptr, none, err);
    return rc ? sd_set_err(m->ctx, rc, "sd_hop_drive_check: " + err) : SD_OK;
  });
}
