// The host call layer: what every entry point does between the C ABI and a kernel launch, each behaviour once.
// Host code only: no .hip file includes this header.
#pragma once
#include <algorithm>
#include <cstdint>
#include <new>
#include <stdexcept>
#include <string>
#include <vector>

#include "sd_internal.hpp"

#define RC(x) do { int rc__ = (x); if (rc__) return rc__; } while (0)

// No C++ exception may cross the C ABI: a failed host allocation (std::vector of the m x m work, std::string of a message) inside a
// call comes back as a status.  Every extern "C" entry point that allocates is abi_guard(ctx, [&]() -> int { body }).
template <class F>
int abi_guard(sd_ctx *ctx, F &&body) {
  try {
    return body();
  } catch (const std::bad_alloc &) {
    return ctx ? sd_set_err(ctx, SD_ENOMEM, "out of host memory inside the call") : SD_ENOMEM;
  } catch (const std::exception &e) {
    return ctx ? sd_set_err(ctx, SD_EINTERNAL, std::string("unexpected exception: ") + e.what()) : SD_EINTERNAL;
  } catch (...) {
    return ctx ? sd_set_err(ctx, SD_EINTERNAL, "unexpected exception") : SD_EINTERNAL;
  }
}

// what an unsharded entry point asks of its model before anything else; selects the context's device
inline int check_unsharded_model(sd_ctx *ctx, const sd_model *m) {
  if (!ctx) return SD_EARG;
  if (!m || !m->dev_ready) return sd_set_err(ctx, SD_EARG, "model has no device tables");
  if (m->nranks != 1) return sd_set_err(ctx, SD_EARG, "a sharded model needs a communicator (the unsharded entry points take an unsharded model)");
  SD_HIP(ctx, hipSetDevice(ctx->device));
  return SD_OK;
}

struct DBuf {   // device work vector, taken from / returned to the context's pool
  double *p = nullptr;
  sd_ctx *owner = nullptr;
  size_t bytes = 0;
  DBuf() = default;
  DBuf(const DBuf &) = delete;
  DBuf &operator=(const DBuf &) = delete;
  ~DBuf() { release(); }
  void release() {
    if (p) sd_pool_give(owner, p, bytes);
    p = nullptr; bytes = 0;
  }
  int alloc_bytes(sd_ctx *ctx, size_t want) {
    release();
    owner = ctx;
    void *q = nullptr;
    int rc = sd_pool_take(ctx, std::max(want, sizeof(double)), &q, &bytes);
    p = (double *)q;
    return rc;
  }
  int alloc(sd_ctx *ctx, int64_t doubles) { return alloc_bytes(ctx, sizeof(double) * (size_t)std::max<int64_t>(doubles, 1)); }
};

// the caller's host vectors (src/PublicAPI.jl:50-88): staged through the context's pinned ring when large (xfer.cpp)
inline int h2d(sd_ctx *ctx, double *d, const void *h, int64_t doubles) { return sd_xfer_h2d(ctx, d, h, sizeof(double) * (size_t)doubles); }
inline int d2h(sd_ctx *ctx, void *h, const double *d, int64_t doubles) { return sd_xfer_d2h(ctx, h, d, sizeof(double) * (size_t)doubles); }
inline int d2d(sd_ctx *ctx, double *dst, const double *src, int64_t doubles) {
  SD_HIP(ctx, hipMemcpyAsync(dst, src, sizeof(double) * (size_t)doubles, hipMemcpyDeviceToDevice, ctx->stream));
  return SD_OK;
}

// do the byte ranges [a, a + na) and [b, b + nb) share a byte?  (a gather reads rows of psi that other workgroups' rows of out
// would overwrite: any overlap corrupts the result, not only out == psi)
inline bool ranges_overlap(const void *a, size_t na, const void *b, size_t nb) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x < y + nb && y < x + na;
}

inline int64_t vec_doubles(int dtype, int64_t n) { return (dtype == SD_C128 ? 2 : 1) * n; }

// A caller's input vector (n elements of dtype) on the device in its own element type: the pointer itself when on_dev, else a pool
// block filled from the host vector.
struct DevIn {
  DBuf buf;
  const double *p = nullptr;
  int stage(sd_ctx *ctx, int dtype, const void *v, bool on_dev, int64_t n) {
    if (dtype != SD_F64 && dtype != SD_C128) return sd_set_err(ctx, SD_EARG, "bad dtype");
    if (!v) return sd_set_err(ctx, SD_EARG, "null argument");
    if (on_dev) { p = (const double *)v; return SD_OK; }
    RC(buf.alloc(ctx, vec_doubles(dtype, n))); RC(h2d(ctx, buf.p, v, vec_doubles(dtype, n)));
    p = buf.p;
    return SD_OK;
  }
};

// A caller's output vector: open() gives the device memory to write to -- the caller's own pointer when on_dev, else a pool block --
// and close() delivers it: the host form copies it out (which drains the stream); the device form returns with the work queued,
// or, with sync, after the stream has drained -- needed where a pool block the queued kernels read (a table, a weight list) goes
// back to the pool when the call returns.  Whether an entry synchronises is spelled at its call site; the table is DESIGN.md 4.5.
struct DevOut {
  DBuf buf;
  double *p = nullptr;
  sd_ctx *ctx = nullptr;
  void *host = nullptr;
  int64_t doubles = 0;
  int open(sd_ctx *c, void *out, bool on_dev, int64_t nd) {
    ctx = c; doubles = nd;
    if (on_dev) { p = (double *)out; return SD_OK; }
    host = out;
    RC(buf.alloc(ctx, nd));
    p = buf.p;
    return SD_OK;
  }
  int close(bool sync) {
    if (host) return d2h(ctx, host, p, doubles);
    if (sync) SD_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return SD_OK;
  }
};

// a small result: device -> the caller's host memory, and the stream drained
inline int read_back(sd_ctx *ctx, void *host, const void *dev, size_t bytes) {
  SD_HIP(ctx, hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, ctx->stream));
  SD_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return SD_OK;
}

// Host tables (at most four) packed into one pool block: add() each table (8-byte aligned inside the block; the host copy must live
// until upload() returns), upload() -- once -- takes the block and copies every table in, at<T>(k) is table k on the device.
struct TableBlock {
  DBuf buf;
  struct Part { const void *src; size_t bytes, off; };
  Part parts[4];
  int n_parts = 0;
  size_t total = 0;
  template <class T>
  int add(const T *host, size_t count) {
    parts[n_parts] = Part{host, sizeof(T) * count, total};
    total += (sizeof(T) * count + 7) / 8 * 8;
    return n_parts++;
  }
  int upload(sd_ctx *ctx) {
    RC(buf.alloc_bytes(ctx, total));
    for (int k = 0; k < n_parts; ++k) { RC(sd_xfer_h2d(ctx, (char *)buf.p + parts[k].off, parts[k].src, parts[k].bytes)); parts[k].src = nullptr; }
    return SD_OK;
  }
  template <class T>
  const T *at(int k) const { return (const T *)((const char *)buf.p + parts[k].off); }
};

// ---- shared by observe.cpp and the typicality driver of recur.cpp; defined in observe.cpp ----
// the n_hop products w_b t_b on the device (w == null: ones)
int current_weights(sd_ctx *ctx, const sd_model *m, const double *w, DBuf &wt);
// A caller's list of dressed bond currents (include/spindyn.h, sd_dterm) validated, cut into groups and put on the device: both
// tables in one block from the context's pool, the dressed coefficients halved (exact).  n_groups == 0: the empty list.
struct DList {
  TableBlock tab;
  int n_groups = 0;
  const sd_dgroup *groups = nullptr;
  const sd_dterm_dev *terms = nullptr;
  int init(sd_ctx *ctx, const sd_model *m, const sd_dterm *list, int n_terms);
};
