// The host thread team of the staged host <-> device transfers (xfer.cpp): one copy at a time, cut into page-aligned slices, one
// per member, the caller being member 0.  Standard library only and no HIP header, so that tests/xfer_team_host.cpp can include it
// and run the team on the host alone (tests/test_xfer_team_host.py: the slice bounds over every small length, the copies under
// ThreadSanitizer and AddressSanitizer).
#pragma once
#include <algorithm>
#include <condition_variable>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <thread>
#include <utility>
#include <vector>

struct sd_xfer_team {
  std::vector<std::thread> workers;
  std::mutex mu;
  std::condition_variable cv_work, cv_done;
  char *dst = nullptr;
  const char *src = nullptr;
  size_t bytes = 0;
  uint64_t generation = 0;
  int pending = 0;
  bool stop = false;
  int nthreads = 1;

  explicit sd_xfer_team(int n) : nthreads(n) {
    try {
      for (int t = 1; t < n; ++t) workers.emplace_back([this, t] { loop(t); });
    } catch (...) {            // a destructor is not run for a half-built object: stop and join what did start, then hand the failure on
      { std::lock_guard<std::mutex> lk(mu); stop = true; }
      cv_work.notify_all();
      for (auto &w : workers) w.join();
      throw;
    }
  }
  ~sd_xfer_team() {
    { std::lock_guard<std::mutex> lk(mu); stop = true; }
    cv_work.notify_all();
    for (auto &w : workers) w.join();
  }
  // [lo, hi) of member t of n: the n slices tile [0, bytes) exactly, in ascending order, and every interior boundary is a multiple
  // of 4096 from the start of the buffer.  The slice length is bytes / n rounded UP to a whole byte before it is rounded up to a
  // page: rounding bytes / n down first leaves the last bytes % n bytes to nobody whenever bytes / n is itself a multiple of 4096.
  static std::pair<size_t, size_t> slice_bounds(size_t bytes, int t, int n) {
    const size_t per = ((bytes / (size_t)n + (bytes % (size_t)n != 0)) + 4095) & ~(size_t)4095;
    const size_t lo = std::min(bytes, per * (size_t)t), hi = std::min(bytes, lo + per);
    return {lo, hi};
  }
  static void slice(char *d, const char *s, size_t bytes, int t, int n) {
    // page-aligned slices so that two threads never fault the same page
    const std::pair<size_t, size_t> b = slice_bounds(bytes, t, n);
    if (b.second > b.first) std::memcpy(d + b.first, s + b.first, b.second - b.first);
  }
  void loop(int t) {
    uint64_t seen = 0;
    for (;;) {
      std::unique_lock<std::mutex> lk(mu);
      cv_work.wait(lk, [&] { return stop || generation != seen; });
      if (stop) return;
      seen = generation;
      char *d = dst; const char *s = src; const size_t b = bytes;
      lk.unlock();
      slice(d, s, b, t, nthreads);
      lk.lock();
      if (--pending == 0) cv_done.notify_one();
    }
  }
  // dst[0..bytes) <- src[0..bytes) by the whole team (the caller is member 0); returns when done
  void copy(void *d, const void *s, size_t b) {
    if (nthreads == 1 || b < ((size_t)1 << 20)) { std::memcpy(d, s, b); return; }
    {
      std::lock_guard<std::mutex> lk(mu);
      dst = (char *)d; src = (const char *)s; bytes = b;
      pending = nthreads - 1;
      ++generation;
    }
    cv_work.notify_all();
    slice((char *)d, (const char *)s, b, 0, nthreads);
    std::unique_lock<std::mutex> lk(mu);
    cv_done.wait(lk, [&] { return pending == 0; });
  }
};
