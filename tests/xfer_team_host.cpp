// Host test program of the copy team of the staged transfers (csrc/xfer_team.hpp), driven by tests/test_xfer_team_host.py.
//
//   xfer_team_host bounds              slice_bounds over n = 1..64 and the byte counts listed in check_all_bounds
//   xfer_team_host copy n [reduced]    one team of n threads over a list of copies in sequence
//
// Every failing cell is printed on one line ("FAIL ..."); the last line is "ok <cells>" or "failed <failing cells> of <cells>", and
// the exit status is 0 only when nothing failed.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "xfer_team.hpp"

namespace {

constexpr size_t PAGE = 4096, GUARD = 4096, TEAM_MIN = (size_t)1 << 20;
constexpr unsigned char GUARD_BYTE = 0xA5;

// ---- bounds ----
// "" when the n slices of `bytes` ascend, are disjoint, lie in [0, bytes], cover [0, bytes) and meet at multiples of 4096
std::string bounds_fault(size_t bytes, int n) {
  size_t end = 0, prev_lo = 0;                      // the slices so far cover [0, end) exactly
  char buf[160];
  for (int t = 0; t < n; ++t) {
    const std::pair<size_t, size_t> b = sd_xfer_team::slice_bounds(bytes, t, n);
    const size_t lo = b.first, hi = b.second;
    if (!(lo <= hi && hi <= bytes)) {
      snprintf(buf, sizeof buf, "slice %d = [%zu, %zu) is not inside [0, %zu]", t, lo, hi, bytes);
      return buf;
    }
    if (lo < prev_lo) {
      snprintf(buf, sizeof buf, "slice %d begins at %zu, before slice %d at %zu", t, lo, t - 1, prev_lo);
      return buf;
    }
    prev_lo = lo;
    if (hi > lo) {                                  // an empty slice copies nothing wherever it stands
      if (lo != end) {
        snprintf(buf, sizeof buf, "slice %d begins at %zu, the slices before it end at %zu (%s)", t, lo, end, lo < end ? "overlap" : "gap");
        return buf;
      }
      if (lo % PAGE != 0) {
        snprintf(buf, sizeof buf, "slice %d begins at %zu, no multiple of 4096", t, lo);
        return buf;
      }
      end = hi;
    }
  }
  if (end != bytes) {
    snprintf(buf, sizeof buf, "the slices end at %zu: the last %zu bytes belong to nobody", end, bytes - end);
    return buf;
  }
  return "";
}

int check_all_bounds() {
  long cells = 0, failed = 0;
  auto cell = [&](size_t bytes, int n) {
    ++cells;
    const std::string f = bounds_fault(bytes, n);
    if (!f.empty()) {
      ++failed;
      printf("FAIL bounds n=%d bytes=%zu (bytes/n=%zu, bytes%%n=%zu): %s\n", n, bytes, bytes / (size_t)n, bytes % (size_t)n, f.c_str());
    }
  };
  const size_t js[] = {1, 16, 256, 257};
  for (int n = 1; n <= 64; ++n) {
    for (size_t bytes = 0; bytes <= ((size_t)1 << 17); ++bytes) cell(bytes, n);
    for (size_t j : js)
      for (size_t r = 0; r <= (size_t)n; ++r) cell(PAGE * (size_t)n * j + r, n);
    cell(((size_t)1 << 20) - 8, n);
    cell(((size_t)1 << 20) + 8, n);
    cell(((size_t)1 << 25) + 8, n);
  }
  if (failed) printf("failed %ld of %ld\n", failed, cells);
  else printf("ok %ld\n", cells);
  return failed ? 1 : 0;
}

// ---- copy ----
// byte i of every source, whatever the length and the address: a hash of the offset, so that a slice copied from or to a shifted
// offset, or twice, does not compare equal
unsigned char pattern_byte(uint64_t i) {
  uint64_t z = (i + 1) * 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return (unsigned char)(z >> 56);
}

// the smallest 4096 n j + r >= 2^20 (j >= 1)
size_t class_length(int n, int r) {
  const size_t step = PAGE * (size_t)n;
  size_t j = (TEAM_MIN - (size_t)r + step - 1) / step;
  if (j < 1) j = 1;
  return step * j + (size_t)r;
}

// up and down, with copies below the team's threshold (the caller's own memcpy) between the ones the team shares
std::vector<size_t> copy_lengths(int n, bool reduced) {
  const size_t MiB = (size_t)1 << 20;
  std::vector<size_t> cls;
  for (int r = 1; r < n; ++r) cls.push_back(class_length(n, r));
  std::vector<size_t> v;
  if (!reduced) v.push_back(16 * MiB + 8);
  v.push_back(0);
  v.push_back(MiB + 8);
  v.push_back(1);
  for (size_t k = 0; k < cls.size(); ++k) {
    v.push_back(cls[k]);
    if (k % 4 == 1) v.push_back(8);
  }
  if (!reduced) v.push_back(3 * MiB + 12345);
  v.push_back(MiB - 8);
  if (!reduced) v.push_back(8 * MiB);
  v.push_back(MiB);
  v.push_back(8);
  if (!reduced) v.push_back(16 * MiB + 8);
  for (size_t k = cls.size(); k-- > 0;) v.push_back(cls[k]);          // and the class once more, downwards, the team warm
  return v;
}

char *page_aligned(std::vector<char> &store, size_t bytes) {
  store.assign(bytes + PAGE, 0);
  const uintptr_t p = (uintptr_t)store.data();
  return (char *)((p + PAGE - 1) & ~(uintptr_t)(PAGE - 1));
}

int run_copies(int n, bool reduced) {
  const std::vector<size_t> lengths = copy_lengths(n, reduced);
  size_t maxlen = 0;
  for (size_t len : lengths) maxlen = std::max(maxlen, len);
  const size_t offs[] = {0, 1, 8};

  std::vector<char> pat(maxlen), cpat(maxlen);
  for (size_t i = 0; i < maxlen; ++i) { pat[i] = (char)pattern_byte(i); cpat[i] = (char)~pat[i]; }
  // one source per offset, written once; one destination arena: page | guard | up to 8 bytes | data | guard
  std::vector<char> src_store[3], dst_store;
  char *src_at[3];
  for (int k = 0; k < 3; ++k) {
    src_at[k] = page_aligned(src_store[k], maxlen + PAGE) + offs[k];
    if (maxlen) std::memcpy(src_at[k], pat.data(), maxlen);
  }
  char *dst_base = page_aligned(dst_store, GUARD + PAGE + maxlen + GUARD + PAGE);

  sd_xfer_team team(n);
  long cells = 0, failed = 0;
  for (size_t len : lengths)
    for (int so = 0; so < 3; ++so)
      for (int dof = 0; dof < 3; ++dof) {
        ++cells;
        const char *src = src_at[so];
        char *dst = dst_base + GUARD + offs[dof];
        std::memset(dst - GUARD, GUARD_BYTE, GUARD);
        if (len) std::memcpy(dst, cpat.data(), len);
        std::memset(dst + len, GUARD_BYTE, GUARD);
        team.copy(dst, src, len);
        size_t wrong = 0, first = 0, guard_hit = 0;
        if (len && std::memcmp(dst, pat.data(), len) != 0)
          for (size_t i = 0; i < len; ++i)
            if (dst[i] != pat[i]) { if (!wrong) first = i; ++wrong; }
        for (size_t i = 0; i < GUARD; ++i) guard_hit += ((unsigned char)dst[-(ptrdiff_t)GUARD + (ptrdiff_t)i] != GUARD_BYTE) + ((unsigned char)dst[len + i] != GUARD_BYTE);
        const bool src_changed = len && std::memcmp(src, pat.data(), len) != 0;
        if (wrong || guard_hit || src_changed) {
          ++failed;
          printf("FAIL copy n=%d bytes=%zu src+%zu dst+%zu: %zu bytes wrong, first at %zu of %zu; %zu guard bytes overwritten; source %s\n", n, len,
                 offs[so], offs[dof], wrong, first, len, guard_hit, src_changed ? "changed" : "intact");
        }
      }
  if (failed) printf("failed %ld of %ld\n", failed, cells);
  else printf("ok %ld\n", cells);
  return failed ? 1 : 0;
}

}  // namespace

int main(int argc, char **argv) {
  if (argc == 2 && !strcmp(argv[1], "bounds")) return check_all_bounds();
  if ((argc == 3 || (argc == 4 && !strcmp(argv[3], "reduced"))) && !strcmp(argv[1], "copy")) {
    const int n = atoi(argv[2]);
    if (n < 1 || n > 16) { fprintf(stderr, "n must be 1..16\n"); return 2; }
    return run_copies(n, argc == 4);
  }
  fprintf(stderr, "usage: %s bounds | copy n [reduced]\n", argv[0]);
  return 2;
}
