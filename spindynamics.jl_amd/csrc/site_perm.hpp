// Source map of a site permutation.  pi is given as perm[0..L-1], perm[i] the 1-based site to which the spin of site
// i + 1 moves; U_pi |s> = |pi s>, so (U_pi psi)[idx(s)] = psi[idx(src(s))] with
//     bit i of src(s) = bit (perm[i] - 1) of s.
// src is linear over OR, so it is the OR of one table read per byte of s: table entry (base, v) holds the source bits of the eight
// configuration bits base .. base + 7 taking the value v.  A pure function of its arguments: capi.cpp builds the ceil(L / 8) tables of
// the whole configuration on the host (sd_site_permute_sources), kernels_permute.hip builds its tables per workgroup in LDS from the
// permutation passed by value -- the same code, so the host accessor proves the device's table.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define SD_PERM_HD __host__ __device__
#else
#define SD_PERM_HD
#endif

#define SD_PERM_MAX_SITES 64
#define SD_PERM_MAX_TABLES 8       // ceil(63 / 8); 8 x 256 x 8 bytes = 16 KiB

struct sd_site_perm { uint8_t to[SD_PERM_MAX_SITES]; };   // to[i] = perm[i] - 1, i < L: the 0-based bit the spin of bit i moves to

// perm (1-based, L entries) -> pm when it is a bijection of 1..L (returns 1), else 0; *identity: perm[i] == i + 1 throughout
static inline int sd_site_perm_make(const int *perm, int L, sd_site_perm *pm, int *identity) {
  if (L < 1 || L >= SD_PERM_MAX_SITES) return 0;
  uint64_t seen = 0;
  int id = 1;
  for (int i = 0; i < SD_PERM_MAX_SITES; ++i) pm->to[i] = 0;
  for (int i = 0; i < L; ++i) {
    const int t = perm[i];
    if (t < 1 || t > L || ((seen >> (t - 1)) & 1)) return 0;
    seen |= (uint64_t)1 << (t - 1);
    pm->to[i] = (uint8_t)(t - 1);
    if (t != i + 1) id = 0;
  }
  if (identity) *identity = id;
  return 1;
}

// the source bits of the configuration bits base .. base + 7 taking the value v (0 .. 255)
SD_PERM_HD static inline uint64_t sd_site_perm_entry(const sd_site_perm &pm, int L, int base, int v) {
  uint64_t r = 0;
  for (int i = 0; i < L; ++i) {
    const int j = (int)pm.to[i] - base;
    if (j >= 0 && j < 8 && ((v >> j) & 1)) r |= (uint64_t)1 << i;
  }
  return r;
}

// lut[256 b + v], b < ntab: the table of the bits base + 8 b .. base + 8 b + 7.  Entries first, first + step, ... are written, so a
// workgroup of `step` threads fills a table set with one call per thread (the host: first = 0, step = 1).
SD_PERM_HD static inline void sd_site_perm_fill(uint64_t *lut, const sd_site_perm &pm, int L, int base, int ntab, int first, int step) {
  for (int e = first; e < 256 * ntab; e += step) lut[e] = sd_site_perm_entry(pm, L, base + 8 * (e >> 8), e & 255);
}

// OR of the ntab table reads for the bits of t (t = the configuration shifted down by the tables' base)
SD_PERM_HD static inline uint64_t sd_site_perm_source(const uint64_t *lut, int ntab, uint64_t t) {
  uint64_t r = 0;
  for (int b = 0; b < ntab; ++b) r |= lut[256 * b + (int)((t >> (8 * b)) & 255)];
  return r;
}
