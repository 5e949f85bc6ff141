// Orbit key of a tile for the XCD-aware processing order (basis.cpp, xcd_queues): which orbit a prefix configuration P of
// sites 1..p belongs to (its representative) and its place inside that orbit (member id).  A pure function of its arguments:
// basis.cpp and the stand-alone host test (tests/orbit_key_host.cpp) include it; profiles/l2_model.py restates it in Python.
//
// An orbit collects tiles that read each other through far bonds, so that they can be queued back to back on one XCD.  Its
// size is bounded by a capacity of cap_tenths / 10 bits.  The prefix is walked from site 1:
//   * four-site block j = sites 4j+1 .. 4j+4, j < quad_blocks, wholly in the prefix, with k up spins and c = C(4,k) > 1
//     configurations: if log2(c) still fits the capacity the block is QUAD-ACTIVE -- the orbit holds every configuration of
//     the block with k up spins (all three bonds inside the block close within the orbit), the representative has the k
//     lowest sites up, and the member id takes the configuration's index (ascending as an integer) as a digit of radix c;
//   * otherwise the block's two pairs (4j+1,4j+2), (4j+3,4j+4), like every pair of the later blocks and of the sites left
//     over after the last whole block, are odd pairs: a flippable pair is a generator if one more bit fits the capacity; the
//     representative has it (up, down), the member digit (radix 2) says whether it is flipped.
// Every decision depends only on what no move of the orbit changes (the filling of a quad-active block, the two pair fillings
// of the others, the capacity used so far), so all members of an orbit compute the same representative and the same radices:
// member ids are distinct within an orbit and below 2^(cap_tenths / 10).  All moves keep the filling of the prefix, hence the
// tile length.  quad_blocks = 0, cap_tenths = 10 * FO is the rule of odd-pair orbits with at most FO generators.
// Capacities are counted in thousandths of a bit, rounded up (log2 6 = 2.585), so the bound on the orbit size is never exceeded.
#pragma once
#include <cstdint>

struct sd_orbit_key { uint32_t rep, member; };

static inline sd_orbit_key sd_orbit_key_of(uint32_t P, int p, int quad_blocks, int cap_tenths) {
  static const int quad_count[5] = {1, 4, 6, 4, 1}, quad_mbits[5] = {0, 2000, 2585, 2000, 0};
  const int cap = 100 * cap_tenths;
  sd_orbit_key o = {P, 0};
  uint32_t mult = 1;
  int used = 0;
  for (int b = 1; b + 1 <= p;) {
    if (b % 4 == 1 && (b - 1) / 4 < quad_blocks && b + 3 <= p) {
      const uint32_t cfg = (P >> (b - 1)) & 15u;
      const int k = __builtin_popcount(cfg);
      if (quad_count[k] > 1 && used + quad_mbits[k] <= cap) {
        uint32_t digit = 0;                                     // configurations with k up spins below cfg
        for (uint32_t c = 0; c < cfg; ++c) digit += __builtin_popcount(c) == k;
        o.rep = (o.rep & ~(15u << (b - 1))) | (((1u << k) - 1u) << (b - 1));
        o.member += digit * mult; mult *= (uint32_t)quad_count[k];
        used += quad_mbits[k];
        b += 4;
        continue;
      }
    }
    if ((((P >> (b - 1)) ^ (P >> b)) & 1u) && used + 1000 <= cap) {
      if (!((P >> (b - 1)) & 1u)) { o.rep ^= 3u << (b - 1); o.member += mult; }
      mult *= 2; used += 1000;
    }
    b += 2;
  }
  return o;
}
