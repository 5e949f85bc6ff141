// Stand-alone host program for tests/test_orbit_key_host.py: prints the orbit key of csrc/orbit_key.hpp for every prefix.
//   orbit_key_host table <p> <quad_blocks> <cap_tenths>   -> one line "P rep member" per prefix P of p sites
//   orbit_key_host pairs <p> <FO>                         -> compares (quad_blocks 0, capacity FO bits) with the odd-pair rule
//                                                            the planner used before block orbits, for every P; prints "equal <n>"
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "orbit_key.hpp"

// the rule of odd-pair orbits as basis.cpp had it: the first FO flippable odd pairs are generators, set to (up, down)
static uint32_t pair_canon(uint32_t P, int p, int FO, int *member_out) {
  uint32_t C0 = P; int member = 0, ng = 0;
  for (int b = 1; b + 1 <= p && ng < FO; b += 2)
    if (((P >> (b - 1)) ^ (P >> b)) & 1u) {
      if (!((P >> (b - 1)) & 1u)) { C0 ^= 3u << (b - 1); member |= 1 << ng; }
      ++ng;
    }
  *member_out = member;
  return C0;
}

int main(int argc, char **argv) {
  if (argc == 5 && !strcmp(argv[1], "table")) {
    const int p = atoi(argv[2]), qb = atoi(argv[3]), cap = atoi(argv[4]);
    if (p < 1 || p > 24) return 2;
    for (uint32_t P = 0; P < (1u << p); ++P) {
      const sd_orbit_key o = sd_orbit_key_of(P, p, qb, cap);
      printf("%u %u %u\n", P, o.rep, o.member);
    }
    return 0;
  }
  if (argc == 4 && !strcmp(argv[1], "pairs")) {
    const int p = atoi(argv[2]), FO = atoi(argv[3]);
    if (p < 1 || p > 24) return 2;
    for (uint32_t P = 0; P < (1u << p); ++P) {
      int member = 0;
      const uint32_t C0 = pair_canon(P, p, FO, &member);
      const sd_orbit_key o = sd_orbit_key_of(P, p, 0, 10 * FO);
      if (o.rep != C0 || o.member != (uint32_t)member) {
        printf("differs at P=%u: (%u, %u) against (%u, %d)\n", P, o.rep, o.member, C0, member);
        return 1;
      }
    }
    printf("equal %u\n", 1u << p);
    return 0;
  }
  fprintf(stderr, "usage: %s table <p> <quad_blocks> <cap_tenths> | pairs <p> <FO>\n", argv[0]);
  return 2;
}
