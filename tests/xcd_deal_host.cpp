// Stand-alone host program for tests/test_xcd_deal_host.py: deals the orbits of a small sector with csrc/xcd_deal.hpp.
//   xcd_deal_host <p> <LS> <nup> <quad_blocks> <cap_tenths> <cost> <run> [<mix_a> <w_a> <mix_b> <w_b>]
// Tiles: every prefix P of p sites whose suffix filling nup - popcount(P) lies in 0..LS, by ascending base row (site 1 most
// significant, up first: the order in which sd_build_plan hands them to xcd_queues); orbits numbered by first appearance.
// -> one line "o tiles rows slots req_bytes out_bytes queue" per orbit, in sequence order.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <vector>

#include "xcd_deal.hpp"

static int64_t binom(int n, int k) {
  if (k < 0 || n < 0 || k > n) return 0;
  int64_t r = 1;
  for (int i = 1; i <= k; ++i) r = r * (n - k + i) / i;
  return r;
}

int main(int argc, char **argv) {
  if (argc != 8 && argc != 12) return 2;
  const int p = atoi(argv[1]), LS = atoi(argv[2]), nup = atoi(argv[3]), qb = atoi(argv[4]), cap = atoi(argv[5]);
  sd_deal_rule rule = {atoi(argv[6]), SD_DEAL_ROWS, SD_DEAL_ROWS, 0, 0, atoi(argv[7])};
  if (argc == 12) { rule.mix_a = atoi(argv[8]); rule.w_a = atoll(argv[9]); rule.mix_b = atoi(argv[10]); rule.w_b = atoll(argv[11]); }
  if (p < 2 || p > 20 || LS < 1 || LS > 12) return 2;
  std::vector<std::pair<uint32_t, uint32_t>> tiles;            // (order key, P)
  for (uint32_t P = 0; P < (1u << p); ++P) {
    const int t = nup - __builtin_popcount(P);
    if (t < 0 || t > LS) continue;
    uint32_t key = 0;
    for (int k = 1; k <= p; ++k) key |= (1u - ((P >> (k - 1)) & 1u)) << (p - k);
    tiles.push_back({key, P});
  }
  std::sort(tiles.begin(), tiles.end());
  std::map<uint32_t, size_t> first_seen;
  std::vector<sd_deal_orbit> orb;
  for (const auto &kp : tiles) {
    const uint32_t P = kp.second;
    const uint32_t rep = sd_orbit_key_of(P, p, qb, cap).rep;
    auto it = first_seen.find(rep);
    if (it == first_seen.end()) { it = first_seen.insert({rep, orb.size()}).first; orb.push_back(sd_deal_orbit{0, 0, 0, 0, 0}); }
    const int t = nup - __builtin_popcount(P);
    sd_deal_add_tile(orb[it->second], P, p, binom(LS, t), ((P >> (p - 1)) & 1u) ? binom(LS - 1, t) : binom(LS - 1, t - 1), qb, cap, true);
  }
  std::vector<uint8_t> q(orb.size());
  sd_xcd_deal(orb.data(), orb.size(), rule, q.data());
  for (size_t o = 0; o < orb.size(); ++o)
    printf("%zu %lld %lld %lld %lld %lld %d\n", o, (long long)orb[o].tiles, (long long)orb[o].rows, (long long)orb[o].slots,
           (long long)orb[o].req_bytes, (long long)orb[o].out_bytes, (int)q[o]);
  return 0;
}
