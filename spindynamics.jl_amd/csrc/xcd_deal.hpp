// Dealing of whole orbits to the eight XCD queues (basis.cpp, xcd_queues): a pure function from the orbit list, in sequence
// order, to a queue index per orbit.  basis.cpp and the stand-alone host test (tests/xcd_deal_host.cpp) include it;
// profiles/orbit_key.py restates it in Python for the L2 model.
//
// An orbit goes to the queue whose cost so far is lowest, ties to the lowest queue index (least-loaded dealing: the queues never
// end further apart than the largest single orbit's cost), or round-robin (orbit o -> queue o % 8).  With run > 1 the unit that
// is dealt is a run of that many consecutive orbits (the last run may be shorter).  The cost is the clock by
// which the queues are kept at the same place of the orbit sequence; all of them are computable on the host:
//   rows       rows of the orbit's tiles;
//   slots      256-row wave slots its tiles take in the packed launch (ceil(len / 256) each; four slots are a workgroup);
//   req bytes  what its tiles ask the memory system for: 16 bytes for every own row read, every row of a partner tile across a
//              flippable prefix bond (same filling, same length), every partner row of the straddling bond (the tile's rows
//              whose first suffix site can hop: about half a partner), and every row written;
//   out bytes  req bytes minus the partner tiles that are members of the same orbit (read back to back on one XCD: L2 hits);
//   mix        w_a * cost_a + w_b * cost_b of two of the above, integer weights.
#pragma once
#include <cstddef>
#include <cstdint>
#include "orbit_key.hpp"

enum sd_deal_cost { SD_DEAL_ROUND_ROBIN = 0, SD_DEAL_ROWS = 1, SD_DEAL_SLOTS = 2, SD_DEAL_REQ_BYTES = 3, SD_DEAL_OUT_BYTES = 4, SD_DEAL_MIX = 5 };

struct sd_deal_orbit { int64_t tiles, rows, slots, req_bytes, out_bytes; };
struct sd_deal_rule { int cost, mix_a, mix_b; int64_t w_a, w_b; int run; };      // mix_a, mix_b: SD_DEAL_ROWS .. SD_DEAL_OUT_BYTES; run >= 1

static inline bool sd_deal_needs_bytes(const sd_deal_rule &r) {
  return r.cost == SD_DEAL_REQ_BYTES || r.cost == SD_DEAL_OUT_BYTES ||
         (r.cost == SD_DEAL_MIX && (r.mix_a >= SD_DEAL_REQ_BYTES || r.mix_b >= SD_DEAL_REQ_BYTES));
}

// Adds tile P (prefix of p sites, len rows, straddle_rows of them with a hop across the bond (p, p+1)) to its orbit's entry.
// with_bytes = false leaves the two byte costs alone (they cost an orbit key per flippable bond).
static inline void sd_deal_add_tile(sd_deal_orbit &o, uint32_t P, int p, int64_t len, int64_t straddle_rows, int quad_blocks,
                                    int cap_tenths, bool with_bytes) {
  o.tiles += 1;
  o.rows += len;
  o.slots += (len + 255) / 256;
  if (!with_bytes) return;
  const uint32_t rep = sd_orbit_key_of(P, p, quad_blocks, cap_tenths).rep;
  int64_t partners = 0, inside = 0;
  for (int b = 1; b <= p - 1; ++b) {
    if (!((((P >> (b - 1)) ^ (P >> b)) & 1u))) continue;
    ++partners;
    if (sd_orbit_key_of(P ^ (3u << (b - 1)), p, quad_blocks, cap_tenths).rep == rep) ++inside;
  }
  const int64_t req = 16 * ((2 + partners) * len + straddle_rows);
  o.req_bytes += req;
  o.out_bytes += req - 16 * inside * len;
}

static inline int64_t sd_deal_cost_of(const sd_deal_orbit &o, int cost) {
  return cost == SD_DEAL_ROWS ? o.rows : cost == SD_DEAL_SLOTS ? o.slots : cost == SD_DEAL_REQ_BYTES ? o.req_bytes
       : cost == SD_DEAL_OUT_BYTES ? o.out_bytes : 0;
}

static inline int64_t sd_deal_cost_of(const sd_deal_orbit &o, const sd_deal_rule &r) {
  if (r.cost == SD_DEAL_MIX) return r.w_a * sd_deal_cost_of(o, r.mix_a) + r.w_b * sd_deal_cost_of(o, r.mix_b);
  return sd_deal_cost_of(o, r.cost);
}

// queue_out[o] = queue (0..7) of orbit o, o = 0 .. n-1 in sequence order
static inline void sd_xcd_deal(const sd_deal_orbit *orb, size_t n, const sd_deal_rule &rule, uint8_t *queue_out) {
  int64_t q_cost[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  const size_t run = rule.run > 1 ? (size_t)rule.run : 1;
  size_t x = 0;
  for (size_t o = 0; o < n; ++o) {
    if (o % run == 0) {                                          // a new run: choose its queue
      x = (o / run) % 8;
      if (rule.cost != SD_DEAL_ROUND_ROBIN) {
        x = 0;
        for (size_t y = 1; y < 8; ++y) if (q_cost[y] < q_cost[x]) x = y;
      }
    }
    q_cost[x] += sd_deal_cost_of(orb[o], rule);
    queue_out[o] = (uint8_t)x;
  }
}
