// Entanglement across a chain cut, host side: the block layout of the reduced density matrix, the segment tables and
// the flat work list of k_cut_gram.  Nothing here touches the device, so all of it is checked on the CPU (tests/test_cut_plan_host.py).
//
// Layout.  The basis order is a binary tree over the sites 1, 2, ..., L (sd_internal.hpp), so the rows that share the configuration
// P of sites 1..k are one contiguous run -- a SEGMENT -- that starts at rank(P | lowest suffix) and is ordered like the sector
// (L - k, nup - popcount(P)).  The segments of one m = popcount(P) therefore have one length dB(m) and one internal order, and psi is
// the matrix Psi_m[a, j] = psi[start_m[a] + j] as it stands.  In the full basis the row is the configuration and the segments are the
// runs of one suffix value j: start j 2^k, length 2^k.
//
// Forms.  A Gram matrix over the segments (side A of a sector, side B of the full basis) sums INSIDE a segment: form ACROSS, the
// summation index is the contiguous one.  A Gram matrix over the positions inside a segment (side B of a sector, side A of the full
// basis) sums OVER the segments: form INSIDE, the Gram index is the contiguous one.
//
// Work list.  Per block the upper triangle of tile x tile output tiles; the summation range [0, K) of every tile pair of the block
// cut into ns contiguous pieces, each a multiple of SD_CUT_KC except the last.  With P tile pairs in all blocks together and P <
// SD_CUT_TARGET_ITEMS, want = ceil(TARGET / P) pieces per pair are asked for; a block gives piece = KC ceil(ceil(K / want) / KC) and
// ns = ceil(K / piece), so K is never cut below KC.  Every item owns tile x tile elements of the workspace; the pieces of a pair are
// consecutive there and in the list, and k_cut_reduce adds them in that order.
#include <algorithm>
#include <string>
#include <vector>

#include "sd_internal.hpp"

namespace {
int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }
}  // namespace

int sd_cut_layout(const sd_model *m, int cut, int side, std::vector<sd_cut_blk> &blks, int64_t *n_out, std::string &err) {
  blks.clear();
  if (side != SD_CUT_A && side != SD_CUT_B && side != SD_CUT_AUTO) { err = "side must be SD_CUT_A, SD_CUT_B or SD_CUT_AUTO"; return SD_EARG; }
  if (m->L < 2 || m->L > SD_MAX_L || cut < 1 || cut > m->L - 1) { err = "the cut must be in 1..L-1"; return SD_EARG; }
  if (m->nranks != 1) { err = "entanglement needs an unsharded model"; return SD_EARG; }
  const int L = m->L, k = cut;
  const bool full = m->nup < 0;
  const int m_lo = full ? -1 : std::max(0, m->nup - (L - k)), m_hi = full ? -1 : std::min(k, m->nup);
  int64_t off = 0;
  for (int mm = m_lo; mm <= m_hi; ++mm) {
    sd_cut_blk b{};
    b.m = mm;
    b.dA = full ? (int64_t)1 << k : sd_binom(k, mm);
    b.dB = full ? (int64_t)1 << (L - k) : sd_binom(L - k, m->nup - mm);
    b.side = side == SD_CUT_AUTO ? (b.dA <= b.dB ? SD_CUT_A : SD_CUT_B) : side;
    // segments: prefixes in a sector (dA of them, dB rows each), suffix values in the full basis (dB of them, dA rows each)
    b.nseg = full ? b.dB : b.dA;
    b.seglen = full ? b.dA : b.dB;
    const bool over_segments = full ? b.side == SD_CUT_B : b.side == SD_CUT_A;
    b.form = over_segments ? SD_CUT_ACROSS : SD_CUT_INSIDE;
    b.d = over_segments ? b.nseg : b.seglen;
    b.K = over_segments ? b.seglen : b.nseg;
    if (b.d > SD_CUT_MAX_DIM) { err = "a block of the reduced density matrix is larger than SD_CUT_MAX_DIM: take the other side"; return SD_EARG; }
    b.tile = b.d <= SD_CUT_SMALL_TILE ? SD_CUT_SMALL_TILE : SD_CUT_TILE;
    b.out_off = off;
    b.seg_off = 0;
    off += b.d * b.d;
    blks.push_back(b);
  }
  if (n_out) *n_out = off;
  return SD_OK;
}

void sd_cut_fill_segments(const sd_model *m, int cut, const sd_cut_blk &b, std::vector<int64_t> &segs) {
  const size_t first = segs.size();
  segs.reserve(first + (size_t)b.nseg);
  if (m->nup < 0) {
    for (int64_t j = 0; j < b.nseg; ++j) segs.push_back(j << cut);
    return;
  }
  // the prefixes of popcount mm in the order of the tree (sorted site lists, lexicographic), each with the lowest suffix of its run:
  // the nup - mm ups on the first sites after the cut
  const int mm = b.m, t = m->nup - mm;
  const uint64_t low_suffix = (t > 0 ? (~(uint64_t)0 >> (64 - t)) : (uint64_t)0) << cut;
  std::vector<int> c((size_t)mm);
  for (int i = 0; i < mm; ++i) c[(size_t)i] = i;              // 0-based bits
  for (;;) {
    uint64_t P = 0;
    for (int i = 0; i < mm; ++i) P |= (uint64_t)1 << c[(size_t)i];
    segs.push_back(sd_rank_host(m, P | low_suffix));
    int i = mm - 1;
    while (i >= 0 && c[(size_t)i] == cut - mm + i) --i;
    if (i < 0) break;
    ++c[(size_t)i];
    for (int q = i + 1; q < mm; ++q) c[(size_t)q] = c[(size_t)q - 1] + 1;
  }
  if (!std::is_sorted(segs.begin() + (ptrdiff_t)first, segs.end())) std::sort(segs.begin() + (ptrdiff_t)first, segs.end());
}

int sd_cut_build_plan(const sd_model *m, int cut, int side, bool with_segs, sd_cut_plan &plan, std::string &err) {
  plan = sd_cut_plan();
  const int rc = sd_cut_layout(m, cut, side, plan.blks, &plan.n_out, err);
  if (rc) return rc;
  if (with_segs)
    for (sd_cut_blk &b : plan.blks) {
      b.seg_off = (int64_t)plan.segs.size();
      sd_cut_fill_segments(m, cut, b, plan.segs);
    }
  int64_t n_pairs = 0;
  for (const sd_cut_blk &b : plan.blks) {
    const int64_t T = ceil_div(b.d, b.tile);
    n_pairs += T * (T + 1) / 2;
  }
  const int64_t want = n_pairs > 0 && n_pairs < SD_CUT_TARGET_ITEMS ? ceil_div(SD_CUT_TARGET_ITEMS, n_pairs) : 1;
  int64_t slot = 0;
  for (int cls = 0; cls < 4; ++cls) {
    plan.class_first[cls] = (int64_t)plan.items.size();
    for (size_t bi = 0; bi < plan.blks.size(); ++bi) {
      const sd_cut_blk &b = plan.blks[bi];
      if (b.form * 2 + (b.tile == SD_CUT_TILE ? 1 : 0) != cls) continue;
      const int64_t piece = std::max<int64_t>(SD_CUT_KC, SD_CUT_KC * ceil_div(ceil_div(b.K, want), SD_CUT_KC));
      const int ns = (int)std::max<int64_t>(1, ceil_div(b.K, piece));
      plan.max_ns = std::max(plan.max_ns, ns);
      const int T = (int)ceil_div(b.d, b.tile);
      const int64_t tt = (int64_t)b.tile * b.tile;
      for (int ti = 0; ti < T; ++ti)
        for (int tj = ti; tj < T; ++tj) {
          plan.pairs.push_back(sd_cut_pair{(int32_t)bi, ti, tj, ns, slot});
          for (int s = 0; s < ns; ++s) {
            sd_cut_item it{};
            it.block = (int32_t)bi; it.ti = ti; it.tj = tj; it.tile = b.tile; it.form = b.form; it.piece = s; it.ns = ns;
            it.k0 = (int64_t)s * piece;
            it.k1 = std::min<int64_t>(b.K, it.k0 + piece);
            it.slot = slot;
            slot += tt;
            plan.items.push_back(it);
          }
        }
    }
  }
  plan.class_first[4] = (int64_t)plan.items.size();
  plan.ws_elems = slot;
  return SD_OK;
}
