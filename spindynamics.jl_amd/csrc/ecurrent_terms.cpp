// The energy current of a model as a list of dressed bond currents (host only).
// H = sum_a h_a with hops t (S^+_i S^-_j + h.c.), zz terms v S^z_i S^z_j and field terms B_i S^z_i.  A bond (i, j) sits at
// x = i + delta / 2, delta = j - i, a field term at x = i; with `periodic`, delta and every position difference are minimum images
// on a ring of L sites.  J_E = (i/2) sum_{a,b} d(a, b) [h_a, h_b], d(a, b) = x_b - x_a; only pairs sharing exactly one site contribute:
//   hop (p, m) with hop (m, q): i [F_pm, F_mq] = -2 S^z_m j'_pq   -> (p, q, m, -2 t_a t_b d(a, b)), each unordered pair once
//   hop (p, m) with zz (m, q) : i [F_pm, Z_mq] = j'_pm S^z_q      -> (p, m, q, t_a v_b d(a, b))
//   hop (i, j) with the fields of its two sites                   -> (i, j, 0, 1/2 (B_i + B_j) delta t)
// with j'_ij = i (S^+_i S^-_j - S^-_i S^+_j).  Terms of equal (i, j, k) are merged after orienting each to i < j (swapping i and j
// flips the sign), exact zeros dropped, the list sorted by (i, j, k).
#include <cmath>
#include <map>
#include <tuple>

#include "sd_internal.hpp"

namespace {

struct Ambiguous {};

// d, or on a ring its representative in (-L/2, L/2); exactly +-L/2 has two
double min_image(double d, int L, int periodic) {
  if (!periodic) return d;
  d = d - L * std::floor(d / L + 0.5);
  if (2.0 * std::fabs(d) == (double)L) throw Ambiguous{};
  return d;
}
double bond_delta(int i, int j, int L, int periodic) { return min_image((double)(j - i), L, periodic); }
double bond_x(int i, int j, int L, int periodic) { return i + bond_delta(i, j, L, periodic) / 2; }

struct Bond { int i, j; double c; };

// the one site two bonds share (0: none, or both)
int shared_site(const Bond &a, const Bond &b) {
  const bool ii = a.i == b.i, ij = a.i == b.j, ji = a.j == b.i, jj = a.j == b.j;
  if ((int)ii + (int)ij + (int)ji + (int)jj != 1) return 0;
  return (ii || ij) ? a.i : a.j;
}

}  // namespace

int sd_build_energy_current(const sd_model *m, int periodic, std::vector<sd_dterm> &out, std::string &err) {
  const int L = m->L;
  std::vector<Bond> hop, zz;
  for (size_t b = 0; b < m->hop_J.size(); ++b)
    if (m->hop_i[b] != m->hop_j[b]) hop.push_back({m->hop_i[b], m->hop_j[b], m->hop_J[b]});
  for (size_t b = 0; b < m->zz_J.size(); ++b)
    if (m->zz_i[b] != m->zz_j[b]) zz.push_back({m->zz_i[b], m->zz_j[b], m->zz_J[b]});
  std::map<std::tuple<int, int, int>, double> acc;
  auto add = [&](int i, int j, int k, double c) {
    if (i > j) { std::swap(i, j); c = -c; }
    acc[std::make_tuple(i, j, k)] += c;
  };
  try {
    for (size_t a = 0; a < hop.size(); ++a)
      for (size_t b = a + 1; b < hop.size(); ++b) {
        const int s = shared_site(hop[a], hop[b]);
        if (!s) continue;
        const int p = hop[a].j == s ? hop[a].i : hop[a].j, q = hop[b].j == s ? hop[b].i : hop[b].j;
        const double d = min_image(bond_x(hop[b].i, hop[b].j, L, periodic) - bond_x(hop[a].i, hop[a].j, L, periodic), L, periodic);
        add(p, q, s, -2.0 * hop[a].c * hop[b].c * d);
      }
    for (const Bond &a : hop)
      for (const Bond &b : zz) {
        const int s = shared_site(a, b);
        if (!s) continue;
        const int p = a.j == s ? a.i : a.j, q = b.j == s ? b.i : b.j;
        const double d = min_image(bond_x(b.i, b.j, L, periodic) - bond_x(a.i, a.j, L, periodic), L, periodic);
        add(p, s, q, a.c * b.c * d);
      }
    for (const Bond &a : hop) {
      const double bsum = m->field[(size_t)a.i - 1] + m->field[(size_t)a.j - 1];
      if (bsum != 0.0) add(a.i, a.j, 0, 0.5 * bsum * bond_delta(a.i, a.j, L, periodic) * a.c);
    }
  } catch (const Ambiguous &) {
    err = "a position difference of exactly +-L/2 on the ring has no minimum image";
    return SD_EARG;
  }
  out.clear();
  for (const auto &kv : acc) {
    if (kv.second == 0.0) continue;
    sd_dterm t;
    t.i = std::get<0>(kv.first); t.j = std::get<1>(kv.first); t.k = std::get<2>(kv.first); t.c = kv.second;
    out.push_back(t);
  }
  if (out.size() > (size_t)SD_DTERM_MAX) {
    err = "the energy current has more than SD_DTERM_MAX terms";
    return SD_EARG;
  }
  return SD_OK;
}
