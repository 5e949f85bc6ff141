// d(s) of a diagonal drive table, shared by kernels_drive.hip and kernels_hop_drive.hip: the sequential sum of the
// site terms +-W_i/2 and the bond terms +-V_b/4, each selected by bits of the configuration, never multiplied.  Device code only.
#pragma once
#include "gather_common.hpp"

namespace sd_dev {

// A term is +-w with the sign chosen by a bit of the configuration: a selection, written as the sign bit of w's high word so that it
// costs one shift, one xor and one bit-field insert per term instead of a compare and two conditional moves (same bits: the
// magnitude is untouched).  hi_of_bit: bit 31 = bit `at` of s.
__device__ __forceinline__ uint32_t hi_of_bit(uint64_t s, int at) { return (uint32_t)((s << (63 - at)) >> 32); }
__device__ __forceinline__ double with_sign(double w, uint32_t flip) {      // w with its sign flipped where bit 31 of `flip` is set
  const uint32_t hi = (uint32_t)__double2hiint(w);
  return __hiloint2double((int)((hi & 0x7fffffffu) | ((flip ^ hi) & 0x80000000u)), __double2loint(w));
}
// site i up: +w, down: -w
__device__ __forceinline__ double site_term(double w, uint64_t s, int i) { return with_sign(-w, hi_of_bit(s, i)); }
// parallel spins: +q, anti-parallel: -q
__device__ __forceinline__ double bond_term(double q, uint32_t bb, uint64_t s) {
  return with_sign(q, hi_of_bit(s, (int)(bb & 255u)) ^ hi_of_bit(s, (int)(bb >> 8)));
}
// The loops run four terms per trip so that the scalar loads of their weights are issued together and waited for once; the adds stay
// one after the other in list order.
__device__ __forceinline__ double drive_sites(const sd_drive_table &tb, uint64_t s, int from, int to, double d) {
  int i = from;
  for (; i + 4 <= to; i += 4) {
    const double w0 = tb.wh[i], w1 = tb.wh[i + 1], w2 = tb.wh[i + 2], w3 = tb.wh[i + 3];
    d += site_term(w0, s, i); d += site_term(w1, s, i + 1); d += site_term(w2, s, i + 2); d += site_term(w3, s, i + 3);
  }
  for (; i < to; ++i) d += site_term(tb.wh[i], s, i);
  return d;
}
__device__ __forceinline__ double drive_bonds(const sd_drive_table &tb, uint64_t s, int from, int to, double d) {
  int b = from;
  for (; b + 4 <= to; b += 4) {
    const double q0 = tb.vq[b], q1 = tb.vq[b + 1], q2 = tb.vq[b + 2], q3 = tb.vq[b + 3];
    const uint32_t b0 = tb.bits[b], b1 = tb.bits[b + 1], b2 = tb.bits[b + 2], b3 = tb.bits[b + 3];
    d += bond_term(q0, b0, s); d += bond_term(q1, b1, s); d += bond_term(q2, b2, s); d += bond_term(q3, b3, s);
  }
  for (; b < to; ++b) d += bond_term(tb.vq[b], tb.bits[b], s);
  return d;
}

}  // namespace sd_dev
