// The counter-based N(0,1) stream of libspindyn in a form that gives the SAME BITS on the host and on the device.
// Element k of stream `seed` = Box-Muller on two uniforms hashed from (seed, k), as sd_randn_at (device_common.hpp), but with the
// logarithm and the cosine written out in IEEE operations (+, -, *, /, sqrt; the library is built with -ffp-contract=off) instead of
// the C library's and the device math library's own log and cos, which differ from each other in the last bit for about 4 % of
// the arguments.  sd_fill_randn_host (include/spindyn.h) promises the vector sd_fill_randn_dev fills; with this form it is that
// vector bit for bit (tests/test_gpu_recursion_grids.py).  Accuracy: about 1.5 ulp for both functions on the arguments that occur.
#pragma once
#include "device_common.hpp"

namespace sd_dev {

// The counter-based uniform of the projective snapshots (kernels_basis_stats.hip), hashed like the normal stream's uniforms with
// sd_mix64: u_k in [0, 1) = the top 53 bits of the hash times 2^-53, both exact in IEEE arithmetic, so host and device agree to
// the bit.  The salt keeps the stream apart from the normal stream of the same seed.
#define SD_SAMPLE_SALT 0x5AD5B1A5C0F1E2D3ULL
__host__ __device__ inline double sd_sample_uniform(uint64_t seed, uint64_t k) {
  return (double)(sd_mix64((seed ^ SD_SAMPLE_SALT) ^ sd_mix64(k)) >> 11) * (1.0 / 9007199254740992.0);
}

__host__ __device__ inline uint64_t sd_f64_bits(double d) { uint64_t b; __builtin_memcpy(&b, &d, sizeof b); return b; }
__host__ __device__ inline double sd_bits_f64(uint64_t b) { double d; __builtin_memcpy(&d, &b, sizeof d); return d; }

// log x for a positive normal x: x = m 2^e with m in [sqrt(1/2), sqrt(2)), log m = 2 atanh(s), s = (m - 1) / (m + 1), |s| < 0.1716
__host__ __device__ inline double sd_log_pos(double x) {
  const uint64_t b = sd_f64_bits(x);
  int e = (int)(b >> 52) - 1022;
  double m = sd_bits_f64((b & 0x000FFFFFFFFFFFFFULL) | 0x3FE0000000000000ULL);      // [0.5, 1)
  if (m < 0.70710678118654752440) { m = m * 2.0; e -= 1; }
  const double s = (m - 1.0) / (m + 1.0), z = s * s;                                // m - 1 is exact
  double p = 1.0 / 27.0;                                                            // z^13 / 27 < 1e-21
  p = 1.0 / 25.0 + z * p;
  p = 1.0 / 23.0 + z * p;
  p = 1.0 / 21.0 + z * p;
  p = 1.0 / 19.0 + z * p;
  p = 1.0 / 17.0 + z * p;
  p = 1.0 / 15.0 + z * p;
  p = 1.0 / 13.0 + z * p;
  p = 1.0 / 11.0 + z * p;
  p = 1.0 / 9.0 + z * p;
  p = 1.0 / 7.0 + z * p;
  p = 1.0 / 5.0 + z * p;
  p = 1.0 / 3.0 + z * p;
  const double lm = 2.0 * s + 2.0 * s * (z * p);                                    // 2 s (1 + z p)
  const double ln2_hi = 6.93147180369123816490e-01, ln2_lo = 1.90821492927058770002e-10;   // ln2_hi: 32 significant bits, e ln2_hi exact
  const double de = (double)e;
  return de * ln2_hi + (lm + de * ln2_lo);
}

// cos(2 pi u) for 0 <= u < 1: the quadrant and the remainder of 4 u are exact; Taylor series on |y| <= pi / 4
__host__ __device__ inline double sd_cos_2pi(double u) {
  const double t = 4.0 * u;
  int q = (int)t;
  double r = t - (double)q;                                                         // exact, [0, 1)
  if (r > 0.5) { r = r - 1.0; q += 1; }                                             // exact, [-0.5, 0.5]
  const double y = r * 1.57079632679489661923, w = y * y;
  if (q & 1) {                                                                      // -+ sin y
    double p = -1.0 / 121645100408832000.0;                                         // 19!
    p = 1.0 / 355687428096000.0 + w * p;                                            // 17!
    p = -1.0 / 1307674368000.0 + w * p;                                             // 15!
    p = 1.0 / 6227020800.0 + w * p;                                                 // 13!
    p = -1.0 / 39916800.0 + w * p;                                                  // 11!
    p = 1.0 / 362880.0 + w * p;                                                     // 9!
    p = -1.0 / 5040.0 + w * p;
    p = 1.0 / 120.0 + w * p;
    p = -1.0 / 6.0 + w * p;
    const double sn = y + y * (w * p);
    return (q & 2) ? sn : -sn;                                                      // q = 1: -sin y; q = 3: sin y
  }
  double p = 1.0 / 2432902008176640000.0;                                           // 20!
  p = -1.0 / 6402373705728000.0 + w * p;                                            // 18!
  p = 1.0 / 20922789888000.0 + w * p;                                               // 16!
  p = -1.0 / 87178291200.0 + w * p;                                                 // 14!
  p = 1.0 / 479001600.0 + w * p;                                                    // 12!
  p = -1.0 / 3628800.0 + w * p;                                                     // 10!
  p = 1.0 / 40320.0 + w * p;
  p = -1.0 / 720.0 + w * p;
  p = 1.0 / 24.0 + w * p;
  p = -0.5 + w * p;
  const double cs = 1.0 + w * p;
  return (q & 2) ? -cs : cs;                                                        // q = 0, 4: cos y; q = 2: -cos y
}

__host__ __device__ inline double sd_randn(uint64_t seed, uint64_t k) {
  const uint64_t h1 = sd_mix64(seed ^ sd_mix64(2 * k)), h2 = sd_mix64(seed ^ sd_mix64(2 * k + 1));
  const double u1 = ((double)(h1 >> 11) + 0.5) * (1.0 / 9007199254740992.0);        // (0, 1]: 1 when h1 >> 11 = 2^53 - 1 (log 1 = 0)
  const double u2 = ((double)(h2 >> 11) + 0.5) * (1.0 / 9007199254740992.0);
  return sqrt(-2.0 * sd_log_pos(u1)) * sd_cos_2pi(u2);
}

}  // namespace sd_dev
