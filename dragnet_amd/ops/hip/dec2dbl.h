// Correctly rounded decimal -> binary64 for the scan kernels.
//
// dn_dec2dbl(mant, exp10, tbl) returns the double nearest to
// mant * 10^exp10 (ties to even), for any 64-bit mant — i.e. every
// literal of <= 19 significant digits parses exactly as strtod / V8 do.
//
//   fast path   mant < 2^53 and |exp10| <= 22: both operands are exact
//               doubles, so one IEEE multiply/divide is one rounding
//               (Clinger).  Inlined; all integer-valued data stays here.
//   slow path   Eisel-Lemire (D. Lemire, "Number parsing at a gigabyte
//               per second", SPE 2021): one or two 64x64->128 products
//               against a 128-bit power of five.  For a 64-bit mantissa
//               the algorithm has NO indeterminate case (Mushtak &
//               Lemire, "Fast number parsing without fallback", SPE
//               2023), so there is nothing to fall back to or to count.
//               Out of line: the scan kernel is register-limited.
//
// Callers keep the first 19 significant digits in mant and fold the
// count of dropped integer digits into exp10.  A literal with more
// digits therefore converts as its 19-digit truncation: exact whenever
// mant and mant+1 round to the same double, otherwise possibly one ulp
// low (the one documented divergence, COMPONENTS.md).
//
// Host-compilable (plain C++17) so the routine can be unit-checked by a
// stand-alone program; under hipcc the same source builds for device.
#pragma once
#include <stdint.h>
#include <string.h>

#include "hd.h"

#if defined(__HIP_DEVICE_COMPILE__)
#define DN_TABLE_QUAL static __device__ const
#else
#define DN_TABLE_QUAL static const
#endif
#include "pow5_table.h"

namespace dn {

DN_HD_INLINE double dn_bits_to_double(uint64_t b) {
  double d;
  memcpy(&d, &b, 8);
  return d;
}

DN_HD_INLINE uint64_t dn_mulhi64(uint64_t a, uint64_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __umul64hi(a, b);
#else
  return (uint64_t)(((unsigned __int128)a * b) >> 64);
#endif
}

// Eisel-Lemire: nearest double to w * 10^exp10, w != 0 any 64-bit value.
DN_HD_NOINLINE double dn_dec2dbl_slow(uint64_t w, long exp10) {
  const uint64_t INF_BITS = 0x7FF0000000000000ull;
  // clamp before narrowing: anything past these is 0 / inf anyway
  int q = exp10 < -400 ? -400 : (exp10 > 400 ? 400 : (int)exp10);
  if (q < DN_POW5_QMIN) return 0.0;  // w*10^q < 2^-1075: rounds to 0
  if (q > DN_POW5_QMAX) return dn_bits_to_double(INF_BITS);
#if defined(__HIP_DEVICE_COMPILE__)
  int lz = __clzll((long long)w);
#else
  int lz = __builtin_clzll(w);
#endif
  w <<= lz;
  // 128-bit product w * 5^q, refined with the low table word only when
  // the 9 bits below the 55 we need are all ones
  uint32_t idx = 2u * (uint32_t)(q - DN_POW5_QMIN);
  uint64_t t_hi = DN_POW5_128[idx], t_lo = DN_POW5_128[idx + 1];
  uint64_t lo = w * t_hi, hi = dn_mulhi64(w, t_hi);
  if ((hi & 0x1FFull) == 0x1FFull) {
    uint64_t hi2 = dn_mulhi64(w, t_lo);
    lo += hi2;
    if (hi2 > lo) hi++;
  }
  int upper = (int)(hi >> 63);
  int shift = upper + 64 - 52 - 3;
  uint64_t m = hi >> shift;
  // floor(log2(10^q)) + 63, then the biased binary exponent
  int p2 = ((217706 * q) >> 16) + 63 + upper - lz + 1023;
  if (p2 <= 0) {  // subnormal (or zero)
    if (-p2 + 1 >= 64) return 0.0;
    m >>= (-p2 + 1);
    m += (m & 1);
    m >>= 1;
    // m == 2^52 here is the smallest normal: the bit IS the exponent
    return dn_bits_to_double(m);
  }
  // exact halfway only possible for small |q|: round to even
  if (lo <= 1 && q >= -4 && q <= 23 && (m & 3) == 1 &&
      (m << shift) == hi)
    m &= ~1ull;
  m += (m & 1);
  m >>= 1;
  if (m >= (2ull << 52)) { m = 1ull << 52; p2++; }
  m &= ~(1ull << 52);
  if (p2 >= 0x7FF) return dn_bits_to_double(INF_BITS);
  return dn_bits_to_double(((uint64_t)p2 << 52) | m);
}

// mant * 10^exp10, correctly rounded.  tbl22 = {1e0 .. 1e22}.
DN_HD_INLINE double dn_dec2dbl(uint64_t mant, long exp10,
                               const double* tbl22) {
  if (mant == 0) return 0.0;  // 0e999 is 0, not 0*inf
  if (mant < (1ull << 53) && exp10 >= -22 && exp10 <= 22) {
    double v = (double)mant;
    return exp10 >= 0 ? v * tbl22[exp10] : v / tbl22[-exp10];
  }
  return dn_dec2dbl_slow(mant, exp10);
}

}  // namespace dn
