/* xl_dlv_gain.h -- the conversion rule of the narrowing delivery WITH A GAIN (xlating_delivery_pack_device_cs16_gain) and the level of a
 * delivered row: xl_dlv_narrow.h's rule with a power of two per row in front of it, and what the row's meter counts.  Plain C, no HIP,
 * integer arithmetic only: the very same text runs in the kernel (xl_delivery_gain.hip) and under gcc, where
 * tests/c/delivery_gain_sweep.c holds it to libm, and the kernel's code object holds no floating-point instruction.
 *
 * The rule, for a float y and a gain g in XL_DLV_GAIN_MIN .. XL_DLV_GAIN_MAX:  NaN (any payload, either sign) -> 0;  otherwise
 * clamp(rne(y * 2^(15 + g)), -32768, 32767), rne = to nearest, ties to even.  The product by a power of two is exact, so there is ONE
 * rounding.  At g = 0 the value is xl_dlv_narrow's for every bit pattern.
 *
 * In fields: y = (-1)^s * m * 2^(e - 150) with m = 2^23 + fraction (e >= 1), so |y| * 2^(15 + g) = m * 2^(e + g - 135) = m >> k with
 * k = 135 - (e + g): the rule of xl_dlv_narrow.h with the exponent field read as eg = e + g (-48 .. 303).
 *   eg >= 128: the magnitude is at least 65536: saturated, and the clamp acted on either side.  Inf is e = 255 with no fraction, and
 *              eg >= 207 for it under every admitted g; a NaN, e = 255 with a fraction, gives 0 and is no clamp.
 *   eg == 127: k = 8, q = rne(m / 256) = 32768 .. 65536: saturated; the clamp acted on the positive side always, on the negative side
 *              when q > 32768 (-32768 is a value: -1.0 * 2^-g is delivered as it is).
 *   eg <= 110: below half an LSB: 0.  k is held at 25 there, where m >> k = 0 and the remainder m lies below the half 2^24.  A denormal
 *              (e = 0) has eg <= 48 under every admitted g: always 0, whatever its fraction, and the hidden bit it does not have is
 *              never looked at.
 *   between:   k = 9 .. 24 as in xl_dlv_narrow.h; the largest q is 32767 + 1 (eg = 126, the fraction's top bits set), which the clamp
 *              takes on the positive side.
 * The clamp ACTED where the rounded magnitude q exceeds what its side holds: q > 32767 for a positive value, q > 32768 for a negative.
 *
 * The level of a row, over its floats: peak_bits = the largest (bits & 0x7FFFFFFF) of the floats that are no NaN -- positive floats
 * order as their bit patterns do, so this is the bit pattern of the largest magnitude BEFORE the gain (0 for an empty or all-NaN row,
 * 0x7F800000 for an Inf); clipped = the floats where the clamp acted; nans = the NaN floats.  An integer maximum and two integer sums:
 * the same under any chunking, any company of rows and any order of reduction. */
#ifndef XL_DLV_GAIN_H_
#define XL_DLV_GAIN_H_

#include <stdint.h>

#if defined(__HIPCC__)
#define XL_DLV_GAIN_FN static inline __host__ __device__
#else
#define XL_DLV_GAIN_FN static inline
#endif

#define XL_DLV_GAIN_MIN (-48)
#define XL_DLV_GAIN_MAX 48

/* 1 for a NaN */
XL_DLV_GAIN_FN uint32_t xl_dlv_gain_nan(uint32_t bits) { return (bits & 0x7FFFFFFFu) > 0x7F800000u ? 1u : 0u; }

/* what the float offers the row's peak: its magnitude's bits, 0 for a NaN */
XL_DLV_GAIN_FN uint32_t xl_dlv_gain_mag(uint32_t bits) { return xl_dlv_gain_nan(bits) != 0u ? 0u : bits & 0x7FFFFFFFu; }

/* bits: the float's 32 bits; g: the gain, XL_DLV_GAIN_MIN .. XL_DLV_GAIN_MAX; *clamped: 1 where the clamp acted, else 0 */
XL_DLV_GAIN_FN int16_t xl_dlv_gain_narrow(uint32_t bits, int32_t g, uint32_t *clamped) {
  const uint32_t e = (bits >> 23) & 0xFFu, frac = bits & 0x7FFFFFu, neg = bits >> 31;
  const int32_t eg = (int32_t)e + g;
  /* (selects, no early return, as in xl_dlv_narrow.h; k of a saturating eg is any valid shift) */
  const uint32_t m = frac | 0x800000u, k = eg > 110 ? (eg < 128 ? (uint32_t)(135 - eg) : 8u) : 25u;
  const uint32_t rem = m & ((1u << k) - 1u), half = 1u << (k - 1u);
  uint32_t q = m >> k;
  q += ((rem > half) | ((rem == half) & (q & 1u))) != 0u ? 1u : 0u;
  q = eg < 128 ? q : 65536u;
  q = ((e == 0xFFu) & (frac != 0u)) != 0u ? 0u : q;
  const uint32_t lim = neg != 0u ? 32768u : 32767u;
  const uint32_t held = q > lim ? lim : q;
  *clamped = q > lim ? 1u : 0u;
  return (int16_t)(neg != 0u ? -(int32_t)held : (int32_t)held);
}

#endif /* XL_DLV_GAIN_H_ */
