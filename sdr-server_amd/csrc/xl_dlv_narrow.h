/* xl_dlv_narrow.h -- the conversion rule of the narrowing delivery (xlating_delivery_pack_device_cs16): one float of a cf32 row to one
 * int16 of the cs16 row that crosses to the host.  Plain C, no HIP, integer arithmetic only: the very same text runs in the kernel
 * (xl_delivery_narrow.hip) and under gcc, where tests/c/delivery_narrow_sweep.c holds it to libm on all 2^32 bit patterns, and the
 * kernel's code object holds no floating-point instruction.
 *
 * The rule, for a float y:  NaN (any payload, either sign) -> 0;  otherwise clamp(rne(y * 32768), -32768, 32767), rne = to nearest,
 * ties to even.  The scale is the Q15 family's: +1.0 -> 32767, -1.0 -> -32768, +-Inf saturate, denormals and -0.0 -> 0, +-2^-16 (half
 * an LSB, a tie) -> 0, +-1.5 LSB -> +-2.
 *
 * In fields: y = (-1)^s * m * 2^(e - 150) with m = 2^23 + fraction (e >= 1), so |y| * 32768 = m * 2^(e - 135) = m >> k, k = 135 - e.
 *   e >= 127: |y| >= 1, the magnitude saturates (Inf is e = 255 with no fraction; a NaN, e = 255 with one, gives 0).
 *   e <= 110: |y| < 2^-16, below half an LSB: 0.  k is held at 25 there, where m >> k = 0 and the remainder m lies below the half 2^24
 *             (a denormal's m, taken with the hidden bit it does not have, still does).
 *   between:  k = 9 .. 24, q = m >> k, rounded up when the remainder exceeds the half, or equals it with q odd.  The largest q is
 *             32767 + 1 (e = 126, the fraction's top bits set): the clamp takes it on the positive side, -32768 is a value. */
#ifndef XL_DLV_NARROW_H_
#define XL_DLV_NARROW_H_

#include <stdint.h>

#if defined(__HIPCC__)
#define XL_DLV_NARROW_FN static inline __host__ __device__
#else
#define XL_DLV_NARROW_FN static inline
#endif

/* bits: the float's 32 bits */
XL_DLV_NARROW_FN int16_t xl_dlv_narrow(uint32_t bits) {
  const uint32_t e = (bits >> 23) & 0xFFu, frac = bits & 0x7FFFFFu, neg = bits >> 31;
  /* (selects, no early return: the kernel converts eight floats a slot in straight-line code; k of a saturating e is any valid shift) */
  const uint32_t m = frac | 0x800000u, k = e > 110u ? (e < 127u ? 135u - e : 9u) : 25u;
  const uint32_t rem = m & ((1u << k) - 1u), half = 1u << (k - 1u);
  uint32_t q = m >> k;
  q += ((rem > half) | ((rem == half) & (q & 1u))) != 0u ? 1u : 0u;
  q = e < 127u ? q : 32768u;
  q = ((e == 0xFFu) & (frac != 0u)) != 0u ? 0u : q;
  const uint32_t pos = q > 32767u ? 32767u : q;
  return (int16_t)(neg != 0u ? -(int32_t)q : (int32_t)pos);
}

#endif /* XL_DLV_NARROW_H_ */
