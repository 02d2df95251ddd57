/* xl_q15_narrow.h -- the two narrowing steps between a Q15 sum and an int16 of the cs16 family (xlating.c:85-90, 118-119): plain C
 * that a host compiler takes as it is (tests/c/q15_narrow_sweep.c sweeps it against int64 arithmetic, tests/test_q15_extremes_cpu.py)
 * and that the kernels include through xl_dev_inline.h.  Every Q15 kernel that carries its sums in float64 narrows them HERE.
 *
 * The reference sums int16 x int16 products in int64 and writes  saturate_to_int16(temp >> 15);  saturate_to_int16 takes an int32_t,
 * so the shifted sum is first cut to its low 32 bits (two's complement) and only then saturated.  With full-scale samples and taps
 * |sum >> 15| reaches 2^31 from 32768 taps on: a window of 65700 taps of 0.9999 over samples of +32767 gives a shifted sum of
 * 2152529108, which the reference reads as -2142438188 and saturates to -32768, not +32767. */
#ifndef XL_Q15_NARROW_H_
#define XL_Q15_NARROW_H_

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define XL_Q15_FN static __host__ __device__ __forceinline__
#else
#define XL_Q15_FN static inline
#endif

XL_Q15_FN int32_t xl_sat16(int32_t v) { return v > 32767 ? 32767 : (v < -32768 ? -32768 : v); } /* xlating.c:85-90 */

/* acc: an int64 sum held exactly in a double (|acc| < 2^53).  floor(acc / 32768) is the arithmetic shift by 15 -- the scaling by a
 * power of two is exact and the quotient is below 2^38, so its conversion to int64 is defined and exact -- then the reference's cut
 * to 32 bits, then its saturation.  (A direct double -> int32 conversion of a quotient outside the int32 range is undefined in C++
 * and clamps on gfx950: the opposite sign from the reference once the sum has wrapped.) */
XL_Q15_FN int32_t xl_q15_narrow_sum(double acc) {
  const int64_t q = (int64_t)__builtin_floor(acc * (1.0 / 32768.0));
  return xl_sat16((int32_t)(uint32_t)(uint64_t)q);
}

/* The same for a sum held as an int64 (the matrix-core FIR, xl_q15_digits.h): the reference's own line, the cut written on unsigned
 * values.  (>> of a negative int64 is the arithmetic shift on every compiler this project builds with; the reference relies on it too.) */
XL_Q15_FN int32_t xl_q15_narrow_sum64(int64_t sum) { return xl_sat16((int32_t)(uint32_t)(uint64_t)(sum >> 15)); }

#endif /* XL_Q15_NARROW_H_ */
