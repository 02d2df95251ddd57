/* xl_resample_q15_quant.h -- the tap quantiser of the Q15 resampler bank (include/xlating_resample_q15.h): plain C, no HIP (compiled
 * by gcc alone, with the sanitizers, in tests/test_resample_q15_cpu.py).  xlating_resample_q15_quantize and the bank's add call
 * nothing else for this arithmetic.
 *
 * c[i] = (int16) trunc(h[i] * 32768), the product in float32 (a power-of-two scaling: exact, or an overflow to infinity, which is
 * out of range like every other value at or beyond 2^15), truncation toward zero -- the reference's own quantisation of its taps
 * (xlating.c:486-487).  Nothing is clamped: a tap that is not finite, or whose truncated value lies outside [-32768, 32767], is
 * -ERANGE.  The range is decided on the float, BEFORE the conversion: converting an out-of-range float to an integer is undefined.
 * trunc(v) lies in [-32768, 32767] exactly when -32769 < v < 32768 (both bounds are float32 numbers); a NaN fails both. */
#ifndef XL_RESAMPLE_Q15_QUANT_H_
#define XL_RESAMPLE_Q15_QUANT_H_

#include <errno.h>
#include <stddef.h>
#include <stdint.h>

/* 0; -EINVAL: taps == NULL, out == NULL or len == 0; -ERANGE (out[] is then unspecified). */
static inline int xl_resample_q15_quantize(const float *taps, size_t len, int16_t *out) {
  if (taps == NULL || out == NULL || len == 0) return -EINVAL;
  for (size_t i = 0; i < len; ++i) {
    const float v = taps[i] * 32768.0f;
    if (!(v > -32769.0f && v < 32768.0f)) return -ERANGE;
    out[i] = (int16_t)(int32_t)v; /* (in range: the conversion truncates toward zero) */
  }
  return 0;
}

#endif /* XL_RESAMPLE_Q15_QUANT_H_ */
