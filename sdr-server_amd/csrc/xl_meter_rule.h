/* xl_meter_rule.h -- the rule of the power meter (include/xlating_meter.h): how a row is cut into pieces, the power of a sample, and how
 * a row's partials become its mean power.  Plain C, no HIP, no libm, no header but <stdint.h>: the very same text runs in the kernel
 * (xl_meter.hip) and under gcc; tests/meter_ref.py restates it in numpy.
 *
 * PIECES.  A row is cut into pieces of XL_METER_PIECE = 2048 samples from its first sample; the last piece may be short.  One workgroup
 * of XL_METER_THREADS = 256 threads measures one piece and writes one partial of 8 bytes.
 *
 * CF32 ROWS (float32 pairs, 8-byte aligned).  Every operation is float32, single and unfused (the files that include this are compiled
 * with -ffp-contract=off), and float32 subnormals are KEPT (the kernel's default float mode on gfx950, float_denorm_mode_32 = 3; no flush
 * flag is passed):
 *   - sample j of the piece has p_j = fl(fl(re re) + fl(im im)); a sample past the row's end has p = +0;
 *   - thread t accumulates p_t, p_(t + 256), .., p_(t + 7 256) in that order, starting from the first;
 *   - within each wave of 64 threads the lane sums combine pairwise at strides 32, 16, 8, 4, 2, 1:  s[i] <- fl(s[i] + s[i + stride]);
 *   - the four wave sums combine as fl(fl(w0 + w1) + fl(w2 + w3)).
 * The piece's partial is that float32 (its bits in the low half of the 8 bytes, the high half 0).  The host adds a row's partials in
 * double, in ascending order, and divides by the sample count: the mean power, 1.0 = |y| of 1.  A row of 0 samples has power 0.
 *
 * THE BOUND.  u = 2^-24.  Every term is non-negative, so nothing cancels and the relative errors of the terms bound the sum's.  p_j
 * carries two rounding levels (a product, then the sum of the two products); on its way into the partial a term passes through at most
 * 7 additions in its thread, 6 in its wave and 2 across the waves: 15.  A partial therefore is sum p_j (1 + d_j) with
 * |d_j| <= (1 + u)^17 - 1 <= gamma_17 = 17 u / (1 - 17 u), provided no operation underflows: a subnormal product or sum loses absolute,
 * not relative, accuracy (at most 2^-150 per operation), which is why a row of subnormal squares is compared bit for bit with the
 * restatement and not against this bound.  The host's share: m partials take m - 1 double additions and one division, each within
 * v = 2^-53, and the conversions float32 -> double are exact: a factor within (1 + v)^m.  Together
 *     |mean - exact| <= ((1 + gamma_17) (1 + v)^m - 1) exact  <=  (gamma_17 + 1.0001 m v) exact   for m <= 2^19 (rows of up to 2^30 samples).
 *
 * CS16 ROWS (int16 pairs, 4-byte aligned).  p = re re + im im exactly, in integers (at most 2^31); the piece's partial is their sum
 * as a uint64 (at most 2^42), so any order gives the same bits.  The host adds partials in uint64 (a row of 2^30 samples stays below
 * 2^61) and gives  power = (double)sum / (double)count / 2^30:  full scale 32768 = 1.0, a row of all -32768 has power exactly 2.
 *
 * BOTH.  A non-finite partial (a NaN or an infinity in the row, or the overflow of a square) makes the row's power non-finite; the
 * squelch policy (xl_serve_squelch.h) treats that as open: a broken stream is never hidden. */
#ifndef XL_METER_RULE_H_
#define XL_METER_RULE_H_

#include <stdint.h>

#if defined(__HIPCC__)
#define XL_METER_FN static inline __host__ __device__
#else
#define XL_METER_FN static inline
#endif

#define XL_METER_THREADS 256u
#define XL_METER_PER_THREAD 8u /* samples per thread, XL_METER_THREADS apart */
#define XL_METER_PIECE (XL_METER_THREADS * XL_METER_PER_THREAD)
#define XL_METER_COUNT_MAX ((uint64_t)1 << 30) /* samples of one row */

/* pieces of a row of n samples */
XL_METER_FN uint64_t xl_meter_pieces(uint64_t n) { return (n + XL_METER_PIECE - 1u) / XL_METER_PIECE; }

/* the power of one cf32 sample */
XL_METER_FN float xl_meter_p_cf32(float re, float im) {
  const float a = re * re, b = im * im;
  return a + b;
}

/* the power of one cs16 sample: v holds re in its low and im in its high 16 bits */
XL_METER_FN uint32_t xl_meter_p_cs16(uint32_t v) {
  const int32_t re = (int16_t)(uint16_t)(v & 0xFFFFu), im = (int16_t)(uint16_t)(v >> 16);
  return (uint32_t)(re * re) + (uint32_t)(im * im);
}

/* one pairwise step of the float32 tree */
XL_METER_FN float xl_meter_add(float a, float b) { return a + b; }

/* the four wave sums of a piece */
XL_METER_FN float xl_meter_waves(float w0, float w1, float w2, float w3) {
  const float a = w0 + w1, b = w2 + w3;
  return a + b;
}

/* a cf32 row's mean power from its m partials (the float32 bits, ascending) and its n samples */
XL_METER_FN double xl_meter_mean_cf32(const uint64_t *partials, uint64_t m, uint64_t n) {
  union {
    uint32_t u;
    float f;
  } c;
  double sum = 0.0;
  for (uint64_t k = 0; k < m; ++k) {
    c.u = (uint32_t)partials[k];
    sum += (double)c.f;
  }
  return n == 0u ? 0.0 : sum / (double)n;
}

/* a cs16 row's */
XL_METER_FN double xl_meter_mean_cs16(const uint64_t *partials, uint64_t m, uint64_t n) {
  uint64_t sum = 0u;
  for (uint64_t k = 0; k < m; ++k) sum += partials[k];
  return n == 0u ? 0.0 : (double)sum / (double)n / 1073741824.0;
}

#endif /* XL_METER_RULE_H_ */
