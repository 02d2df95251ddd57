/* xl_q15_digits.h -- the host side of the matrix-core Q15 FIR (q15mm/xl_q15_mm.hip; engine option "q15_kernel"): plain C without HIP,
 * in the style of xl_q15_narrow.h and xl_resample_q15_quant.h.  tests/c/q15_digits_sweep.c sweeps it against int64 arithmetic under
 * ASan and UBSan (tests/test_q15_matrix_cpu.py); the kernel includes it for the sample digits and the combine.
 *
 * The reference sums int16 x int16 products in int64 (xlating.c:100-119).  The sums are integers, so any exact decomposition gives
 * the reference's bits.  Here every factor is written in signed int8 digits and the products are summed by v_mfma_i32_32x32x32_i8,
 * whose i32 accumulation is exact:
 *   rows of the A operand   one client's real-part row [cr, -ci] and imaginary-part row [ci, cr] over the interleaved index
 *                           K = 2 t + component, each ENTRY v (not each tap) split into balanced digits
 *                               lo = ((v + 128) mod 256) - 128,   hi = (v - lo) / 256        v = 256 hi + lo
 *   columns of the B operand   the window [xr, xi] of one output.  cs16: x = 256 hi + lo + 128 with hi = x >> 8, lo = (x & 255) - 128;
 *                           cu8 / cs8: x = 256 d with the single digit d = v - 128 / d = v (xlating.c:418, 425)
 *   cs16:      sum = 65536 S(hi,hi) + 256 (S(hi,lo) + S(lo,hi)) + S(lo,lo) + 128 sum(entries)
 *   cu8, cs8:  sum = 256 (256 S(hi,d) + S(lo,d))
 * A sample that does not exist (before the client's join, beyond the call) is the VALUE 0: digits hi = 0, lo = -128 in cs16.
 *
 * Proofs, per client, before the device is touched:
 *   (a) every digit of every entry fits int8 (xl_q15mm_admits_taps): lo always does, hi does for -32768 <= v <= 32639.  -ci is an
 *       entry of its own, so ci >= -32639 as well.  A client that fails stays on the float64 kernel; nothing is clamped.
 *   (b) every i32 accumulator stays below 2^31 (xl_q15mm_acc_bounded): |digit| <= 128, at most 2 products per (k, accumulator). */
#ifndef XL_Q15_DIGITS_H_
#define XL_Q15_DIGITS_H_

#include <stdint.h>

#include "xl_q15_narrow.h" /* XL_Q15_FN */

#define XL_QMM_ROWS 32u  /* clients per tile: the M of the matrix instruction */
#define XL_QMM_COLS 32u  /* most outputs per wave: its N */
#define XL_QMM_WAVES 8u  /* waves per workgroup: it covers XL_QMM_WAVES * nc consecutive outputs */
#define XL_QMM_KTAPS 16u /* complex taps per matrix instruction: K = 32 interleaved entries */
#define XL_QMM_FRAG 1024u /* bytes of one A fragment: 64 lanes x 16 entries */
#define XL_QMM_LDS_SAMPLES 32768u /* window image budget in samples per digit plane (2 bytes each, one or two planes) */
#define XL_QMM_ENTRY_MAX 32639 /* the largest entry with an int8 digit pair */

/* balanced digits of an entry: v = 256 hi + lo, -128 <= lo <= 127 */
XL_Q15_FN void xl_q15mm_entry_digits(int32_t v, int32_t *hi, int32_t *lo) {
  const int32_t l = (int32_t)((uint32_t)(v + 128 + 65536) & 255u) - 128;
  *lo = l;
  *hi = (v - l) / 256;
}
XL_Q15_FN int xl_q15mm_entry_ok(int32_t v) {
  int32_t hi, lo;
  xl_q15mm_entry_digits(v, &hi, &lo);
  return hi >= -128 && hi <= 127 && lo >= -128 && lo <= 127 && 256 * hi + lo == v;
}
/* digits of a cs16 sample component: x = 256 hi + lo + 128 */
XL_Q15_FN void xl_q15mm_cs16_digits(int32_t x, int32_t *hi, int32_t *lo) {
  *hi = x >> 8;
  *lo = (x & 255) - 128;
}

/* entry K (= 2 t' + component) of a client's row, taps delayed by `shift` samples: part 0 = the real-part row [cr, -ci], part 1 = the
 * imaginary-part row [ci, cr]; rtq: the T quantised, rotated taps (xl_prepare_taps), interleaved re, im */
XL_Q15_FN int32_t xl_q15mm_entry(const int16_t *rtq, uint32_t T, uint32_t shift, int part, uint32_t K) {
  const uint32_t tp = K >> 1, comp = K & 1u;
  if (tp < shift || tp - shift >= T) return 0;
  const int32_t cr = rtq[2u * (tp - shift)], ci = rtq[2u * (tp - shift) + 1u];
  return part == 0 ? (comp == 0u ? cr : -ci) : (comp == 0u ? ci : cr);
}

/* proof (a) */
XL_Q15_FN int xl_q15mm_admits_taps(const int16_t *rtq, uint32_t T) {
  for (uint32_t K = 0; K < 2u * T; ++K)
    if (!xl_q15mm_entry_ok(xl_q15mm_entry(rtq, T, 0u, 0, K)) || !xl_q15mm_entry_ok(xl_q15mm_entry(rtq, T, 0u, 1, K))) return 0;
  return 1;
}

/* matrix instructions along the taps: T taps delayed by up to 7 samples */
XL_Q15_FN uint32_t xl_q15mm_ksteps(uint32_t T) { return (T + 7u + XL_QMM_KTAPS - 1u) / XL_QMM_KTAPS; }
/* proof (b): ksteps * 32 entries, |digit x digit| <= 2^14, two such products per entry in the middle accumulator of cs16 */
XL_Q15_FN int xl_q15mm_acc_bounded(uint32_t ksteps) { return (uint64_t)ksteps * 32u * 16384u * 2u < ((uint64_t)1 << 31); }

/* 128 sum(entries) of a row: what the +128 of the cs16 low digit leaves out */
XL_Q15_FN int64_t xl_q15mm_correction(const int16_t *rtq, uint32_t T, int part) {
  int64_t s = 0;
  for (uint32_t K = 0; K < 2u * T; ++K) s += xl_q15mm_entry(rtq, T, 0u, part, K);
  return 128 * s;
}

XL_Q15_FN int64_t xl_q15mm_combine8(int32_t s_hi, int32_t s_lo) { return 256 * (256 * (int64_t)s_hi + (int64_t)s_lo); }
XL_Q15_FN int64_t xl_q15mm_combine16(int32_t s_hh, int32_t s_mid, int32_t s_ll, int64_t corr) {
  return 65536 * (int64_t)s_hh + 256 * (int64_t)s_mid + (int64_t)s_ll + corr;
}

/* ---- tile geometry.  Output i of a workgroup (i = 0 .. 8 nc - 1) reads its window at sample i D of the image; a lane's B fragment is
 * 8 consecutive samples, so the read is 16-byte aligned when i D = 0 mod 8.  Wave w takes the outputs of one residue class
 * i = r mod P, P = 8 / gcd(D, 8), r = w mod P: there i D mod 8 = r D mod 8 is one number, the taps are delayed by it (an image per
 * residue) and the window is read from the aligned sample below. */
XL_Q15_FN uint32_t xl_q15mm_residues(uint32_t D) { return (D & 1u) ? 8u : ((D & 2u) ? 4u : ((D & 4u) ? 2u : 1u)); }
XL_Q15_FN uint32_t xl_q15mm_shift(uint32_t D, uint32_t r) { return (r * (D & 7u)) & 7u; }
/* samples of the window image of a workgroup with nc outputs per wave */
XL_Q15_FN uint64_t xl_q15mm_span(uint32_t D, uint32_t ksteps, uint32_t nc) {
  return (uint64_t)(XL_QMM_WAVES * nc - 1u) * D + (uint64_t)XL_QMM_KTAPS * ksteps;
}
/* outputs per wave: the largest of 32, 16, .. 1 whose window image fits; 0: none does */
XL_Q15_FN uint32_t xl_q15mm_pick_nc(uint32_t D, uint32_t ksteps) {
  for (uint32_t nc = XL_QMM_COLS; nc >= 1u; nc >>= 1)
    if (xl_q15mm_span(D, ksteps, nc) <= XL_QMM_LDS_SAMPLES) return nc;
  return 0u;
}
/* bytes of a tile's A image: [residue][plane: real hi, real lo, imag hi, imag lo][kstep][lane][16 entries] */
XL_Q15_FN uint64_t xl_q15mm_image_bytes(uint32_t D, uint32_t ksteps) {
  return (uint64_t)xl_q15mm_residues(D) * 4u * ksteps * XL_QMM_FRAG;
}

/* One client's rows of a tile's image.  Lane l of a fragment holds row l & 31, entries K = 32 kstep + 16 (l >> 5) + 0..15 -- the B
 * fragments (the window) are laid out by the same rule, so the order of k inside the instruction cancels.  Rows without a client
 * stay zero (the caller clears the image). */
static inline void xl_q15mm_fill_row(int8_t *image, uint32_t row, const int16_t *rtq, uint32_t T, uint32_t D, uint32_t ksteps) {
  const uint32_t P = xl_q15mm_residues(D);
  for (uint32_t r = 0; r < P; ++r) {
    const uint32_t s = xl_q15mm_shift(D, r);
    for (int part = 0; part < 2; ++part)
      for (uint32_t kk = 0; kk < ksteps; ++kk)
        for (uint32_t h = 0; h < 2u; ++h)
          for (uint32_t e = 0; e < 16u; ++e) {
            int32_t hi, lo;
            xl_q15mm_entry_digits(xl_q15mm_entry(rtq, T, s, part, 32u * kk + 16u * h + e), &hi, &lo);
            const uint64_t at = ((uint64_t)kk * 64u + (row + 32u * h)) * 16u + e;
            image[(((uint64_t)r * 4u + 2u * (uint32_t)part) * ksteps) * XL_QMM_FRAG + at] = (int8_t)hi;
            image[(((uint64_t)r * 4u + 2u * (uint32_t)part + 1u) * ksteps) * XL_QMM_FRAG + at] = (int8_t)lo;
          }
  }
}

#endif /* XL_Q15_DIGITS_H_ */
