/* xl_tune_rule.h -- the rule of the tuner bank (include/xlating_tune.h): the phase of every sample of a stream, the sine and cosine of
 * a phase.  Plain C, no HIP, no table, no libm, no header but <stdint.h>: the very same text runs in the kernel (xl_tune.hip) and under
 * gcc, where tests/c/tune_rule_sweep.c holds it to libm and to 128-bit integers.  The steps from Hz are the host's alone: xl_tune_hz.h.
 *
 * PHASE.  64-bit and modular; 2^64 is one turn.  A stream's state is P (uint64, the phase of the next sample), F (int64, turns * 2^64
 * per sample) and R (int64, turns * 2^64 per sample^2).  Sample j = 0, 1, .. of a feed has
 *     phi_j = P + j F + (j (j - 1) / 2) R   mod 2^64,
 * and after a feed of n samples  P <- P + n F + (n (n - 1) / 2) R,  F <- F + n R,  both wrapping.  j and n stay at or below 2^30 (a little
 * above in the kernel's last workgroup of a row, whose surplus threads compute a phase nobody uses), so j (j - 1) is exact in 64 bits
 * and its half is an integer.  The arithmetic is exact: stepping phi by additions gives the bits of the closed form (xl_tune_stride).
 *
 * SINE AND COSINE of 2 pi p / 2^32, p the top 32 bits of a phase.  In integers: q = the nearest quarter turn, r = p - q 2^30 in
 * [-2^29, 2^29), a = |r|.  In float32, every operation single and unfused (the files that include this are compiled with
 * -ffp-contract=off): x = fl(fl(a) K), K = fl(2 pi / 2^32); z = fl(x x); the Taylor polynomials of degree 9 (sine) and 10 (cosine) in
 * Horner form over z, s0 = fl(x + fl(x fl(z ps))), c0 = fl(1 + fl(z pc)).  At a = 2^29, the eighth of a turn, s0 is c0: the one
 * point both symmetries below map to itself.  s0 takes the sign of r, and the quarter turn q maps (c0, s0) to (c0, s0), (-s0, c0),
 * (-c0, -s0), (s0, -c0).  What follows, and what the sweep holds over all 2^32 phases:
 *   - at p = k 2^30 the values are 0 and +-1 exactly (a = 0: x = 0, s0 = 0, c0 = 1);
 *   - cs(p + 2^30) = (-s, c) as values, bit for bit (q moves by one, r stays);
 *   - cs(-p) = (c, -s) as values, bit for bit (q and r change sign; at r = -2^29, where they do not, c0 = s0);
 *   - the largest error against libm's double cos and sin is the sweep's to measure.
 *
 * THE PRODUCT, in float32:  re = fl(fl(xr c) - fl(xi s)),  im = fl(fl(xr s) + fl(xi c)),  (c, s) = xl_tune_cs(phi_j >> 32).  A positive
 * F moves the spectrum up. */
#ifndef XL_TUNE_RULE_H_
#define XL_TUNE_RULE_H_

#include <stdint.h>

#if defined(__HIPCC__)
#define XL_TUNE_FN static inline __host__ __device__
#else
#define XL_TUNE_FN static inline
#endif

#define XL_TUNE_COUNT_MAX ((uint64_t)1 << 30) /* samples of one stream in one feed */

/* j (j - 1) / 2, j <= 2^32 */
XL_TUNE_FN uint64_t xl_tune_tri(uint64_t j) { return (j * (j - 1u)) >> 1; }

/* phi_j */
XL_TUNE_FN uint64_t xl_tune_phase(uint64_t P, int64_t F, int64_t R, uint64_t j) {
  return P + j * (uint64_t)F + xl_tune_tri(j) * (uint64_t)R;
}

/* phi_(j + S) - phi_j = S F + (S j + S (S - 1) / 2) R; the same difference S samples on is larger by S S R */
XL_TUNE_FN uint64_t xl_tune_stride(int64_t F, int64_t R, uint64_t j, uint64_t S) {
  return S * (uint64_t)F + (S * j + xl_tune_tri(S)) * (uint64_t)R;
}

/* the state after n samples */
XL_TUNE_FN void xl_tune_advance(uint64_t *P, int64_t *F, int64_t R, uint64_t n) {
  *P = xl_tune_phase(*P, *F, R, n);
  *F = (int64_t)((uint64_t)*F + n * (uint64_t)R);
}

XL_TUNE_FN void xl_tune_cs(uint32_t p, float *c, float *s) {
  const uint32_t q = (uint32_t)(p + 0x20000000u) >> 30;
  const int32_t r = (int32_t)(p - (q << 30));
  const uint32_t a = r < 0 ? 0u - (uint32_t)r : (uint32_t)r;
  const float x = (float)a * 1.4629180792671596e-9f;
  const float z = x * x;
  float ps = 2.7557319223985893e-6f; /* 1 / 9! */
  ps = ps * z - 1.9841269841269841e-4f; /* 1 / 7! */
  ps = ps * z + 8.3333333333333333e-3f; /* 1 / 5! */
  ps = ps * z - 1.6666666666666667e-1f; /* 1 / 3! */
  float pc = -2.7557319223985888e-7f; /* 1 / 10! */
  pc = pc * z + 2.4801587301587302e-5f; /* 1 / 8! */
  pc = pc * z - 1.3888888888888889e-3f; /* 1 / 6! */
  pc = pc * z + 4.1666666666666664e-2f; /* 1 / 4! */
  pc = pc * z - 0.5f;
  const float zs = z * ps, zc = z * pc;
  const float xs = x * zs;
  const float c0 = 1.0f + zc;
  float s0 = x + xs;
  s0 = a == 0x20000000u ? c0 : s0;
  s0 = r < 0 ? -s0 : s0;
  const float cc = (q & 1u) != 0u ? -s0 : c0, ss = (q & 1u) != 0u ? c0 : s0;
  *c = (q & 2u) != 0u ? -cc : cc;
  *s = (q & 2u) != 0u ? -ss : ss;
}

/* one sample of the product */
XL_TUNE_FN void xl_tune_rotate(float xr, float xi, uint64_t phi, float *re, float *im) {
  float c, s;
  xl_tune_cs((uint32_t)(phi >> 32), &c, &s);
  const float a = xr * c, b = xi * s, d = xr * s, e = xi * c;
  *re = a - b;
  *im = d + e;
}

#endif /* XL_TUNE_RULE_H_ */
