/* xl_resample_cut.h -- what a feed of n samples holds for one stream of the resampler bank: pure integer state, plain C, no HIP
 * (compiled by gcc in tests/test_resample_cpu.py, with the sanitizers in that file's stand-alone sweep).  The bank's host side
 * (xl_resample.cpp) calls nothing else for this arithmetic.
 *
 * A stream of ratio L / M (coprime) with Q = ceil(taps / L) taps per phase: output m sits at t = m * M on the grid of the input
 * upsampled by L; it reads inputs n_m = t / L, n_m - 1, .. n_m - (Q - 1) with phase p_m = t % L, and exists once x[n_m] has been
 * consumed.  After P consumed samples the stream has produced ceil(P * L / M) outputs.  Samples P0 .. P0 + n - 1 therefore bring
 *   - outputs m_first .. m_first + count - 1, m_first = ceil(P0 * L / M);
 *   - the first of them at input n_first (RELATIVE to the feed's first sample, so >= 0 here; the taps reach back to
 *     n_first - (Q - 1), and what is negative lies in the carry) with phase p_first;
 *   - a new carry of the stream's last Q - 1 inputs: its last carry_new samples are the feed's last ones, the carry_old before them
 *     are the old carry's last ones (a short feed shifts the carry).
 * m * M stays within 64 bits: m_first * M < P0 * L + M, with P0 * L < 2^64 for P0 < 2^52 (L <= 4096). */
#ifndef XL_RESAMPLE_CUT_H_
#define XL_RESAMPLE_CUT_H_

#include <stdint.h>

typedef struct {
  uint64_t m_first, count;
  int64_t n_first;
  uint32_t p_first;
  uint32_t carry_new, carry_old;
} XlResampleCut;

static inline uint64_t xl_resample_produced(uint64_t L, uint64_t M, uint64_t P) { return (P * L + M - 1u) / M; }

static inline XlResampleCut xl_resample_cut(uint32_t L, uint32_t M, uint32_t Q, uint64_t P0, uint64_t n) {
  XlResampleCut c;
  const uint64_t t = xl_resample_produced(L, M, P0) * (uint64_t)M;
  c.m_first = t / M;
  c.count = xl_resample_produced(L, M, P0 + n) - c.m_first;
  c.n_first = (int64_t)(t / L - P0);
  c.p_first = (uint32_t)(t % L);
  c.carry_new = (uint32_t)(n < (uint64_t)(Q - 1u) ? n : (uint64_t)(Q - 1u));
  c.carry_old = (Q - 1u) - c.carry_new;
  return c;
}

#endif /* XL_RESAMPLE_CUT_H_ */
