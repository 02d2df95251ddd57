/* xl_spectrum_cut.h -- how a feed cuts a stream's next n samples into transforms: pure integer state, plain C, no HIP (compiled by
 * gcc in tests/test_spectrum_bank_cpu.py, with the sanitizers under tools/sanitize.sh).  The single object (xl_spectrum.cpp) cuts every
 * span of a feed with it, the spectrum bank (xl_spectrum_bank.cpp) every stream of a feed.
 *
 * A stream of sampling_rate sr and width W has rows of F = sr / W transforms: transform g = row g / F, k = g % F covers stream samples
 * (g / F) * sr + (g % F) * W .. + W; the sr % W samples after a row's F-th transform are skipped.  Samples P0 .. P0 + n - 1 hold:
 *   - the end (or a further piece) of the transform that straddles P0, whose first `carry_have` samples are in the stream's carry:
 *     `carry_app` samples from the feed's start are appended; carry_done: that completes it, as transform carry_g starting at carry_t0;
 *   - `T` transforms wholly inside, g_first ..;
 *   - the first `save_n` samples of the transform that straddles P0 + n and starts inside the feed, at offset save_off of the feed:
 *     the new carry;
 *   - rows_done: how many rows have their F-th transform in once the feed is consumed (rows 0 .. rows_done - 1). */
#ifndef XL_SPECTRUM_CUT_H_
#define XL_SPECTRUM_CUT_H_

#include <stdint.h>

typedef struct {
  int64_t carry_have, carry_app, carry_done, carry_g, carry_t0;
  int64_t g_first, T;
  int64_t save_off, save_n;
  int64_t rows_done;
} XlSpecCut;

static inline XlSpecCut xl_spec_cut(int64_t sr, int64_t W, int64_t P0, int64_t n) {
  const int64_t F = sr / W, FW = F * W, P1 = P0 + n;
  const int64_t row0 = P0 / sr, pos0 = P0 % sr, row1 = P1 / sr, pos1 = P1 % sr;
  XlSpecCut c = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  if (n > 0 && pos0 < FW && pos0 % W != 0) {
    const int64_t k = pos0 / W, t0 = row0 * sr + k * W, t1 = t0 + W;
    c.carry_have = P0 - t0;
    c.carry_app = (t1 < P1 ? t1 : P1) - P0;
    c.carry_done = P0 + c.carry_app == t1;
    c.carry_g = row0 * F + k;
    c.carry_t0 = t0;
  }
  const int64_t kc = (pos0 + W - 1) / W;
  c.g_first = kc >= F ? (row0 + 1) * F : row0 * F + kc;
  const int64_t g_end = row1 * F + (pos1 / W < F ? pos1 / W : F);
  c.T = g_end > c.g_first ? g_end - c.g_first : 0;
  if (n > 0 && pos1 < FW && pos1 % W != 0) {
    const int64_t t0 = row1 * sr + (pos1 / W) * W;
    if (t0 >= P0) c.save_off = t0 - P0, c.save_n = P1 - t0;
  }
  c.rows_done = P1 >= FW ? (P1 - FW) / sr + 1 : 0;
  return c;
}

/* A stream has `slots` row slots for its maxima (row % slots).  Before sample P0 every row below P0 / sr is complete, so the samples up
 * to the end of row P0 / sr + slots - 1 touch `slots` distinct slots: the most one round of a feed may consume of this stream. */
static inline int64_t xl_spec_round_limit(int64_t sr, int64_t P0, int64_t slots) { return (P0 / sr + slots) * sr - P0; }

#endif /* XL_SPECTRUM_CUT_H_ */
