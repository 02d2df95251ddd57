/* xl_spectrum_bank_plan.h -- the integer rules of the spectrum bank's wide form (widths above 8192: xl_spectrum_bank.cpp,
 * xl_spectrum_bank_wide.hip): pure integers, plain C, no HIP (compiled by gcc, with the sanitizers, in tests/c/spectrum_bank_plan_sweep.c).
 * The only place that decides them.
 *
 * Chunks: a round's T transforms (all streams' runs, one ragged list) go through the scratch `per` = xl_specw_chunk(scratch, N)
 * transforms at a time: chunk i is transforms i * per .. of the list, the last one shorter.  Where a chunk ends has nothing to do with
 * where a stream's run ends.
 * Staging: a round's completed rows go through one staging buffer of `stage_bytes` (a row is W floats and W pixel bytes), at least one
 * row.  A round has a budget of that many rows; a stream may consume in a round what its row slots allow (xl_spec_round_limit) and at
 * most up to one sample short of completing one row more than what is left of the budget.  A stream that finds the budget used up
 * waits for the next round.  The first stream of a round always finds a budget of at least one row, and completing a row takes at least
 * one sample: no round is empty.
 * Growth: the per-stream arrays of a wide bank start at as many streams as XL_BANKW_FIRST_BYTES hold (1 .. 64), not at 64. */
#ifndef XL_SPECTRUM_BANK_PLAN_H_
#define XL_SPECTRUM_BANK_PLAN_H_

#include <stdint.h>

#include "xl_spectrum_cut.h"

#define XL_BANKW_STAGE_DEFAULT ((uint64_t)32 << 20) /* bytes of the dB staging and the pixel staging together */
#define XL_BANKW_FIRST_BYTES ((uint64_t)64 << 20)
#define XL_BANKW_CARRY_PIECE 4096u /* samples of a carry that one workgroup copies */

/* chunks of `per` (>= 1) transforms that cover T */
static inline uint64_t xl_bankw_chunks(uint64_t T, uint64_t per) { return (T + per - 1u) / per; }
/* transforms of chunk i (< xl_bankw_chunks): its base is i * per */
static inline uint64_t xl_bankw_chunk_len(uint64_t T, uint64_t per, uint64_t i) {
  const uint64_t base = i * per;
  return T - base < per ? T - base : per;
}

/* rows a staging of stage_bytes holds (W * 5 bytes each), at least one */
static inline uint64_t xl_bankw_stage_rows(uint64_t stage_bytes, uint32_t W) {
  const uint64_t r = stage_bytes / (5ull * W);
  return r > 0 ? r : 1;
}

/* rows complete before sample P0 (xl_spec_cut's rows_done of everything consumed so far) */
static inline int64_t xl_bankw_rows_before(int64_t sr, int64_t W, int64_t P0) {
  const int64_t FW = (sr / W) * W;
  return P0 >= FW ? (P0 - FW) / sr + 1 : 0;
}

/* the most a stream at P0 may consume in a round that may still complete `budget` rows: 0 when budget <= 0, else > 0 */
static inline int64_t xl_bankw_round_limit(int64_t sr, int64_t W, int64_t P0, int64_t slots, int64_t budget) {
  if (budget <= 0) return 0;
  const int64_t by_slots = xl_spec_round_limit(sr, P0, slots);
  const int64_t FW = (sr / W) * W;
  /* row r completes with sample r * sr + FW - 1: stop one short of completing row rows_before + budget */
  const int64_t by_rows = (xl_bankw_rows_before(sr, W, P0) + budget) * sr + FW - 1 - P0;
  return by_slots < by_rows ? by_slots : by_rows;
}

/* streams the per-stream arrays of a wide bank start at: what XL_BANKW_FIRST_BYTES hold of `stream_bytes` each, 1 .. 64 */
static inline uint32_t xl_bankw_first_streams(uint64_t stream_bytes) {
  const uint64_t n = stream_bytes > 0 ? XL_BANKW_FIRST_BYTES / stream_bytes : 64u;
  return n < 1u ? 1u : (n > 64u ? 64u : (uint32_t)n);
}

#endif /* XL_SPECTRUM_BANK_PLAN_H_ */
