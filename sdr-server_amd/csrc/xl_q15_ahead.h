/* xl_q15_ahead.h -- the decisions of the Q15 family's phase look-ahead (engine option "q15_nco"; xl_batch.cpp, xl_call_q15): plain C
 * without HIP, in the style of xl_q15_digits.h.  tests/c/q15_ahead_sweep.c sweeps both functions under ASan and UBSan
 * (tests/test_q15_nco_cpu.py); the engine calls them and decides nothing of this on its own.
 *
 * After a Q15 call at stream position `pos`, xl_nco_q15_ahead_kernel tabulates on the side stream the phases of a call at
 * xl_grid_next(pos): same block length, same block count, right behind this one.  The record of what was tabulated is the XlPos
 * itself.  The Q15 phase is never renormalised and takes no flag of the position (XlPos::pad belongs to the float families), so a
 * table serves exactly the calls whose trel, S and G are the record's: those three numbers fix every client's output count
 * (xl_grid_dyn), and the committed phases it started from are the ones the call starts from as long as no Q15 call ran in between --
 * any call in between, of either family, moves trel. */
#ifndef XL_Q15_AHEAD_H_
#define XL_Q15_AHEAD_H_

#include <stdint.h>

#include "xl_grid.h"

#define XL_Q15_AHEAD_TREL_END ((uint64_t)1 << 31) /* the engine re-plans before a call would carry trel to here (xl_call_begin) */

/* Does the pending look-ahead (pending != 0, tabulated for `rec`) serve the call at `pos`? */
static inline int xl_q15_ahead_serves(int pending, XlPos rec, XlPos pos) {
  return pending != 0 && rec.trel == pos.trel && rec.S == pos.S && rec.G == pos.G;
}

/* May a look-ahead for the call behind the one at `pos` be launched?  Not when that call is going to re-plan anyway, which drops
 * every table: clients the plan holds as immature (they merge into their classes once mature), a stream position that would reach
 * 2^31 within two more calls of this size (the next call starts at trel + N; the re-base test in xl_call_begin is on ITS end,
 * trel + 2 N), an engine without clients.  All in 64 bits: S * G alone may pass 2^32. */
static inline int xl_q15_ahead_may_launch(XlPos pos, int planned_immature, uint32_t nclients) {
  const uint64_t N = (uint64_t)pos.S * (uint64_t)pos.G;
  if (planned_immature > 0 || nclients == 0u) return 0;
  return (uint64_t)pos.trel + 2u * N < XL_Q15_AHEAD_TREL_END;
}

#endif /* XL_Q15_AHEAD_H_ */
