/* xl_q15_ahead.h -- the Q15 family's phase look-ahead (engine option "q15_nco"; xl_batch.cpp, xl_call_q15): its state and every decision,
 * plain C without HIP, the twin of xl_ahead.h.  tests/c/q15_ahead_sweep.cpp sweeps the two predicates position by position and drives the
 * rest through sequences of calls against a model of streams and events, under ASan and UBSan (tests/test_q15_nco_cpu.py); the engine
 * calls these functions, executes the synchronisation they return (XlAheadOps, by xl_ahead_run) and launches what they tell it to: it
 * decides nothing of this on its own.
 *
 * After a Q15 call at stream position `pos`, xl_nco_q15_ahead_kernel tabulates on the side stream the phases of a call at
 * xl_grid_next(pos): same block length, same block count, right behind this one.  The record of what was tabulated is the XlPos
 * itself.  The Q15 phase is never renormalised and takes no flag of the position (XlPos::pad belongs to the float families), so a
 * table serves exactly the calls whose trel, S and G are the record's: those three numbers fix every client's output count
 * (xl_grid_dyn), and the committed phases it started from are the ones the call starts from as long as no Q15 call ran in between --
 * any call in between, of either family, moves trel.
 *
 * The buffers.  The engine owns two phase buffers d_qphase[2] (per slot the running Q15 phase, xlating.c:546-547: it starts at
 * 32767 + 0j) and two phase tables d_qphtab[2] (every XL_PH_STRIDE-th phase), the events ev_qchain and ev_qready and the side stream
 * nco_stream; this state holds indices into them.
 *   - [cur] holds the committed running phases: those behind the latest Q15 call.  The host writes a new client's start phase there and
 *     reads a client's phase from there, with every stream synchronised.  Table [tab] is the latest Q15 call's.
 *   - Option 0: xl_nco_q15_batch_kernel steps [cur] in place into table [tab], in front of the call's launches on the call's stream;
 *     [cur ^ 1] and [tab ^ 1] hold nothing anybody reads, the indices never move.
 *   - Option 1: every tabulation is xl_nco_q15_ahead_kernel's, [cur] -> [cur ^ 1] into table [tab ^ 1], which the call's FIR, matrix and
 *     wide launches read; the call's commit flips both indices, whoever tabulated.  Between calls [cur ^ 1] holds the phases in front of
 *     the latest call and [tab ^ 1] the table of the call before it: nothing anybody reads.
 *   - A look-ahead pending (option 1 only): [cur ^ 1] and [tab ^ 1] hold, or will hold once ev_qchain has come, the phases behind and the
 *     table of a call at `rec`, tabulated from [cur] on nco_stream.  [cur] and [tab] are untouched by it.
 *   - ev_qchain: the look-ahead is complete.  While one is pending EVERY Q15 call waits for it on its own stream in front of its
 *     tabulation, hit or miss: a hit reads the table, a miss writes the very buffers the look-ahead writes, and an option-0 call steps in
 *     place the phases it reads.
 *   - ev_qready, recorded on the call's stream between its table and its FIR launches (option 1): the phases this call commits are written,
 *     and -- calls being ordered one behind the other -- the previous call's launches, the readers of the table that is now the spare
 *     one, have been passed.  That is what a look-ahead launched behind this call reads and overwrites; nco_stream waits for it first.
 *     One launch per call carries an event (~8 us).
 *   - Dropped.  A call the record does not serve and an option-0 call drop a pending look-ahead behind their wait for ev_qchain; a join,
 *     a re-plan and the rebuild of the all-clients launch set drop it after they have synchronised every stream; setting the option (every
 *     stream synchronised as well) forgets it and restarts the counters.  xlating_batch_sync waits for nco_stream while one is pending. */
#ifndef XL_Q15_AHEAD_H_
#define XL_Q15_AHEAD_H_

#include <stdbool.h>
#include <stdint.h>

#include "xl_grid.h"
#include "xl_ahead.h"

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

typedef struct {
  int cur, tab;
  bool pending; /* a look-ahead is in flight or complete, for the call at `rec` */
  XlPos rec;
  uint64_t used, dropped; /* since the option was set: look-aheads that served their call / that were tabulated for nothing */
} XlQ15Ahead;

static inline XlQ15Ahead xl_q15_ahead_init(void) {
  const XlQ15Ahead a = {0, 0, false, {0u, 0u, 0u, 0u}, 0u, 0u};
  return a;
}
static inline bool xl_q15_ahead_pending(const XlQ15Ahead *a) { return a->pending; }
/* Forget the table tabulated a call ahead.  The caller has waited for it: every stream synchronised, or `pre` of xl_q15_ahead_begin. */
static inline void xl_q15_ahead_drop(XlQ15Ahead *a) {
  if (a->pending) a->dropped++;
  a->pending = false;
}
/* The option is set (to either value), every stream synchronised: the counters count from here. */
static inline void xl_q15_ahead_option_set(XlQ15Ahead *a) {
  a->pending = false;
  a->used = a->dropped = 0;
}

/* A Q15 call at `pos` begins: run `pre` on the call's stream; unless `hit`, tabulate [phase_in] -> table [tab], [phase_out] there
 * (in_place: xl_nco_q15_batch_kernel on phase_in == phase_out, else xl_nco_q15_ahead_kernel); run `post`; the call's launches read
 * table [tab]. */
typedef struct {
  bool hit;      /* the table was tabulated ahead */
  bool in_place; /* option 0 */
  int phase_in, phase_out, tab;
  XlAheadOps pre, post;
} XlQ15AheadBegin;

static inline XlQ15AheadBegin xl_q15_ahead_begin(XlQ15Ahead *a, bool option_on, XlPos pos) {
  XlQ15AheadBegin d = {false, !option_on, a->cur, a->cur, a->tab, {0, {{0, 0, 0, 0}}}, {0, {{0, 0, 0, 0}}}};
  if (a->pending) xl_ahead_op(&d.pre, XL_AHEAD_WAIT, XL_AHEAD_S_CALL, XL_AHEAD_EV_QCHAIN, 0);
  if (option_on) {
    d.hit = xl_q15_ahead_serves(a->pending, a->rec, pos) != 0;
    d.phase_out = a->cur ^ 1, d.tab = a->tab ^ 1;
    xl_ahead_op(&d.post, XL_AHEAD_RECORD, XL_AHEAD_S_CALL, XL_AHEAD_EV_QREADY, 0);
  }
  if (d.hit)
    a->used++, a->pending = false;
  else
    xl_q15_ahead_drop(a);
  return d;
}

/* Everything of the call is enqueued. */
static inline void xl_q15_ahead_commit(XlQ15Ahead *a, const XlQ15AheadBegin *d) { a->cur = d->phase_out, a->tab = d->tab; }

/* Behind the commit of the call at `pos`: is the table of the call at xl_grid_next(pos) started on the side stream?  If `launch`: run
 * `pre`, launch xl_nco_q15_ahead_kernel for `pos` [phase_in] -> table [tab], [phase_out] on the side stream, run `post`, then
 * xl_q15_ahead_launched. */
typedef struct {
  bool launch;
  XlPos pos;
  int phase_in, phase_out, tab;
  XlAheadOps pre, post;
} XlQ15AheadNext;

static inline XlQ15AheadNext xl_q15_ahead_next(const XlQ15Ahead *a, bool option_on, XlPos pos, int planned_immature, uint32_t nclients) {
  XlQ15AheadNext n = {false, xl_grid_next(pos), a->cur, a->cur ^ 1, a->tab ^ 1, {0, {{0, 0, 0, 0}}}, {0, {{0, 0, 0, 0}}}};
  n.launch = option_on && xl_q15_ahead_may_launch(pos, planned_immature, nclients) != 0;
  if (n.launch) {
    xl_ahead_op(&n.pre, XL_AHEAD_WAIT, XL_AHEAD_S_SIDE, XL_AHEAD_EV_QREADY, 0);
    xl_ahead_op(&n.post, XL_AHEAD_RECORD, XL_AHEAD_S_SIDE, XL_AHEAD_EV_QCHAIN, 0);
  }
  return n;
}

/* `pre`, the launch and `post` of `n` have all been enqueued. */
static inline void xl_q15_ahead_launched(XlQ15Ahead *a, const XlQ15AheadNext *n) { a->pending = true, a->rec = n->pos; }

#endif /* XL_Q15_AHEAD_H_ */
