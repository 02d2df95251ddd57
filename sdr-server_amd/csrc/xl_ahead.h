/* xl_ahead.h -- the float families' phase look-ahead (xl_batch.cpp, stages xl_call_table .. xl_call_finish): its state and every decision,
 * plain C without HIP, in the style of xl_q15_ahead.h.  tests/c/ahead_sweep.cpp drives these functions through sequences of calls against a
 * model of streams and events under ASan and UBSan (tests/test_ahead_cpu.py); the engine calls them, executes the synchronisation they
 * return (XlAheadOps) and decides nothing of this on its own.
 *
 * The ring.  The engine owns XL_NTAB phase tables d_phtab[] and XL_NTAB phase buffers d_phase[], with one event pair per table,
 * ev_chain[] / ev_done[]; this state holds indices into them.
 *   - d_phase[pcur] holds the committed running phases: those behind the latest float call.  Table [tab] is that call's.
 *   - Call k reads table [tab + 1]; its tabulation reads d_phase[pcur] and writes that table and d_phase[pcur + 1], which the call commits.
 *     Both indices advance by one per float call, whoever tabulated: a hit and a miss leave the ring in the same position.
 *   - Look-ahead: tables [tab + 1 .. tab + spec_n] (phases [pcur + 1 ..]) hold the next spec_n calls, tabulated for calls of spec_S samples x
 *     spec_G blocks with position flags spec_flags, each right behind the one before.  They come from the latest call's own launches (the NCO
 *     role: spec_n = 1, spec_on_side = false, in stream order on the call's stream), or from ONE chain launch on a side stream (spec_n <=
 *     XL_AHEAD_MAXCALLS, spec_on_side = true), whose completion is ev_chain[spec_ev].  A call of another shape, a Q15 call (it moves the stream
 *     position), a join and a re-plan drop them; the committed phases are never touched by a look-ahead.
 *   - A chain launch is made by a side-stream call that has no look-ahead table left behind it.  It covers min(chain_calls, chain_ahead)
 *     calls; chain_ahead is 1 behind a wrong guess and doubles with every launch, up to XL_AHEAD_MAXCALLS: 1, 2, 4, 4, ...  With XL_NTAB =
 *     2 XL_AHEAD_MAXCALLS a launch for calls k+1 .. k+n writes tables last read by calls k+n-XL_NTAB+1 .. k+n-XL_NTAB+n, at the latest the call
 *     that made the previous full launch.
 *   - Readers before writers.  ev_done[t], where ev_done_valid[t], stands behind every launch that read table t -- and, calls being ordered
 *     one behind the other, behind every earlier call's.  tab_call[t] is the number (calls processed + 1) of the latest call that read table t
 *     since a side stream was first used, done_call / done_tab the latest call that recorded an ev_done.  A chain launch waits for
 *     ev_done[done_tab] when done_call is not older than the latest reader of the tables it writes; else it is ordered behind the call's stream
 *     on the spot.  Side-stream calls record ev_done only when they launch a chain, other calls always once a side stream has been used
 *     (side_used), and never before: a launch that carries an event keeps the queue ~8 us from starting the next one.
 *   - Writers before readers.  The first launch of a call that reads a side-stream table waits for ev_chain[spec_ev], once per launch and
 *     stream: waited_* remembers which stream has waited for which event since that event was last recorded.
 *   - Chain launches follow each other through the phase buffers: on one side stream in stream order, across two by an event; the launch that
 *     follows a table tabulated on the call's stream (tab_from_s) is ordered behind that stream.
 * A stream is an opaque identity here; which side stream a call uses, and its handle, are the engine's. */
#ifndef XL_AHEAD_H_
#define XL_AHEAD_H_

#include <stdbool.h>
#include <stdint.h>
#include <string.h>

#define XL_AHEAD_MAXCALLS 4 /* most calls per chain launch: XL_CHAIN_MAXCALLS of xl_device.h (xl_batch.cpp asserts it) */
#define XL_NTAB (2 * XL_AHEAD_MAXCALLS)
static inline int xl_nx(int i) { return (i + 1) % XL_NTAB; }

/* One synchronisation operation: wait for / record event `ev` (of index idx, for the per-table events) on stream `stream`. */
enum { XL_AHEAD_WAIT, XL_AHEAD_RECORD };
enum { XL_AHEAD_S_CALL, XL_AHEAD_S_SIDE, XL_AHEAD_S_PREV_SIDE }; /* the call's stream, its side stream, the previous chain launch's */
enum { XL_AHEAD_EV_DEP, XL_AHEAD_EV_CHAIN, XL_AHEAD_EV_DONE,     /* the engine's dep_ev (re-recorded at will), ev_chain[idx], ev_done[idx] */
       XL_AHEAD_EV_QCHAIN, XL_AHEAD_EV_QREADY };                 /* ev_qchain, ev_qready: xl_q15_ahead.h's alone, side stream nco_stream */
typedef struct {
  uint8_t op, stream, ev, idx;
} XlAheadOp;
#define XL_AHEAD_MAXOPS 5 /* the most any decision returns: two orderings and a wait (xl_ahead_chain) */
typedef struct {
  int n;
  XlAheadOp op[XL_AHEAD_MAXOPS];
} XlAheadOps;

static inline void xl_ahead_op(XlAheadOps *l, int op, int stream, int ev, int idx) {
  const XlAheadOp o = {(uint8_t)op, (uint8_t)stream, (uint8_t)ev, (uint8_t)idx};
  l->op[l->n++] = o;
}
/* `to` is ordered behind everything enqueued on `from` so far */
static inline void xl_ahead_order(XlAheadOps *l, int from, int to) {
  xl_ahead_op(l, XL_AHEAD_RECORD, from, XL_AHEAD_EV_DEP, 0);
  xl_ahead_op(l, XL_AHEAD_WAIT, to, XL_AHEAD_EV_DEP, 0);
}

typedef struct {
  int pcur, tab;
  int spec_n, spec_ev;
  uint32_t spec_S, spec_G, spec_flags;
  bool spec_on_side;
  bool side_used; /* a chain launch was made since the last reset */
  bool ev_done_valid[XL_NTAB];
  uint64_t tab_call[XL_NTAB], done_call;
  int done_tab;
  bool waited_valid;
  int waited_ev;
  const void *waited_stream;
  int chain_calls; /* engine option "nco_calls_per_launch", 1 .. XL_AHEAD_MAXCALLS */
  int chain_ahead; /* what the next launch covers at most.  Irregular block lengths, one block per call, 1024 clients: 134 us per call with
                      four calls ahead every time (profiles/r05_ragged_blocks.txt) against 39.5 us for constant lengths: a dropped look-ahead
                      is chain work the call has to wait out */
} XlAhead;

static inline XlAhead xl_ahead_init(void) {
  XlAhead a;
  memset(&a, 0, sizeof(a));
  a.chain_calls = a.chain_ahead = XL_AHEAD_MAXCALLS;
  return a;
}

/* Forget the tables tabulated ahead.  The caller has made sure that a chain launch still writing them is waited for: every stream
 * synchronised (join, re-plan), or the ops of xl_ahead_pending_wait on the stream that goes on. */
static inline void xl_ahead_drop(XlAhead *a) { a->spec_n = 0; }

/* The masked stream pair is re-created, every stream synchronised: no event recorded so far is needed again. */
static inline void xl_ahead_reset(XlAhead *a) {
  memset(a->ev_done_valid, 0, sizeof(a->ev_done_valid));
  memset(a->tab_call, 0, sizeof(a->tab_call));
  a->done_call = 0;
  a->side_used = false;
}

/* In front of a launch that overwrites, or moves the stream past, a look-ahead that may still be running on a side stream. */
static inline XlAheadOps xl_ahead_pending_wait(const XlAhead *a) {
  XlAheadOps l = {0, {{0, 0, 0, 0}}};
  if (a->spec_n > 0 && a->spec_on_side) xl_ahead_op(&l, XL_AHEAD_WAIT, XL_AHEAD_S_CALL, XL_AHEAD_EV_CHAIN, a->spec_ev);
  return l;
}

/* A float call of G blocks of S samples with position flags `flags` on `stream` begins. */
typedef struct {
  bool hit;        /* its table was tabulated ahead.  Else: run `pre`, then tabulate d_phase[phase_in] -> table [tab], d_phase[pcur] on the call's stream */
  bool tab_from_s; /* the table is (or will be) written on the call's own stream */
  bool chain_wait; /* the table comes from a side stream this stream has not waited for: ev_chain[chain_ev] before the first reader */
  bool fuse;       /* the call's launches tabulate the next call's table (the NCO role) */
  int tab, phase_in, pcur; /* pcur: the phases the call commits */
  int chain_ev, spec_left; /* spec_left: look-ahead calls that stay valid behind this one */
  XlAheadOps pre;
} XlAheadBegin;

static inline XlAheadBegin xl_ahead_begin(XlAhead *a, uint32_t S, uint32_t G, uint32_t flags, const void *stream, bool side, bool nofuse) {
  XlAheadBegin d;
  memset(&d, 0, sizeof(d));
  d.tab = xl_nx(a->tab), d.phase_in = a->pcur, d.pcur = xl_nx(a->pcur), d.chain_ev = a->spec_ev;
  d.tab_from_s = true;
  d.hit = a->spec_n > 0 && a->spec_S == S && a->spec_G == G && a->spec_flags == flags;
  if (d.hit) {
    d.tab_from_s = !a->spec_on_side;
    d.chain_wait = a->spec_on_side && !(a->waited_valid && a->waited_ev == d.chain_ev && a->waited_stream == stream);
    d.spec_left = a->spec_n - 1;
  } else {
    d.pre = xl_ahead_pending_wait(a);  /* (it runs on these very buffers) */
    if (a->spec_n > 0) a->chain_ahead = 1; /* (a wrong guess: look less far ahead until the guesses hold again) */
    if (a->ev_done_valid[d.tab]) xl_ahead_op(&d.pre, XL_AHEAD_WAIT, XL_AHEAD_S_CALL, XL_AHEAD_EV_DONE, d.tab); /* (same stream normally) */
  }
  /* (with a look-ahead table still in hand the launches carry no NCO role: the call after this one has its table) */
  d.fuse = !side && d.spec_left == 0 && !nofuse;
  return d; /* the engine drops the look-ahead (xl_ahead_drop) once the table is in hand */
}

/* The call's stream has waited for ev_chain[d->chain_ev]. */
static inline void xl_ahead_chain_waited(XlAhead *a, XlAheadBegin *d, const void *stream) {
  d->chain_wait = false;
  a->waited_valid = true, a->waited_ev = d->chain_ev, a->waited_stream = stream;
}

/* A side-stream call with spec_left == 0 launches the chain kernel for the next n calls, same shape assumed: run `pre`, then the launch on
 * the side stream, d_phase[phase_in] -> tables tab[i] and phases phase[i], completion = ev_chain[ev].  side_changed: the side stream is not
 * the previous chain launch's. */
typedef struct {
  int n, ev, phase_in;
  int tab[XL_AHEAD_MAXCALLS], phase[XL_AHEAD_MAXCALLS];
  XlAheadOps pre;
} XlAheadChain;

static inline XlAheadChain xl_ahead_chain(XlAhead *a, const XlAheadBegin *d, bool side_changed) {
  XlAheadChain c;
  uint64_t need = 0; /* the latest call that read one of the tables written */
  memset(&c, 0, sizeof(c));
  if (side_changed && a->side_used) xl_ahead_order(&c.pre, XL_AHEAD_S_PREV_SIDE, XL_AHEAD_S_SIDE);
  a->side_used = true;
  if (d->tab_from_s) xl_ahead_order(&c.pre, XL_AHEAD_S_CALL, XL_AHEAD_S_SIDE);
  c.n = a->chain_calls < a->chain_ahead ? a->chain_calls : a->chain_ahead;
  c.n = c.n < 1 ? 1 : (c.n > XL_AHEAD_MAXCALLS ? XL_AHEAD_MAXCALLS : c.n);
  a->chain_ahead = 2 * a->chain_ahead < XL_AHEAD_MAXCALLS ? 2 * a->chain_ahead : XL_AHEAD_MAXCALLS; /* (the previous launch's calls were all used) */
  c.phase_in = d->pcur, c.ev = xl_nx(d->tab);
  for (int i = 0, t = d->tab, p = d->pcur; i < c.n; ++i) {
    c.tab[i] = t = xl_nx(t), c.phase[i] = p = xl_nx(p);
    if (a->tab_call[t] > need) need = a->tab_call[t];
  }
  /* one wait for the latest reader covers the earlier ones (every wait is a queue packet of its own, ~4 us in front of the launch) */
  if (need != 0 && a->done_call >= need)
    xl_ahead_op(&c.pre, XL_AHEAD_WAIT, XL_AHEAD_S_SIDE, XL_AHEAD_EV_DONE, a->done_tab);
  else if (need != 0 && !d->tab_from_s) /* (tab_from_s: already ordered behind the call's stream) */
    xl_ahead_order(&c.pre, XL_AHEAD_S_CALL, XL_AHEAD_S_SIDE);
  a->waited_valid = false; /* (ev_chain[ev] stands for this launch from now on) */
  return c;
}

/* Does the call record ev_done[tab] behind its last launch?  launched_n: XlAheadChain::n, 0 without a chain launch. */
static inline bool xl_ahead_want_done(const XlAhead *a, bool side, int launched_n) {
  return (side || a->side_used) && (!side || launched_n > 0);
}

/* Everything of the call is enqueued (ev_done[d->tab] too, if wanted).  call_no: calls processed + 1; nco_fused: a launch carried the NCO role. */
static inline void xl_ahead_finish(XlAhead *a, const XlAheadBegin *d, uint64_t call_no, bool side, bool want_done, int launched_n,
                                   bool nco_fused, uint32_t S, uint32_t G, uint32_t flags) {
  if (side || a->side_used) a->tab_call[d->tab] = call_no;
  a->ev_done_valid[d->tab] = want_done;
  if (want_done) a->done_call = call_no, a->done_tab = d->tab;
  a->pcur = d->pcur, a->tab = d->tab;
  if (launched_n > 0) {
    a->spec_n = launched_n, a->spec_on_side = true, a->spec_ev = xl_nx(d->tab);
  } else if (d->spec_left > 0) {
    a->spec_n = d->spec_left; /* (same launch, same event) */
  } else if (nco_fused) {
    a->spec_n = 1, a->spec_on_side = false;
  } /* else (tiny call, or the tuning switch): the next call tabulates for itself */
  a->spec_S = S, a->spec_G = G, a->spec_flags = flags;
}

#endif /* XL_AHEAD_H_ */
