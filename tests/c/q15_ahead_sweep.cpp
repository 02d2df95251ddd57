/* A stand-alone sweep over sdr-server_amd/csrc/xl_q15_ahead.h (engine option "q15_nco"), built by tests/test_q15_nco_cpu.py under ASan
 * and UBSan and run as a process of its own.
 *
 * Part 1, position by position.  Stream positions up to the 2^31 edge, block lengths, block counts, immature counts, client counts,
 * pending or not:
 *   - a pending record serves a call if and only if trel, S and G all match (the flags word of the position is not the Q15 family's);
 *     nothing serves without a pending record;
 *   - "launch allowed" is false exactly when the plan holds immature clients, the engine has no clients, or the position would reach
 *     2^31 within two more calls of this size -- stated here in 64-bit arithmetic of its own;
 *   - whenever a launch is allowed, the predicted position xl_grid_next(pos) is the exact sum: no 32-bit product or sum wrapped, the
 *     next call at it does not re-base (xl_call_begin's test), and a call there is served by the record.
 *
 * Part 2, sequences.  The header's state and decisions driven through sequences of calls in the engine's order (xl_batch.cpp:
 * xl_call_begin's re-plan and stream hand-over through dep_ev; xl_call_q15: begin, its operations and the tabulation, the FIR-side
 * launches as readers of the table, commit, next, its operations, the launch and launched; add_client, xl_batch_plan, set_option,
 * xlating_batch_sync), the operation lists executed on the device model of ahead_model.h.  13 symbols: Q15 calls of two shapes on two
 * caller streams and the engine's, float calls on a caller stream and the engine's (they move trel and hand the stream over), a join (the
 * plan after it holds an immature client until a later re-plan), a re-plan, the option set to 0 and to 1, xlating_batch_sync.  Every
 * sequence of five, from option 0 and 1 and from trel = 0 and four calls short of 2^31; 6000 fixed-seed random sequences of 64; the
 * steady patterns.  Checked at every Q15 call:
 *   (a) every reader of the call's table comes after the tabulation that wrote it, and the table was tabulated for this call's trel, S and
 *       G from the phases the previous Q15 call committed;
 *   (b) every write of a table or phase buffer comes after its earlier writer and every earlier reader (the in-place kernel reads and
 *       writes the committed buffer);
 *   (c) the committed buffer holds the hash chain of all Q15 calls so far; a join's start phase lands there with nothing in flight;
 *   (d) `used` and `dropped` equal the sweep's own counts, and every look-ahead launched is used, dropped or still pending;
 *   (e) steady state (option 1, one shape, no immature client, from the second call on): no tabulation on the call's stream; there one
 *       wait for the chain event and one record of the ready event; on the side stream one wait for the ready event, one launch, one
 *       record of the chain event.
 * The rebuild of the all-clients launch set (xl_batch_build_all_set) drops like a re-plan and only ever runs right behind one, or in
 * front of an engine's first Q15 call: it is no symbol of its own.
 * Prints "ok <checks of part 1> <checks of part 2>" or the first failure; exit status 0 or 1. */
#include <stdint.h>
#include <stdio.h>

#include "xl_q15_ahead.h"

#include "ahead_model.h"

static uint64_t rng_state = 88172645463325252ull;
static uint64_t rnd(void) {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return rng_state;
}

static XlPos mk(uint32_t trel, uint32_t S, uint32_t G, uint32_t pad) {
  XlPos p;
  p.trel = trel, p.S = S, p.G = G, p.pad = pad;
  return p;
}

/* ---- part 1 */
static int fail(const char *what, XlPos p, int immature, uint32_t ncl) {
  printf("FAIL %s: trel %u S %u G %u pad %u immature %d clients %u\n", what, p.trel, p.S, p.G, p.pad, immature, ncl);
  return 1;
}

/* one position: the launch rule against its 64-bit statement, then the prediction */
static int one(XlPos p, int immature, uint32_t ncl, unsigned long *n) {
  const uint64_t edge = (uint64_t)1 << 31, N = (uint64_t)p.S * (uint64_t)p.G;
  const int replans = immature > 0 || ncl == 0u || (uint64_t)p.trel + N + N >= edge; /* the three cases */
  const int got = xl_q15_ahead_may_launch(p, immature, ncl);
  ++*n;
  if (got != !replans) return fail("launch rule", p, immature, ncl);
  if (got) {
    const XlPos nx = xl_grid_next(p);
    const uint64_t want = (uint64_t)p.trel + N;
    if ((uint64_t)nx.trel != want || nx.S != p.S || nx.G != p.G) return fail("prediction wrapped", p, immature, ncl);
    if (want + N >= edge) return fail("the predicted call re-bases", p, immature, ncl);
    if (!xl_q15_ahead_serves(1, nx, mk((uint32_t)want, p.S, p.G, 0u))) return fail("the record does not serve its own call", p, immature, ncl);
    ++*n;
  }
  return 0;
}

/* one record against the calls around it */
static int serves(XlPos rec, unsigned long *n) {
  const uint32_t dt[] = {0u, 1u, 0xFFFFFFFFu, 42u, rec.S, rec.S * rec.G};
  const uint32_t ds[] = {0u, 1u, 0xFFFFFFFFu, 2u};
  const uint32_t dg[] = {0u, 1u, 0xFFFFFFFFu, 7u};
  for (size_t a = 0; a < sizeof dt / sizeof dt[0]; ++a)
    for (size_t b = 0; b < sizeof ds / sizeof ds[0]; ++b)
      for (size_t c = 0; c < sizeof dg / sizeof dg[0]; ++c)
        for (uint32_t pad = 0; pad < 4u; ++pad)
          for (int pending = 0; pending < 2; ++pending) {
            const XlPos call = mk(rec.trel + dt[a], rec.S + ds[b], rec.G + dg[c], pad);
            const int want = pending && dt[a] == 0u && ds[b] == 0u && dg[c] == 0u;
            ++*n;
            if (xl_q15_ahead_serves(pending, rec, call) != want) {
              printf("FAIL serves: record (%u, %u, %u) call (%u, %u, %u) pad %u pending %d\n", rec.trel, rec.S, rec.G, call.trel, call.S,
                     call.G, pad, pending);
              return 1;
            }
          }
  return 0;
}

static int positions(unsigned long *np) {
  unsigned long n = 0;
  const uint32_t edge = 0x80000000u;
  const uint32_t Ss[] = {1u, 2u, 41u, 42u, 100u, 10001u, 15001u, 32768u, 131072u, 1048576u, 0x7FFFFFFFu};
  const uint32_t Gs[] = {1u, 2u, 3u, 8u, 64u};
  const int imm[] = {0, 1, 1024};
  const uint32_t ncls[] = {0u, 1u, 1024u};
  for (size_t si = 0; si < sizeof Ss / sizeof Ss[0]; ++si)
    for (size_t gi = 0; gi < sizeof Gs / sizeof Gs[0]; ++gi) {
      const uint32_t S = Ss[si], G = Gs[gi];
      const uint64_t N = (uint64_t)S * G;
      /* positions: the start, around edge - 2 N (where the rule turns), around edge - N, the last position an engine can hold */
      uint64_t at[16];
      size_t k = 0;
      at[k++] = 0u, at[k++] = 1u, at[k++] = N, at[k++] = edge - 1u;
      for (int d = -2; d <= 2; ++d) {
        if ((uint64_t)edge >= 2u * N + 2u) at[k++] = (uint64_t)edge - 2u * N + (uint64_t)(int64_t)d;
        if ((uint64_t)edge >= N + 2u) at[k++] = (uint64_t)edge - N + (uint64_t)(int64_t)d;
      }
      for (size_t i = 0; i < k; ++i) {
        if (at[i] >= edge) continue; /* (trel < 2^31: the engine re-plans before a call would carry it further) */
        for (size_t a = 0; a < sizeof imm / sizeof imm[0]; ++a)
          for (size_t b = 0; b < sizeof ncls / sizeof ncls[0]; ++b)
            if (one(mk((uint32_t)at[i], S, G, (uint32_t)(i & 3u)), imm[a], ncls[b], &n)) return 1;
        if (serves(mk((uint32_t)at[i], S, G, 0u), &n)) return 1;
      }
    }
  for (int i = 0; i < 200000; ++i) {
    const uint32_t S = (uint32_t)(rnd() % 262144u) + 1u, G = (uint32_t)(rnd() % 64u) + 1u;
    const uint32_t trel = (rnd() & 1u) ? (uint32_t)(rnd() % edge) : edge - 1u - (uint32_t)(rnd() % (4u * (uint64_t)S * G + 1u) % edge);
    if (one(mk(trel, S, G, (uint32_t)(rnd() & 3u)), (rnd() % 4u) == 0u ? (int)(rnd() % 5u) : 0, (rnd() % 8u) == 0u ? 0u : 1u + (uint32_t)(rnd() % 4096u), &n))
      return 1;
    if ((i & 63) == 0 && serves(mk(trel, S, G, 0u), &n)) return 1;
  }
  *np = n;
  return 0;
}

/* ---- part 2 */
enum { ENGINE = -1 };  /* XL_STREAM_ENGINE_P */
static const uint64_t kEdge = (uint64_t)1 << 31;
static const Shape kShapes[2] = {{4096u, 1u, 0u}, {4096u, 4u, 0u}};
static const uint32_t kClients = 3u; /* (an engine without clients ends its calls before xl_call_q15) */

struct Counts { /* per kind of operation and stream */
  unsigned call_tabs, call_chain_waits, call_ready_records, side_ready_waits, side_launches, side_chain_records;
};

struct Model : Streams {
  XlQ15Ahead a;
  /* the engine's side of it */
  bool option_on, dirty, joined;
  int last_stream, planned_immature;
  uint32_t trel;
  /* the device */
  Event dep, qchain, qready;
  Res tab[2], ph[2];
  /* what is true, kept by the sweep on its own */
  uint64_t committed; /* hash of the phases behind the latest Q15 call */
  bool la_out;        /* a look-ahead was launched and neither used nor dropped yet ... */
  XlPos la_pos;       /* ... for a call here */
  uint64_t launched, used, dropped;
  Counts n;
};

static void model_init(Model &m, bool option_on, uint32_t trel) {
  memset(&m, 0, sizeof(m));
  m.a = xl_q15_ahead_init();
  m.option_on = option_on, m.trel = trel, m.last_stream = ST_OWN;
  for (int i = 0; i < 2; ++i) m.tab[i].wstream = m.ph[i].wstream = -1;
  m.committed = m.ph[m.a.cur].hash = 1u;
}

static uint64_t q15_step_hash(uint64_t h, XlPos p) { return mix(step_hash(h, Shape{p.S, p.G, 0u}), p.trel); }

/* one tabulation, launch `o`: phases [pin] -> table [t], phases [pout] (pin == pout: in place), for a call at `p` */
static void tabulate(Model &m, const Op &o, int pin, int t, int pout, XlPos p) {
  CHECK(pin >= 0 && pin < 2 && t >= 0 && t < 2 && pout >= 0 && pout < 2);
  const uint64_t from = m.ph[pin].hash;
  res_read(m.ph[pin], o);
  res_write(m.tab[t], o);
  res_write(m.ph[pout], o);
  m.tab[t].hash = from, m.tab[t].trel = p.trel, m.tab[t].S = p.S, m.tab[t].G = p.G;
  m.ph[pout].hash = q15_step_hash(from, p);
}

/* the sweep's own executor of a decision's synchronisation (the engine's: xl_ahead_run with ns = nco_stream) */
static void run_ops(Model &m, const XlAheadOps &l, int s) {
  CHECK(l.n >= 0 && l.n <= XL_AHEAD_MAXOPS);
  for (int i = 0; i < l.n; ++i) {
    const XlAheadOp o = l.op[i];
    CHECK((o.stream == XL_AHEAD_S_CALL || o.stream == XL_AHEAD_S_SIDE) && (o.ev == XL_AHEAD_EV_QCHAIN || o.ev == XL_AHEAD_EV_QREADY) && o.idx == 0);
    const int st = o.stream == XL_AHEAD_S_CALL ? s : ST_NCO;
    const bool side = o.stream == XL_AHEAD_S_SIDE, chain = o.ev == XL_AHEAD_EV_QCHAIN;
    Event &e = chain ? m.qchain : m.qready;
    if (o.op == XL_AHEAD_WAIT) {
      CHECK(e.recorded && side != chain); /* (no decision asks for an event never recorded; each stream waits for the other's event) */
      wait(m, st, e);
      (side ? m.n.side_ready_waits : m.n.call_chain_waits)++;
    } else {
      CHECK(o.op == XL_AHEAD_RECORD && side == chain);
      record(m, e, st);
      (side ? m.n.side_chain_records : m.n.call_ready_records)++;
    }
  }
}

static void own_drop(Model &m) {
  if (m.la_out) m.dropped++;
  m.la_out = false;
}
/* (d) */
static void check_counts(const Model &m) {
  CHECK(m.a.used == m.used && m.a.dropped == m.dropped && xl_q15_ahead_pending(&m.a) == m.la_out);
  CHECK(m.launched == m.used + m.dropped + (m.la_out ? 1u : 0u));
}
/* the host touches `r` with its clock at `h`: nothing of it is in flight */
static void check_idle(const Res &r, const Clock &h) {
  CHECK(r.wstream < 0 || r.wtick <= h.t[r.wstream]);
  for (int s = 0; s < NST; ++s) CHECK(r.rtick[s] <= h.t[s]);
}

/* ---- the interruptions */
static void join(Model &m) { /* add_client: the new client's start phase lands in the committed buffer */
  sync_all(m);
  xl_q15_ahead_drop(&m.a), own_drop(m);
  m.dirty = m.joined = true;
  Res &r = m.ph[m.a.cur];
  CHECK(r.hash == m.committed); /* (c) */
  check_idle(r, m.st[0]);
  r.wstream = -1, memset(r.rtick, 0, sizeof(r.rtick));
  m.committed = r.hash = mix(m.committed, 0x4A4F494Eu);
  check_counts(m);
}
static void plan(Model &m) { /* xl_batch_plan */
  sync_all(m);
  xl_q15_ahead_drop(&m.a), own_drop(m);
  m.trel = 0, m.dirty = false;
  m.planned_immature = m.joined ? 1 : 0; /* (the joined client is immature in this plan and merges with the next one) */
  m.joined = false;
}
static void set_option(Model &m, bool on) { /* xlating_batch_set_option("q15_nco") */
  sync_all(m);
  xl_q15_ahead_option_set(&m.a);
  m.la_out = false, m.launched = m.used = m.dropped = 0;
  m.option_on = on;
  check_counts(m);
}
static void host_sync(Model &m) { /* xlating_batch_sync: everything the engine enqueued has happened */
  Clock h = m.st[m.last_stream];
  if (xl_q15_ahead_pending(&m.a))
    for (int i = 0; i < NST; ++i)
      if (m.st[ST_NCO].t[i] > h.t[i]) h.t[i] = m.st[ST_NCO].t[i];
  for (int i = 0; i < 2; ++i) check_idle(m.tab[i], h), check_idle(m.ph[i], h);
  check_counts(m);
}

/* ---- one call, of the Q15 family or a float one, of shape `sh` on caller stream ST_A / ST_B or ENGINE */
static void call(Model &m, bool q15, Shape sh, int s_in, bool replan) {
  const uint32_t N = sh.S * sh.G;
  /* xl_call_begin: re-base, re-plan, the stream, ordered behind the previous call's */
  if ((uint64_t)m.trel + N >= kEdge) m.dirty = true;
  if (m.dirty || replan) plan(m);
  const int s = s_in != ENGINE ? s_in : ST_OWN;
  if (s != m.last_stream) {
    record(m, m.dep, m.last_stream);
    wait(m, s, m.dep);
  }
  m.last_stream = s;
  if (!q15) { /* a float call: its launches on `s`; no Q15 buffer touched, the Q15 look-ahead kept (its record no longer serves) */
    (void)launch(m, s);
    m.trel += N;
    check_counts(m);
    return;
  }
  /* xl_call_q15 */
  const XlPos pos = mk(m.trel, sh.S, sh.G, 0u);
  const XlQ15Ahead before = m.a;
  const bool want_hit = m.option_on && m.la_out && m.la_pos.trel == pos.trel && m.la_pos.S == pos.S && m.la_pos.G == pos.G;
  CHECK(before.pending == m.la_out);
  if (m.la_out) want_hit ? m.used++ : m.dropped++;
  m.la_out = false;
  const XlQ15AheadBegin d = xl_q15_ahead_begin(&m.a, m.option_on, pos);
  CHECK(d.hit == want_hit && d.in_place == !m.option_on && d.phase_in == before.cur);
  CHECK(m.option_on ? (d.phase_out == (before.cur ^ 1) && d.tab == (before.tab ^ 1)) : (d.phase_out == before.cur && d.tab == before.tab));
  check_counts(m);
  run_ops(m, d.pre, s);
  if (!d.hit) {
    tabulate(m, launch(m, s), d.phase_in, d.tab, d.phase_out, pos);
    m.n.call_tabs++;
  }
  run_ops(m, d.post, s);
  { /* the matrix, FIR and wide launches: readers of the call's table.  (a): it is this call's */
    const Op rd = launch(m, s);
    const Res &t = m.tab[d.tab];
    res_read(m.tab[d.tab], rd);
    CHECK(t.hash == m.committed && t.trel == pos.trel && t.S == pos.S && t.G == pos.G);
  }
  xl_q15_ahead_commit(&m.a, &d);
  m.trel += N;
  m.committed = q15_step_hash(m.committed, pos);
  CHECK(m.a.cur == d.phase_out && m.a.tab == d.tab);
  CHECK(m.ph[m.a.cur].hash == m.committed); /* (c) */
  const XlQ15AheadNext nx = xl_q15_ahead_next(&m.a, m.option_on, pos, m.planned_immature, kClients);
  CHECK(nx.launch == (m.option_on && m.planned_immature == 0 && (uint64_t)pos.trel + 2u * (uint64_t)N < kEdge));
  if (nx.launch) {
    CHECK(nx.pos.trel == m.trel && nx.pos.S == sh.S && nx.pos.G == sh.G);
    CHECK(nx.phase_in == m.a.cur && nx.phase_out == (m.a.cur ^ 1) && nx.tab == (m.a.tab ^ 1));
    run_ops(m, nx.pre, s);
    tabulate(m, launch(m, ST_NCO), nx.phase_in, nx.tab, nx.phase_out, nx.pos);
    m.n.side_launches++;
    run_ops(m, nx.post, s);
    xl_q15_ahead_launched(&m.a, &nx);
    CHECK(m.a.pending && m.a.rec.trel == nx.pos.trel && m.a.rec.S == nx.pos.S && m.a.rec.G == nx.pos.G);
    m.la_out = true, m.la_pos = nx.pos, m.launched++;
  } else {
    CHECK(nx.pre.n == 0 && nx.post.n == 0);
  }
  CHECK(m.ph[m.a.cur].hash == m.committed); /* (the look-ahead left the committed phases alone) */
  check_counts(m);
}

/* ---- the alphabet */
enum { NSYM = 13, SYM_FLOAT = 6, SYM_JOIN = 8, SYM_PLAN, SYM_OPT0, SYM_OPT1, SYM_SYNC };
static const char *const kSymNames[NSYM] = {"qA0", "qB0", "qE0", "qA1", "qB1", "qE1", "fA", "fE", "J", "P", "O0", "O1", "Y"};
static void apply(Model &m, bool &replan, int sym) {
  static const int streams[3] = {ST_A, ST_B, ENGINE};
  if (sym < SYM_FLOAT)
    call(m, true, kShapes[sym / 3], streams[sym % 3], replan), replan = false;
  else if (sym < SYM_JOIN)
    call(m, false, kShapes[0], streams[sym == SYM_FLOAT ? 0 : 2], replan), replan = false;
  else if (sym == SYM_JOIN)
    join(m);
  else if (sym == SYM_PLAN)
    replan = true; /* (in front of the next call) */
  else if (sym == SYM_SYNC)
    host_sync(m);
  else
    set_option(m, sym == SYM_OPT1);
}

static void dfs(const Model &m, bool replan, int depth, size_t ctx_len) {
  if (depth == 5) return;
  for (int sym = 0; sym < NSYM; ++sym) {
    Model n = m;
    bool r = replan;
    snprintf(g_ctx + ctx_len, sizeof(g_ctx) - ctx_len, " %s", kSymNames[sym]);
    apply(n, r, sym);
    dfs(n, r, depth + 1, ctx_len + strlen(g_ctx + ctx_len));
  }
}

/* (e): per call from the second on, counts read off xl_call_q15 */
static void steady(void) {
  static const int patterns[4][2] = {{ST_A, ST_A}, {ST_B, ST_B}, {ENGINE, ENGINE}, {ST_A, ST_B}};
  for (int p = 0; p < 4; ++p)
    for (int sh = 0; sh < 2; ++sh) {
      Model m;
      model_init(m, true, 0u);
      for (int k = 0; k < 40; ++k) {
        snprintf(g_ctx, sizeof(g_ctx), "steady pattern=%d shape=%d call=%d", p, sh, k);
        memset(&m.n, 0, sizeof(m.n));
        call(m, true, kShapes[sh], patterns[p][k & 1], false);
        CHECK(m.n.call_tabs == (k == 0 ? 1u : 0u) && m.n.call_chain_waits == (k == 0 ? 0u : 1u) && m.n.call_ready_records == 1u);
        CHECK(m.n.side_ready_waits == 1u && m.n.side_launches == 1u && m.n.side_chain_records == 1u);
      }
      CHECK(m.used == 39u && m.dropped == 0u && m.la_out);
      host_sync(m);
    }
}

int main(void) {
  unsigned long n = 0;
  if (positions(&n)) return 1;
  steady();
  for (int opt = 0; opt < 2; ++opt)
    for (int late = 0; late < 2; ++late) {
      Model m;
      /* four calls of the smaller shape short of 2^31: the third launches no look-ahead, the fourth re-bases */
      model_init(m, opt != 0, late ? (uint32_t)(kEdge - 4u * 4096u) : 0u);
      const int len = snprintf(g_ctx, sizeof(g_ctx), "exhaustive option=%d trel=%u:", opt, m.trel);
      dfs(m, false, 0, (size_t)len);
    }
  for (int run = 0; run < 6000; ++run) {
    Model m;
    bool replan = false;
    model_init(m, run % 2 != 0, (run / 2) % 4 == 3 ? (uint32_t)(kEdge - (1u + (uint32_t)(rnd() % 40u)) * 4096u) : 0u);
    const unsigned sticky = (unsigned)(rnd() % 4u); /* how strongly the sequence repeats its previous Q15 call: 0 not at all */
    int prev = (int)(rnd() % SYM_FLOAT);
    for (int k = 0; k < 64; ++k) {
      int sym = rnd() % 5u == 0 ? SYM_FLOAT + (int)(rnd() % (NSYM - SYM_FLOAT)) : (int)(rnd() % SYM_FLOAT);
      if (sym < SYM_FLOAT && sticky && rnd() % 4u < sticky) sym = prev;
      if (sym < SYM_FLOAT) prev = sym;
      snprintf(g_ctx, sizeof(g_ctx), "random run=%d step=%d %s", run, k, kSymNames[sym]);
      apply(m, replan, sym);
    }
  }
  printf("ok %lu %lu\n", n, g_checks);
  return 0;
}
