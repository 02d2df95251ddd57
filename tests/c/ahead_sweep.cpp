// tests/c/ahead_sweep.cpp -- stand-alone host program (its own main; tests/test_ahead_cpu.py builds it with ASan + UBSan and runs it):
// the float families' phase look-ahead (csrc/xl_ahead.h) driven through sequences of calls in the order of the engine's stages
// (xl_batch.cpp: xl_call_begin's stream hand-over, xl_call_q15's drop, xl_call_table, xl_call_chain, the launches with xl_call_chain_wait
// in front of the first reader, xl_call_finish; add_client, xl_batch_plan, xl_batch_reserve_cus), against the device model of
// ahead_model.h, which the Q15 look-ahead's sweep shares: streams as vector clocks, events, and phase tables and buffers that remember
// their writer, their readers and what they hold (a buffer: a hash chained over every float call's shape).
// Checked for every call: (a) its launches read a table written before them, for this call's position and shape, from the phases the
// previous call committed; (b) every write of a table or buffer comes after its earlier writer and readers; (c) the committed buffer holds
// the chain of all float calls so far; (d), (e) the steady-state and ev_done counts of steady() below.
// A fused call is modelled as the direct launches are enqueued: the chain wait, then ONE launch that reads the table and carries the
// NCO role.  Prints "ok <checks>".
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "xl_ahead.h"

#include "ahead_model.h"

enum { ENGINE = -1 };  // XL_STREAM_ENGINE_P

static const Shape kShapes[2] = {{4096u, 1u, 0u}, {4096u, 4u, 1u}};

struct Counts {
  unsigned chain_waits, done_records, launches, launched_calls, hits, misses, chain_pre_ops, chain_pre_done_waits;
  int last_n;
};

struct Model : Streams {
  XlAhead a;
  // the engine's side of it
  int last_stream, last_nco;  // stream indices; last_nco -1: none
  bool masked, dirty, nofuse;
  uint64_t ncalls;
  uint32_t trel;
  // the device (its streams: Streams::st)
  Event dep, chain[XL_NTAB], done[XL_NTAB];
  Res tab[XL_NTAB], ph[XL_NTAB];
  // what is true
  uint64_t committed;  // hash of the phases behind the latest float call
  Counts n;
};

static void model_init(Model &m, int chain_calls, bool masked, bool nofuse) {
  memset(&m, 0, sizeof(m));
  m.a = xl_ahead_init();
  m.a.chain_calls = chain_calls;
  m.last_stream = ST_OWN, m.last_nco = -1, m.masked = masked, m.nofuse = nofuse;
  for (int i = 0; i < XL_NTAB; ++i) m.tab[i].wstream = m.ph[i].wstream = -1;
  m.committed = m.ph[m.a.pcur].hash = 1u;
}

// one tabulation inside launch `o`: d_phase[pin] -> table [t], d_phase[pout], for a call of `sh` at `trel`
static void tabulate(Model &m, const Op &o, int pin, int t, int pout, uint32_t trel, Shape sh) {
  CHECK(pin >= 0 && pin < XL_NTAB && t >= 0 && t < XL_NTAB && pout >= 0 && pout < XL_NTAB && pin != pout);
  res_read(m.ph[pin], o);
  res_write(m.tab[t], o);
  res_write(m.ph[pout], o);
  m.tab[t].hash = m.ph[pin].hash, m.tab[t].trel = trel, m.tab[t].S = sh.S, m.tab[t].G = sh.G, m.tab[t].flags = sh.flags;
  m.ph[pout].hash = step_hash(m.ph[pin].hash, sh);
}

// the sweep's own executor of a decision's synchronisation (the engine's: xl_ahead_run)
static void run_ops(Model &m, const XlAheadOps &l, int s, int ns) {
  CHECK(l.n >= 0 && l.n <= XL_AHEAD_MAXOPS);
  for (int i = 0; i < l.n; ++i) {
    const XlAheadOp o = l.op[i];
    const int st = o.stream == XL_AHEAD_S_CALL ? s : (o.stream == XL_AHEAD_S_SIDE ? ns : m.last_nco);
    CHECK(o.stream <= XL_AHEAD_S_PREV_SIDE && st >= 0 && st < NST && o.idx < XL_NTAB && o.ev <= XL_AHEAD_EV_DONE);
    Event &e = o.ev == XL_AHEAD_EV_DEP ? m.dep : (o.ev == XL_AHEAD_EV_CHAIN ? m.chain[o.idx] : m.done[o.idx]);
    if (o.op == XL_AHEAD_WAIT) {
      CHECK(e.recorded);  // (no decision asks for an event that was never recorded)
      wait(m, st, e);
      if (o.ev == XL_AHEAD_EV_CHAIN && o.stream == XL_AHEAD_S_CALL) m.n.chain_waits++;
    } else {
      CHECK(o.op == XL_AHEAD_RECORD && o.ev == XL_AHEAD_EV_DEP);  // (the per-table events are recorded by the launches and by finish)
      record(m, e, st);
    }
  }
}

// ---- the interruptions
static void join(Model &m) {  // add_client: the new client's phase lands in the committed buffer
  sync_all(m);
  xl_ahead_drop(&m.a);
  m.dirty = true;
  m.committed = m.ph[m.a.pcur].hash = mix(m.committed, 0x4A4F494Eu);
}
static void plan(Model &m, bool recreate_pair) {  // xl_batch_plan (+ xl_batch_reserve_cus)
  sync_all(m);
  xl_ahead_drop(&m.a);
  m.trel = 0, m.dirty = false;
  if (recreate_pair) {
    m.last_nco = -1, m.last_stream = ST_OWN;
    xl_ahead_reset(&m.a);
  }
}

// ---- one call: kind 0 side, 1 fused, 2 Q15; on caller stream ST_A / ST_B or ENGINE
static const void *stream_id(int s) { return (const void *)(uintptr_t)(0x1000 + s); }

static void call(Model &m, int kind, Shape sh, int s_in, int replan) {
  const bool side = kind == 0;
  if (m.dirty || replan) plan(m, replan == 2);
  // xl_call_begin: the stream, ordered behind the previous call's
  const int s = s_in != ENGINE ? s_in : ((side && m.masked) ? ST_CS_MASKED : ST_OWN);
  if (s != m.last_stream) {
    record(m, m.dep, m.last_stream);
    wait(m, s, m.dep);
  }
  m.last_stream = s;
  const uint32_t N = sh.S * sh.G;
  if (kind == 2) {  // xl_call_q15: the float phases stay, the stream position moves
    run_ops(m, xl_ahead_pending_wait(&m.a), s, -1);
    xl_ahead_drop(&m.a);
    (void)launch(m, s);
    m.trel += N, m.ncalls++;
    CHECK(m.ph[m.a.pcur].hash == m.committed);  // (c)
    return;
  }
  // xl_call_table
  XlAheadBegin d = xl_ahead_begin(&m.a, sh.S, sh.G, sh.flags, stream_id(s), side, m.nofuse);
  CHECK(d.tab == xl_nx(m.a.tab) && d.phase_in == m.a.pcur && d.pcur == xl_nx(m.a.pcur));
  CHECK(d.hit || (d.tab_from_s && !d.chain_wait && d.spec_left == 0));
  CHECK(d.fuse == (!side && d.spec_left == 0 && !m.nofuse));
  if (d.hit) {
    m.n.hits++;
    CHECK(d.pre.n == 0);
  } else {
    m.n.misses++;
    run_ops(m, d.pre, s, -1);
    tabulate(m, launch(m, s), d.phase_in, d.tab, d.pcur, m.trel, sh);
  }
  xl_ahead_drop(&m.a);
  // xl_call_chain
  XlAheadChain ch;
  memset(&ch, 0, sizeof(ch));
  if (side && d.spec_left == 0) {
    const int ns = (s == ST_CS_MASKED && m.masked) ? ST_NCO_MASKED : ST_NCO;
    const int before = m.a.chain_ahead;
    ch = xl_ahead_chain(&m.a, &d, ns != m.last_nco);
    int want_n = m.a.chain_calls < before ? m.a.chain_calls : before;
    want_n = want_n < 1 ? 1 : (want_n > XL_AHEAD_MAXCALLS ? XL_AHEAD_MAXCALLS : want_n);
    CHECK(ch.n == want_n && ch.ev == xl_nx(d.tab) && ch.phase_in == d.pcur);
    CHECK(m.a.chain_ahead == (2 * before < XL_AHEAD_MAXCALLS ? 2 * before : XL_AHEAD_MAXCALLS) && !m.a.waited_valid);
    m.n.chain_pre_ops += (unsigned)ch.pre.n;
    for (int i = 0; i < ch.pre.n; ++i) m.n.chain_pre_done_waits += ch.pre.op[i].ev == XL_AHEAD_EV_DONE ? 1u : 0u;
    run_ops(m, ch.pre, s, ns);
    m.last_nco = ns;
    const Op o = launch(m, ns);
    uint32_t trel = m.trel;
    for (int i = 0, t = d.tab, p = d.pcur; i < ch.n; ++i) {
      t = xl_nx(t), trel += N;
      CHECK(ch.tab[i] == t && ch.phase[i] == xl_nx(p));
      tabulate(m, o, p, ch.tab[i], ch.phase[i], trel, sh);
      p = ch.phase[i];
    }
    record(m, m.chain[ch.ev], ns);  // (the launch records its completion)
    m.n.launches++, m.n.launched_calls += (unsigned)ch.n, m.n.last_n = ch.n;
  }
  // xl_call_direct ..: the first reader waits for a side-stream table, the launches read it, a fused call's carry the NCO role
  const bool want_done = xl_ahead_want_done(&m.a, side, ch.n);
  CHECK(want_done == (side ? ch.n > 0 : m.last_nco >= 0));  // (d), (e): only chain-launching side calls; fused calls iff a side stream was used
  if (d.chain_wait) {
    CHECK(m.chain[d.chain_ev].recorded);
    wait(m, s, m.chain[d.chain_ev]);
    m.n.chain_waits++;
    xl_ahead_chain_waited(&m.a, &d, stream_id(s));
    CHECK(!d.chain_wait);
  }
  const Op rd = launch(m, s);
  res_read(m.tab[d.tab], rd);
  {  // (a): the table is this call's
    const Res &t = m.tab[d.tab];
    CHECK(t.hash == m.committed && t.trel == m.trel && t.S == sh.S && t.G == sh.G && t.flags == sh.flags);
  }
  if (d.fuse) tabulate(m, rd, d.pcur, xl_nx(d.tab), xl_nx(d.pcur), m.trel + N, sh);
  // xl_call_finish
  if (want_done) record(m, m.done[d.tab], s), m.n.done_records++;
  xl_ahead_finish(&m.a, &d, m.ncalls + 1, side, want_done, ch.n, d.fuse, sh.S, sh.G, sh.flags);
  m.trel += N, m.ncalls++;
  m.committed = step_hash(m.committed, sh);
  CHECK(m.a.pcur == d.pcur && m.a.tab == d.tab);
  CHECK(m.ph[m.a.pcur].hash == m.committed);  // (c): the committed buffer is the one written for this call
  CHECK(m.a.spec_n == (ch.n > 0 ? ch.n : (d.spec_left > 0 ? d.spec_left : (d.fuse ? 1 : 0))));
}

// ---- the alphabet: 12 float calls (side / fused x two shapes x A / B / ENGINE), 3 Q15 calls, 3 interruptions in front of the next call
enum { NSYM = 18 };
static const char *const kSymNames[NSYM] = {"sA0", "sB0", "sE0", "sA1", "sB1", "sE1", "fA0", "fB0", "fE0",
                                            "fA1", "fB1", "fE1", "qA",  "qB",  "qE",  "J",   "P",   "M"};
struct Pending {
  int replan;  // 0 none, 1 re-plan, 2 re-plan that re-creates the masked pair
};
static void apply(Model &m, Pending &pd, int sym) {
  static const int streams[3] = {ST_A, ST_B, ENGINE};
  if (sym < 12)
    call(m, sym / 6, kShapes[(sym / 3) % 2], streams[sym % 3], pd.replan), pd.replan = 0;
  else if (sym < 15)
    call(m, 2, kShapes[0], streams[sym - 12], pd.replan), pd.replan = 0;
  else if (sym == 15)
    join(m);
  else
    pd.replan = sym == 16 ? (pd.replan > 1 ? pd.replan : 1) : 2;
}

static int g_depth_max;
static void dfs(const Model &m, Pending pd, int depth, size_t ctx_len) {
  if (depth == g_depth_max) return;
  for (int sym = 0; sym < NSYM; ++sym) {
    Model n = m;
    Pending p = pd;
    snprintf(g_ctx + ctx_len, sizeof(g_ctx) - ctx_len, " %s", kSymNames[sym]);
    apply(n, p, sym);
    dfs(n, p, depth + 1, ctx_len + strlen(g_ctx + ctx_len));
  }
}

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;  // fixed seed (xorshift64*)
static uint32_t rnd(uint32_t n) {
  g_rng ^= g_rng >> 12, g_rng ^= g_rng << 25, g_rng ^= g_rng >> 27;
  return (uint32_t)((g_rng * 0x2545F4914F6CDD1Dull) >> 33) % n;
}

// (d), (e): the counts of the steady patterns, read off the engine's code
static void steady(int cc, bool masked) {
  const int streams[3] = {ST_A, ST_B, ENGINE};
  for (int si = 0; si < 3; ++si) {
    Model m;
    model_init(m, cc, masked, false);
    snprintf(g_ctx, sizeof(g_ctx), "steady cc=%d masked=%d stream=%d", cc, (int)masked, si);
    // a fresh engine: the first call misses, every later one hits; every launch covers min(chain_calls, 4) calls
    for (int k = 0; k < 41; ++k) {
      const unsigned launches = m.n.launches;
      call(m, 0, kShapes[0], streams[si], 0);
      if (m.n.launches > launches) CHECK(m.n.last_n == cc);
    }
    CHECK(m.n.misses == 1u && m.n.hits == 40u);
    CHECK(m.n.launches == (unsigned)(40 / cc + 1) && m.n.launched_calls == m.n.launches * (unsigned)cc);
    CHECK(m.n.chain_waits == m.n.launches - (40 % cc == 0 ? 1u : 0u));  // one ev_chain wait per launch (the latest one's is still to come)
    CHECK(m.n.done_records == m.n.launches);                            // only chain-launching calls record ev_done
    // a launch's own synchronisation: the first follows a table made on the call's stream (one ordering: two ops); the later ones wait
    // for one ev_done as soon as the tables they write have had readers (calls 1 .. 8 - cc .. have written fresh slots)
    CHECK(m.n.chain_pre_ops == 2u + m.n.chain_pre_done_waits);
    {
      unsigned fresh = 0;  // launches behind the first whose tables nobody has read yet
      for (int k = cc; k <= 40; k += cc)
        if (k + cc < XL_NTAB) fresh++;
      CHECK(m.n.chain_pre_done_waits == m.n.launches - 1u - fresh);
    }
    // a call of another shape: a miss, and the launches cover 1, 2, 4, 4, ... calls, capped by chain_calls
    const unsigned dropped = m.a.spec_n > 0 && m.a.spec_on_side ? 1u : 0u;  // (the miss waits for the look-ahead it drops)
    memset(&m.n, 0, sizeof(m.n));
    int want = 1, avail = 0;
    bool launched = false;
    for (int k = 0; k < 24; ++k) {
      const unsigned launches = m.n.launches;
      call(m, 0, kShapes[1], streams[si], 0);
      if (avail > 0) avail--;
      launched = m.n.launches > launches;
      CHECK(launched == (avail == 0));
      if (launched) {
        CHECK(m.n.last_n == (want < cc ? want : cc));
        avail = m.n.last_n, want = want * 2 > XL_AHEAD_MAXCALLS ? XL_AHEAD_MAXCALLS : want * 2;
      }
    }
    CHECK(m.n.misses == 1u && m.n.hits == 23u && m.n.done_records == m.n.launches);
    CHECK(m.n.chain_waits == dropped + m.n.launches - (launched ? 1u : 0u));
    // (e) fused calls behind them record ev_done every time ...
    memset(&m.n, 0, sizeof(m.n));
    for (int k = 0; k < 12; ++k) call(m, 1, kShapes[0], streams[si], 0);
    CHECK(m.n.done_records == 12u && m.n.launches == 0u);
    // ... and an engine that never used a side stream records none, and waits for nothing
    model_init(m, cc, masked, false);
    for (int k = 0; k < 12; ++k) call(m, 1, kShapes[k / 5 % 2], streams[si], 0);
    CHECK(m.n.done_records == 0u && m.n.chain_waits == 0u && m.n.misses == 3u);
  }
}

int main(int argc, char **argv) {
  g_depth_max = argc > 1 ? atoi(argv[1]) : 5;
  for (int cc = 1; cc <= XL_AHEAD_MAXCALLS; ++cc)
    for (int masked = 0; masked < 2; ++masked) steady(cc, masked != 0);
  // every sequence of g_depth_max symbols, for each chain_calls (with the masked pair; chain_calls = 4 also without)
  for (int cc = 1; cc <= XL_AHEAD_MAXCALLS + 1; ++cc) {
    Model m;
    const Pending pd = {0};
    model_init(m, cc > XL_AHEAD_MAXCALLS ? XL_AHEAD_MAXCALLS : cc, cc <= XL_AHEAD_MAXCALLS, false);
    const int len = snprintf(g_ctx, sizeof(g_ctx), "exhaustive cc=%d masked=%d:", m.a.chain_calls, (int)m.masked);
    dfs(m, pd, 0, (size_t)len);
  }
  // random sequences of 64 symbols: the ring of 8 wraps several times between the interruptions (one symbol in nine)
  for (int run = 0; run < 6000; ++run) {
    Model m;
    Pending pd = {0};
    const int cc = 1 + run % XL_AHEAD_MAXCALLS;
    model_init(m, cc, (run / 4) % 2 == 0, (run / 8) % 4 == 3);
    const int sticky = (int)rnd(4);  // how strongly the sequence repeats its previous call: 0 not at all
    int prev = (int)rnd(12);
    for (int k = 0; k < 64; ++k) {
      int sym = rnd(9) == 0 ? 12 + (int)rnd(6) : (int)rnd(12);
      if (sym < 12 && sticky && rnd(4) < (uint32_t)sticky) sym = prev;
      if (sym < 12) prev = sym;
      snprintf(g_ctx, sizeof(g_ctx), "random run=%d cc=%d masked=%d nofuse=%d step=%d %s", run, cc, (int)m.masked, (int)m.nofuse, k, kSymNames[sym]);
      apply(m, pd, sym);
    }
  }
  printf("ok %lu\n", g_checks);
  return 0;
}
