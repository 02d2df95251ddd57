// tests/c/plan_sweep.cpp -- stand-alone host program (its own main; tests/test_plan_cpu.py builds it with ASan + UBSan, links
// csrc/xl_plan.cpp and runs it): the host logic of the batch engine's plan (csrc/xl_plan.h) without a device.  A fixed-seed churn over
// plans -- joins, leaves, recycled client ids, calls that advance the stream by multiples and non-multiples of D, clients maturing
// between plans -- with every invariant of the plan asserted after every plan, then the size rules at their edges, the row
// allocator, the tile height and the CU reservation.  Prints "ok <plans> <checks>".
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <map>
#include <set>
#include <vector>

#include "xl_plan.h"
#include "xl_common.h"
#include "xl_mixf_layout.h"
#include "xl_wide.h"

// (Defined beside the kernels in the library, xl_kernels.hip; this program links xl_plan.cpp alone, so this is a second copy of the
// window image's size: tests/test_plan_cpu.py holds it against the library's own function.)
size_t xl_fir_lds_bytes_ota(uint32_t D, uint32_t Tpad, uint32_t ota) { return ((size_t)(ota - 1u) * D + Tpad) * 8u; }

static const int CHURN_STEPS = 400;  // per setting; about half of the steps plan
static unsigned long g_checks = 0, g_plans = 0;
#define CHECK(cond)                                                  \
  do {                                                               \
    ++g_checks;                                                      \
    if (!(cond)) {                                                   \
      fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      exit(1);                                                       \
    }                                                                \
  } while (0)

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;  // fixed seed (xorshift64*)
static uint32_t rnd(uint32_t n) {
  g_rng ^= g_rng >> 12, g_rng ^= g_rng << 25, g_rng ^= g_rng >> 27;
  return (uint32_t)((g_rng * 0x2545F4914F6CDD1Dull) >> 33) % n;
}

static XlPlanOpts default_opts(uint32_t max_samples, uint32_t gcap) {  // xlating_batch_t's defaults
  XlPlanOpts o;
  o.fmt = XLF_CU8, o.max_samples = max_samples, o.gcap = gcap;
  o.poly_mode = -1, o.poly_min_set = false, o.poly_min_clients = 32, o.poly_m = 0, o.mix_kernel = 1, o.mix_img = -1;
  o.riders = true, o.riders_min_wgs = 512, o.exp_h = 0, o.nco_side = -1, o.expected_clients = 0;
  return o;
}

// The engine's host state and the host part of its plan sequence (xl_batch.cpp: add_client, remove_client, xl_batch_plan, the commit).
struct Eng {
  XlPlanOpts o;
  std::vector<Client> clients;
  std::vector<PolyClass> poly;
  std::vector<XlPolyPending> pending;
  std::vector<DirectClass> classes, classes_rest;
  std::vector<bool> rest_use;
  std::map<uint32_t, uint32_t> free_rows;
  uint32_t rows_end = 0;
  uint64_t next_uid = 1;
  uint32_t trel = 0;
  int big_h = 8;
  bool with_taps = true;

  int add(uint32_t D, uint32_t T) {
    int id = -1;
    for (size_t i = 0; i < clients.size(); ++i)
      if (!clients[i].alive) {
        id = (int)i;
        break;
      }
    if (id < 0) {
      clients.emplace_back();
      id = (int)clients.size() - 1;
    }
    Client &c = clients[id];
    c = Client();
    c.alive = true;
    c.uid = next_uid++;
    c.D = D, c.T = T, c.Tpad = xl_roundup(T, XL_TAP_UNROLL);
    c.wide = xl_fir_needs_wide(D, T, 12u) != 0;
    if (with_taps) {
      c.rt.assign(2 * (size_t)c.Tpad, 0.0f);
      c.rtq.assign(2 * (size_t)T, 0);
      for (uint32_t i = 0; i < 2 * T; ++i) c.rt[i] = (float)((int)rnd(2001) - 1000) / 1024.0f, c.rtq[i] = (int16_t)((int)rnd(2001) - 1000);
    }
    c.incr[0] = (float)c.uid, c.incr[1] = -(float)c.uid;
    c.qincr[0] = (int16_t)(c.uid & 0x7FFF), c.qincr[1] = (int16_t)-(int)(c.uid & 0xFFF);
    c.out_cap = o.gcap * (o.max_samples / D + 1);
    c.row_len = xl_roundup(c.out_cap, 2 * XL_PH_STRIDE);
    c.out_off = xl_row_alloc(free_rows, rows_end, c.row_len);
    return id;
  }
  void remove(int id) {
    clients[id].alive = false;
    clients[id].rt.clear();
    xl_row_free(free_rows, rows_end, clients[id].out_off, clients[id].row_len);
    clients[id].row_len = 0;
  }
  bool wants_plan() const {  // a client that was inside its zero history when the plan was built has matured
    for (const Client &c : clients)
      if (c.alive && !c.planned_mature && xl_mature(c)) return true;
    return false;
  }
  // returns `advanced`; kept[i]: the previous plan's class i was taken over
  uint32_t plan(std::vector<bool> *kept) {
    const uint32_t advanced = trel;
    trel = 0;
    for (Client &c : clients)
      if (c.alive) c.planned_mature = xl_mature(c);
    std::vector<bool> all_use(clients.size(), true);
    for (size_t i = 0; i < clients.size(); ++i)
      if (clients[i].wide) all_use[i] = false;
    rest_use = all_use;
    std::vector<PolyClass> next;
    pending.clear();
    xl_poly_form_classes(o, clients, poly, advanced, &next, &pending, &rest_use);
    kept->clear();
    for (const PolyClass &pc : poly) {
      kept->push_back(pc.keep);
      if (pc.keep) CHECK(pc.d_Rh == nullptr && pc.d_X == nullptr && pc.d_Y == nullptr && pc.d_cols == nullptr && pc.d_cscale == nullptr && pc.d_segmax == nullptr);
    }
    poly = std::move(next);
    for (size_t k = 0; k < poly.size(); ++k)  // (a stand-in for the class's device images: they travel with the class)
      if (pending[k].fresh) poly[k].d_Rh = reinterpret_cast<void *>((uintptr_t)next_uid++ << 4);
    xl_direct_classes(clients, all_use, &classes);
    classes_rest.clear();
    if (!poly.empty()) xl_direct_classes(clients, rest_use, &classes_rest);
    big_h = xl_pick_tile_height(o, classes);
    ++g_plans;
    return advanced;
  }
  void call(uint32_t S, uint32_t G) {
    std::vector<uint64_t> before;
    for (const Client &c : clients) before.push_back(c.consumed);
    xl_clients_commit(clients, S, G);
    trel += S * G;
    for (size_t i = 0; i < clients.size(); ++i) {  // ---- end-of-call commit
      const Client &c = clients[i];
      if (!c.alive) continue;
      CHECK(c.consumed == before[i] + (uint64_t)S * G);
      CHECK(c.last_Kg.size() == G);
      uint32_t sum = 0;
      for (uint32_t k : c.last_Kg) sum += k;
      CHECK(sum == c.last_K);
      const uint32_t j0 = (uint32_t)((c.D - before[i] % c.D) % c.D);
      CHECK(c.last_K == xl_grid_mstart(j0, c.D, S, G));
      uint64_t want = 0;  // outputs on the client's grid n = k D inside the call's samples [before, before + S G)
      for (uint64_t n = (before[i] + c.D - 1) / c.D * c.D; n < before[i] + (uint64_t)S * G; n += c.D) ++want;
      CHECK(c.last_K == want);
    }
  }
};

static uint32_t ceil_div(uint32_t a, uint32_t b) { return (a + b - 1u) / b; }

// ---- membership and the classes' numbers
static void check_classes(const Eng &e) {
  std::vector<int> in_poly(e.clients.size(), 0), in_rest(e.clients.size(), 0), in_all(e.clients.size(), 0);
  std::set<std::tuple<uint32_t, uint32_t, uint32_t>> pkeys;
  for (const PolyClass &pc : e.poly) {
    CHECK(pkeys.insert(std::make_tuple(pc.D, pc.T, pc.hv0)).second);
    for (int id : pc.members) in_poly[id]++;
    const uint32_t D = pc.D;
    // col_of and col_client are inverse maps over the members
    CHECK(pc.col_of.size() == pc.members.size());
    CHECK(pc.col_client.size() == pc.ncols && pc.col_delta.size() == pc.ncols && pc.col_uid.size() == pc.ncols);
    size_t used = 0;
    for (size_t j = 0; j < pc.col_client.size(); ++j) {
      if (pc.col_client[j] < 0) continue;
      ++used;
      auto it = pc.col_of.find(pc.col_client[j]);
      CHECK(it != pc.col_of.end() && it->second == j);
    }
    CHECK(used == pc.members.size());
    CHECK(pc.col_client.empty() || pc.col_client.back() >= 0);  // trailing free columns are dropped
    uint32_t dmax = 0;
    for (int id : pc.members) {
      const Client &c = e.clients[id];
      CHECK(c.alive && !c.wide && c.D == D && c.T == pc.T);
      CHECK((c.planned_mature ? XL_HCAP : (uint32_t)c.consumed) == pc.hv0);
      auto it = pc.col_of.find(id);
      CHECK(it != pc.col_of.end() && pc.col_client[it->second] == id);
      const uint32_t delta = (pc.rem_ref0 + D - (uint32_t)(c.consumed % D)) % D;
      CHECK(pc.col_delta[it->second] == delta);
      CHECK(pc.col_uid[it->second] == c.uid);
      dmax = std::max(dmax, delta);
    }
    CHECK(pc.dmax == dmax);
    CHECK(pc.A == ceil_div(pc.T + pc.dmax, D));
    CHECK(pc.A >= 2u && pc.A <= pc.M / 2u);
    CHECK(D <= 504u);
    CHECK(pc.V == pc.M - pc.A + 1u);
    CHECK(pc.M == 64u || pc.M == 128u || pc.M == 256u);
    CHECK(pc.Dpad >= D && pc.Dpad % XLP_BSTEP == 0u && pc.Dpad < D + XLP_BSTEP && pc.nkb == ceil_div(D, 8u));
    CHECK(pc.mix_kind == ((e.o.mix_kernel == 3u || D > 112u) ? 3u : 1u));
  }
  std::set<std::tuple<uint32_t, uint32_t, uint32_t, uint32_t>> dkeys, rkeys;
  for (const DirectClass &cs : e.classes) {
    CHECK(dkeys.insert(std::make_tuple(cs.D, cs.T, cs.rem0, cs.hv0)).second);
    for (int id : cs.members) {
      in_all[id]++;
      const Client &c = e.clients[id];
      CHECK(c.D == cs.D && c.T == cs.T && c.consumed % c.D == cs.rem0 && (xl_mature(c) ? XL_HCAP : (uint32_t)c.consumed) == cs.hv0);
    }
  }
  for (const DirectClass &cs : e.classes_rest) {
    CHECK(rkeys.insert(std::make_tuple(cs.D, cs.T, cs.rem0, cs.hv0)).second);
    for (int id : cs.members) in_rest[id]++;
  }
  for (size_t i = 0; i < e.clients.size(); ++i) {
    const Client &c = e.clients[i];
    if (!c.alive || c.wide) {
      CHECK(in_poly[i] == 0 && in_rest[i] == 0 && in_all[i] == 0);
      continue;
    }
    CHECK(in_all[i] == 1);
    if (e.poly.empty()) {  // (no polyphase class: the all-clients set serves optimized calls too, no rest set is built)
      CHECK(in_poly[i] == 0 && in_rest[i] == 0);
    } else {
      CHECK(in_poly[i] + in_rest[i] == 1);
    }
    CHECK(e.rest_use[i] == (in_poly[i] == 0));
  }
}

// ---- incremental planning: `prev` = the classes before the plan (a copy), `kept` = their keep flags after it
static void check_incremental(const Eng &e, const std::vector<PolyClass> &prev, const std::vector<bool> &kept, uint32_t advanced) {
  CHECK(e.pending.size() == e.poly.size());
  std::vector<bool> taken(prev.size(), false);
  size_t nreused = 0;
  for (size_t k = 0; k < e.poly.size(); ++k) {
    const PolyClass &pc = e.poly[k];
    const XlPolyPending &pd = e.pending[k];
    CHECK(pd.idx == k);
    std::map<uint32_t, int> times;
    for (uint32_t col : pd.new_cols) {
      CHECK(col < pc.ncols && pc.col_client[col] >= 0);
      times[col]++;
    }
    for (auto &kv : times) CHECK(kv.second == 1);
    if (pd.fresh) {
      // every member is new, columns 0 .. n-1 in member order; no other member offset as the reference gives a smaller dmax
      CHECK(pd.new_cols.size() == pc.members.size() && pc.ncols == pc.members.size());
      for (int cand : pc.members) {
        uint32_t dm = 0;
        for (int id : pc.members)
          dm = std::max(dm, (uint32_t)((e.clients[cand].consumed % pc.D + pc.D - e.clients[id].consumed % pc.D) % pc.D));
        CHECK(dm >= pc.dmax);
      }
      continue;
    }
    // the class this one continues: the first one not yet taken over of its (D, T) and kind -- the planner's choice
    ++nreused;
    size_t si = prev.size();
    for (size_t i = 0; i < prev.size() && si == prev.size(); ++i) {
      const PolyClass &oc = prev[i];
      if (taken[i] || oc.D != pc.D || oc.T != pc.T) continue;
      if (oc.hv0 == pc.hv0 || (pc.hv0 == XL_HCAP && oc.hv0 != XL_HCAP && oc.col_of.count(pc.members[0]))) si = i;
    }
    CHECK(si < prev.size() && kept[si]);
    taken[si] = true;
    const PolyClass &S = prev[si];
    CHECK(pc.rem_ref0 == (S.rem_ref0 + advanced % pc.D) % pc.D);
    CHECK(pc.A == S.A && pc.M == S.M && pc.V == S.V && pc.mix_kind == S.mix_kind && pc.ximg == S.ximg && pc.d_Rh == S.d_Rh);
    // the old columns without the leavers, trailing free ones dropped
    std::vector<int> base(S.col_client);
    std::set<int> here(pc.members.begin(), pc.members.end());
    for (int &id : base)
      if (id >= 0 && !here.count(id)) id = -1;
    while (!base.empty() && base.back() < 0) base.pop_back();
    CHECK(pc.col_scale.size() == base.size());  // (the kept columns' scales: xl_poly_sync_device adds the new columns' behind them)
    std::vector<uint32_t> free_cols;
    for (size_t j = 0; j < base.size(); ++j)
      if (base[j] < 0) free_cols.push_back((uint32_t)j);
    std::vector<uint32_t> joiner_cols;
    size_t nnew = 0;
    for (int id : pc.members) {
      const Client &c = e.clients[id];
      const uint32_t col = pc.col_of.at(id);
      const uint32_t delta = (pc.rem_ref0 + pc.D - (uint32_t)(c.consumed % pc.D)) % pc.D;
      auto it = S.col_of.find(id);
      if (it != S.col_of.end()) {
        CHECK(col == it->second);  // a member (or a recycled id) keeps the column
        const bool same = S.col_uid[col] == c.uid && S.col_delta[col] == delta;
        CHECK(times.count(col) == (same ? 0u : 1u));
        nnew += same ? 0 : 1;
      } else {
        CHECK(times.count(col) == 1u);
        joiner_cols.push_back(col);
        ++nnew;
      }
    }
    CHECK(pd.new_cols.size() == nnew);
    // freed columns are handed out before new ones, lowest first
    std::sort(joiner_cols.begin(), joiner_cols.end());
    const size_t from_free = std::min(joiner_cols.size(), free_cols.size());
    for (size_t j = 0; j < joiner_cols.size(); ++j)
      CHECK(joiner_cols[j] == (j < from_free ? free_cols[j] : (uint32_t)(base.size() + (j - from_free))));
    CHECK(pc.ncols == base.size() + (joiner_cols.size() - from_free));
  }
  size_t nkept = 0;
  for (bool k : kept) nkept += k ? 1 : 0;
  CHECK(nkept == nreused);
}

// ---- one set of direct launches over `classes`
static void check_launches(const Eng &e, const std::vector<DirectClass> &classes, bool q15) {
  Launch Ls[XL_NLAUNCH];
  std::vector<float> image;
  std::vector<double> imageq;
  CHECK(xl_build_launches(e.o, e.clients, Ls, classes, e.big_h, &image, q15 ? &imageq : nullptr) == 0);
  if (q15) CHECK(imageq.size() == image.size());
  std::map<uint32_t, int> by_row;
  size_t members = 0;
  for (const DirectClass &cs : classes)
    for (int id : cs.members) by_row[e.clients[id].out_off] = id, ++members;
  CHECK(by_row.size() == members);
  std::vector<int> slots(e.clients.size(), 0);
  std::vector<std::pair<uint32_t, uint32_t>> ranges;
  for (int li = 0; li < XL_NLAUNCH; ++li) {
    const Launch &L = Ls[li];
    CHECK(L.ct == kHeights[li]);
    uint32_t idle = 0;
    for (const XlGroup &g : L.groups) {
      CHECK(g.ntiles >= 1u && g.ntiles <= (uint32_t)L.nw && L.nw <= XL_NW_MAX);
      CHECK(g.idle_before == idle);
      idle += (uint32_t)L.nw - g.ntiles;
      CHECK(g.Tpad == xl_roundup(g.T, xl_tap_step(L.ct)) && g.D >= L.minD && g.D <= L.maxD);
      for (uint32_t t = 0; t < g.ntiles; ++t) {
        const XlTile &tl = g.tiles[t];
        CHECK(tl.nclients >= 1u && tl.nclients <= (uint32_t)L.ct);
        ranges.push_back(std::make_pair(tl.tap_off, g.Tpad * (uint32_t)L.ct));
        CHECK((size_t)tl.tap_off + (size_t)g.Tpad * L.ct <= image.size() / 2);
        for (uint32_t j = 0; j < tl.nclients; ++j) {
          auto it = by_row.find(tl.out_off[j]);
          CHECK(it != by_row.end());
          const Client &c = e.clients[it->second];
          slots[it->second]++;
          CHECK(c.D == g.D && c.T == g.T && c.consumed % c.D == g.rem0);
          CHECK(tl.incr[j].x == c.incr[0] && tl.incr[j].y == c.incr[1]);
          CHECK(tl.qincr[j] == ((uint32_t)(uint16_t)c.qincr[0] | ((uint32_t)(uint16_t)c.qincr[1] << 16)));
          bool taps_ok = true;  // the image holds the client's taps at [(i ct + j)], zeros in the padding
          for (uint32_t i = 0; i < g.Tpad; ++i) {
            const size_t at = 2 * ((size_t)tl.tap_off + (size_t)i * L.ct + j);
            taps_ok = taps_ok && image[at] == (i < c.T ? c.rt[2 * i] : 0.0f) && image[at + 1] == (i < c.T ? c.rt[2 * i + 1] : 0.0f);
            if (q15) taps_ok = taps_ok && imageq[at] == (i < c.T ? (double)c.rtq[2 * i] : 0.0) && imageq[at + 1] == (i < c.T ? (double)c.rtq[2 * i + 1] : 0.0);
          }
          CHECK(taps_ok);
        }
      }
    }
    CHECK(L.idle_waves == idle);
    if (!L.groups.empty()) {
      CHECK(L.lds <= 160u * 1024u && (L.ota == 64u || L.ota == 32u || L.ota == 16u || L.ota == 8u));
      size_t need = 0;
      for (const XlGroup &g : L.groups) need = std::max(need, xl_fir_lds_bytes_ota(g.D, g.Tpad, L.ota));
      CHECK(L.lds == need);
    }
  }
  for (const DirectClass &cs : classes)
    for (int id : cs.members) CHECK(slots[id] == 1);
  std::sort(ranges.begin(), ranges.end());
  for (size_t i = 1; i < ranges.size(); ++i) CHECK(ranges[i - 1].first + ranges[i - 1].second <= ranges[i].first);
}

// ---- the churn
static void churn(XlPlanOpts o, int steps) {
  static const uint32_t shapes[][2] = {{42, 505}, {42, 505}, {42, 505}, {5, 57}, {100, 257}, {21, 253}, {400, 101}, {128, 300}, {2926, 101}};
  Eng e;
  e.o = o;
  for (int i = 0; i < 40; ++i) e.add(42, 505);
  bool dirty = true;
  for (int step = 0; step < steps; ++step) {
    const uint32_t what = rnd(10);
    std::vector<int> live;
    for (size_t i = 0; i < e.clients.size(); ++i)
      if (e.clients[i].alive) live.push_back((int)i);
    if (what < 3 && live.size() < 90) {  // joins: one, or a few at once (an immature class of their own)
      const uint32_t *s = shapes[rnd(sizeof(shapes) / sizeof(shapes[0]))];
      for (uint32_t n = rnd(4) ? 1u : 2u + rnd(40); n > 0; --n) e.add(s[0], s[1]);
      dirty = true;
    } else if (what < 5 && live.size() > 20) {  // leaves (their ids are recycled by the next joins)
      for (uint32_t n = 1u + (rnd(4) ? 0u : rnd(12)); n > 0 && !live.empty(); --n) {
        const size_t at = rnd((uint32_t)live.size());
        e.remove(live[at]);
        live.erase(live.begin() + at);
      }
      dirty = true;
    } else if (what == 5) {
      dirty = true;  // (an option was set: plan again with nothing changed)
    }
    if (dirty || e.wants_plan()) {
      const std::vector<PolyClass> prev(e.poly);
      std::vector<bool> kept;
      const uint32_t advanced = e.plan(&kept);
      dirty = false;
      check_classes(e);
      check_incremental(e, prev, kept, advanced);
      check_launches(e, e.classes, true);
      if (!e.poly.empty()) check_launches(e, e.classes_rest, false);
    }
    // a call: blocks of a multiple of 42 samples or of any length, short ones too (clients stay immature over several plans) -- or none
    // (two plans at one stream position: a client that leaves and one that takes its id over at once have the same delay)
    if (rnd(4) == 0) continue;
    const uint32_t G = 1u << rnd(3);
    uint32_t S = rnd(3) == 0 ? 42u * (1u + rnd(40)) : 1u + rnd(rnd(2) ? 3000u : 300u);
    if (G > 1u) S = std::max(S, 2926u);
    e.call(std::min(S, o.max_samples), std::min(G, o.gcap));
  }
}

// ---- a client leaves and another one takes over its id at the same stream position, between two plans: same class, same column, same
// delay -- only the uid tells that the column's spectra are another client's
static void recycled_id(void) {
  Eng e;
  e.o = default_opts(16384, 4);
  e.o.poly_mode = 1;
  std::vector<int> ids;
  for (int i = 0; i < 5; ++i) ids.push_back(e.add(42, 505));
  std::vector<bool> kept;
  e.plan(&kept);
  check_classes(e);
  CHECK(e.poly.size() == 1 && e.pending[0].fresh && e.pending[0].new_cols.size() == 5);
  for (int round = 0; round < 2; ++round) {  // inside the zero history, then mature
    e.remove(ids[2]);
    const int id = e.add(42, 505);
    CHECK(id == ids[2]);
    e.clients[id].consumed = e.clients[ids[0]].consumed;
    const std::vector<PolyClass> prev(e.poly);
    const uint32_t advanced = e.plan(&kept);
    check_classes(e);
    check_incremental(e, prev, kept, advanced);
    CHECK(e.poly.size() == 1 && !e.pending[0].fresh && e.pending[0].new_cols == std::vector<uint32_t>(1, prev[0].col_of.at(id)));
    e.call(4200, 1);
    e.plan(&kept);
    CHECK(e.poly.size() == 1 && e.poly[0].hv0 == XL_HCAP && e.pending[0].new_cols.empty());  // (the immature class, taken over as it matures)
  }
}

// ---- the rider split: a first launch whose groups are all full gives its last group's fourth tile a group of its own (3 + 1 tiles),
// so that the NCO riders find a spare wave -- when riders are on and the launch is inside their window (here: riders_min_wgs = 1)
static void rider_split(void) {
  for (int riders = 0; riders < 2; ++riders) {
    Eng e;
    e.o = default_opts(16384, 4);
    e.o.poly_mode = 0, e.o.riders = riders != 0, e.o.riders_min_wgs = 1;
    for (int i = 0; i < 64; ++i) e.clients[e.add(42, 505)].consumed = 100000u;  // 8 tiles of 8: two full groups
    std::vector<bool> kept;
    e.plan(&kept);
    CHECK(e.poly.empty() && e.classes.size() == 1 && e.big_h == 8);
    check_launches(e, e.classes, true);
    Launch Ls[XL_NLAUNCH];
    std::vector<float> image;
    CHECK(xl_build_launches(e.o, e.clients, Ls, e.classes, e.big_h, &image, nullptr) == 0);
    const Launch &L = Ls[3];  // (height 8)
    if (riders) {
      CHECK(L.groups.size() == 3 && L.groups[0].ntiles == 4u && L.groups[1].ntiles == 3u && L.groups[2].ntiles == 1u && L.idle_waves == 4u);
      CHECK(L.groups[2].tiles[0].tap_off == 7u * 508u * 8u && L.groups[2].idle_before == 1u);
    } else {
      CHECK(L.groups.size() == 2 && L.groups[0].ntiles == 4u && L.groups[1].ntiles == 4u && L.idle_waves == 0u);
    }
    e.o.riders_min_wgs = 512;  // (the default: two workgroup rows are no launch for riders)
    Launch Ld[XL_NLAUNCH];
    image.clear();
    CHECK(xl_build_launches(e.o, e.clients, Ld, e.classes, e.big_h, &image, nullptr) == 0 && Ld[3].groups.size() == 2);
  }
}

// ---- the size rules at their edges: one engine of `n` mature clients of one shape on one grid (+ `spread`: offsets 0 .. spread)
static std::vector<PolyClass> classes_of(const XlPlanOpts &o, uint32_t n, uint32_t D, uint32_t T, uint32_t spread = 0) {
  Eng e;
  e.o = o;
  e.with_taps = false;
  for (uint32_t i = 0; i < n; ++i) e.clients[e.add(D, T)].consumed = 100000u + (spread ? i % (spread + 1u) : 0u);
  std::vector<bool> kept;
  e.plan(&kept);
  check_classes(e);
  return e.poly;
}

static void size_rule_edges(void) {
  const XlPlanOpts def = default_opts(131072, 8);
  XlPlanOpts o = def;
  // option "polyphase": 0 never, 1 whenever the shape fits (A >= 2, A <= M / 2, D <= 504), -1 by the size rule
  o.poly_mode = 0;
  CHECK(classes_of(o, 200, 42, 505).empty());
  o.poly_mode = 1;
  CHECK(classes_of(o, 3, 5, 57).size() == 1 && classes_of(o, 1, 42, 505).size() == 1);
  CHECK(classes_of(o, 3, 42, 50).size() == 1);   // T < 2 D, A = 2
  CHECK(classes_of(o, 3, 42, 42).empty());       // A = 1
  CHECK(classes_of(o, 42, 42, 1, 41).empty() && classes_of(o, 42, 42, 2, 41).size() == 1);  // (every offset taken: dmax = 41, A = 1 / 2)
  CHECK(classes_of(o, 3, 504, 1008).size() == 1 && classes_of(o, 3, 505, 1010).empty());
  CHECK(classes_of(o, 3, 2, 256).size() == 1 && classes_of(o, 3, 2, 257).empty());  // A = 128 / 129 > M / 2
  // the size rule: T >= 2 D and 32 members, 128 for streamed classes (D > 112)
  CHECK(classes_of(def, 31, 42, 505).empty() && classes_of(def, 32, 42, 505).size() == 1);
  CHECK(classes_of(def, 127, 128, 300).empty() && classes_of(def, 128, 128, 300).size() == 1);
  CHECK(classes_of(def, 32, 42, 83).empty() && classes_of(def, 32, 42, 84).size() == 1);      // T = 2 D - 1 / 2 D
  CHECK(classes_of(def, 128, 128, 255).empty() && classes_of(def, 128, 128, 256).size() == 1);
  // D 64 / 65: up to 8 k-blocks the four-wave two-half mix and 128 / 256 points; above, 64 points for short branch filters
  {
    const std::vector<PolyClass> a = classes_of(def, 32, 64, 192), b = classes_of(def, 32, 65, 195);
    CHECK(a.size() == 1 && a[0].nkb == 8u && a[0].M == 256u && a[0].mix_kind == 1u && a[0].A == 3u && a[0].V == 254u);
    CHECK(b.size() == 1 && b[0].nkb == 9u && b[0].M == 64u && b[0].mix_kind == 1u && b[0].A == 3u && b[0].V == 62u);
    CHECK(classes_of(def, 32, 65, 65 * 9).at(0).M == 256u);  // (9 taps per branch: no 64-point class)
  }
  // D 112 / 113: the two-half mix's last branch count; beyond it float32 operands, streamed, from 128 members on
  {
    const std::vector<PolyClass> a = classes_of(def, 32, 112, 336), b = classes_of(def, 128, 113, 339);
    CHECK(a.size() == 1 && a[0].nkb == 14u && a[0].mix_kind == 1u && a[0].M == 64u);
    CHECK(b.size() == 1 && b[0].nkb == 15u && b[0].mix_kind == 3u && b[0].M == 64u);
    CHECK(classes_of(def, 127, 113, 339).empty() && classes_of(def, 127, 112, 336).size() == 1);
    o = def, o.mix_kernel = 3;
    CHECK(classes_of(o, 32, 42, 505).at(0).mix_kind == 3u);
  }
  // D 504 / 505
  CHECK(classes_of(def, 128, 504, 1008).size() == 1 && classes_of(def, 128, 505, 1010).empty());
  // transform length (767 / 768 members) and operand image (768 .. 1088 members, 4 blocks per call or more)
  for (uint32_t gcap = 3; gcap <= 4; ++gcap) {
    const XlPlanOpts og = default_opts(131072, gcap);
    const struct {
      uint32_t n, M;
      bool ximg;
    } want[] = {{767, 256, false}, {768, 128, gcap >= 4}, {1088, 128, gcap >= 4}, {1089, 128, false}};
    for (const auto &w : want) {
      const std::vector<PolyClass> c = classes_of(og, w.n, 42, 505);
      CHECK(c.size() == 1 && c[0].members.size() == w.n && c[0].M == w.M && c[0].ximg == w.ximg && c[0].A == 13u && c[0].V == w.M - 12u);
    }
  }
  o = def, o.fmt = XLF_CF32;
  CHECK(!classes_of(o, 1024, 42, 505).at(0).ximg);  // (no constant scale on a cf32 stream: no operand image)
  o = def, o.mix_img = 0;
  CHECK(!classes_of(o, 1024, 42, 505).at(0).ximg);
  o = def, o.mix_img = 1;
  CHECK(classes_of(o, 40, 42, 505).at(0).ximg);
  o = def, o.poly_m = 128;
  CHECK(classes_of(o, 40, 42, 505).at(0).M == 128u);
  o = def, o.poly_min_set = true, o.poly_min_clients = 5;
  CHECK(classes_of(o, 4, 42, 505).empty() && classes_of(o, 5, 42, 505).size() == 1);
}

// ---- output rows: extents never overlap, freeing coalesces, the last extent lowers rows_end
static void rows(void) {
  std::map<uint32_t, uint32_t> free_rows, live;
  uint32_t rows_end = 0;
  for (int step = 0; step < 4000; ++step) {
    if (live.size() < 48 && (live.empty() || rnd(5) < 3)) {  // (a few dozen rows: every state of a short free list comes up)
      const uint32_t len = 32u * (1u + rnd(12));
      const uint32_t off = xl_row_alloc(free_rows, rows_end, len);
      CHECK(off + len <= rows_end);
      CHECK(live.emplace(off, len).second);
    } else {
      auto it = live.begin();
      std::advance(it, rnd((uint32_t)live.size()));
      const bool last = it->first + it->second == rows_end;
      const uint32_t end_before = rows_end;
      xl_row_free(free_rows, rows_end, it->first, it->second);
      CHECK(last ? rows_end <= it->first : rows_end == end_before);
      live.erase(it);
    }
    // live and free extents tile [0, rows_end) exactly; no two free extents touch, none touches the end
    std::map<uint32_t, std::pair<uint32_t, bool>> all;
    for (auto &kv : live) CHECK(all.emplace(kv.first, std::make_pair(kv.second, false)).second);
    for (auto &kv : free_rows) CHECK(kv.second > 0u && all.emplace(kv.first, std::make_pair(kv.second, true)).second);
    uint32_t at = 0;
    bool prev_free = false;
    for (auto &kv : all) {
      CHECK(kv.first == at);
      CHECK(!(prev_free && kv.second.second));
      at += kv.second.first, prev_free = kv.second.second;
    }
    CHECK(at == rows_end && !prev_free);
  }
  xl_row_free(free_rows, rows_end, 0, 0);  // (a client without a row)
  while (!live.empty()) {
    xl_row_free(free_rows, rows_end, live.begin()->first, live.begin()->second);
    live.erase(live.begin());
  }
  CHECK(rows_end == 0u && free_rows.empty());
}

// ---- tile height and CU reservation
static XlReserve reserve_of(const Eng &e, int last_band, bool nomask, bool rounds1, int cap) {
  size_t n = 0;
  for (const Client &c : e.clients) n += c.alive ? 1 : 0;
  return xl_reserve_want(e.o, n, e.classes_rest, e.poly, xl_direct_macs(e.classes), xl_direct_macs(e.classes_rest), last_band, nomask,
                         rounds1, cap);
}

static void height_and_reservation(void) {
  // The server-default shape (D = 42, 505 taps, blocks of 262144 bytes of cu8) at 8 blocks per call: {clients, tile height, CUs per XCD}.
  // Source: the reservations at 2304 and 4096 clients are pinned in describe() by tests/test_batch_gpu.py ("side kernel:" absent,
  // test_group_2304_clients_sampled_no_cu_reservation; "side kernel: 32 CUs reserved", test_group_4096_clients_sampled).  The other
  // two and the heights are describe() of the engine on an MI355X at the commit before this logic left xl_batch.cpp: "side kernel:
  // 16 / 32 CUs reserved" at 1024 / 2048 clients, and after a native call "direct: h10 x 26 / h9 x 57 / h8 x 72 / h9 x 114 groups".
  static const uint32_t want[][3] = {{1024, 10, 2}, {2048, 9, 4}, {2304, 8, 0}, {4096, 9, 4}};
  for (const auto &w : want) {
    Eng e;
    e.o = default_opts(131072, 8);
    e.with_taps = false;
    for (uint32_t i = 0; i < w[0]; ++i) e.clients[e.add(42, 505)].consumed = 100000u;
    std::vector<bool> kept;
    e.plan(&kept);
    CHECK(e.poly.size() == 1 && e.classes_rest.empty());
    CHECK((uint32_t)e.big_h == w[1]);
    const XlReserve rv = reserve_of(e, -1, false, false, -1);
    CHECK(rv.want == w[2]);
    CHECK(rv.band == (w[0] <= 2048u ? 0 : (w[0] < 3009u ? 1 : 2)));
    // the tuning switches, as values
    CHECK(reserve_of(e, -1, true, false, -1).want == 0u);
    CHECK(reserve_of(e, -1, false, true, -1).want == (rv.want ? std::min(16u, (w[0] / 64u + 7u) / 8u) : 0u));
    CHECK(reserve_of(e, -1, false, false, 1).want == std::min(rv.want, 1u));
    CHECK(reserve_of(e, -1, false, false, 100).want == rv.want);
    for (int h : {8, 9, 10, 12}) {
      e.o.exp_h = h;
      CHECK(xl_pick_tile_height(e.o, e.classes) == h);
    }
    e.o.exp_h = 7;
    CHECK((uint32_t)xl_pick_tile_height(e.o, e.classes) == w[1]);
    e.o.exp_h = 0;
    e.o.nco_side = 0;
    CHECK(reserve_of(e, -1, false, false, -1).want == 0u);
  }
  {  // the bands' hysteresis (xl_plan_rules.h: a plan keeps its band until the load is XL_BAND_HYST = 2 chain workgroups past an edge):
     // 33 and 34 chain workgroups stay in the one-CU-per-workgroup band after a plan in it (5 CUs per XCD), 35 leave it; without
     // history 33 are in the no-reservation band.  One-block engines take the side stream up to XL_SIDE_ONE_BLOCK_MAX clients only.
    const struct {
      uint32_t n, gcap;
      int last_band, band;
      uint32_t want;
    } cases[] = {{2112, 8, 0, 0, 5}, {2112, 8, -1, 1, 0}, {2176, 8, 0, 0, 5}, {2240, 8, 0, 1, 0}, {2048, 1, -1, 0, 4}, {2049, 1, 0, 0, 0}};
    for (const auto &c : cases) {
      Eng e;
      e.o = default_opts(131072, c.gcap);
      e.with_taps = false;
      for (uint32_t i = 0; i < c.n; ++i) e.clients[e.add(42, 505)].consumed = 100000u;
      std::vector<bool> kept;
      e.plan(&kept);
      const XlReserve rv = reserve_of(e, c.last_band, false, false, -1);
      CHECK(rv.band == c.band && rv.want == c.want);
    }
  }
  {  // tile height: a last round of workgroups counts as three rows of 256 at least.  352 default-shape clients: 11 groups x 49 output
     // tiles = 539 workgroups at height 8 (three rows: 24), 490 at height 9 (two rows, counted as three: 27) -- height 8
    Eng e;
    e.o = default_opts(131072, 8);
    e.with_taps = false;
    for (uint32_t i = 0; i < 352; ++i) e.clients[e.add(42, 505)].consumed = 100000u;
    std::vector<bool> kept;
    e.plan(&kept);
    CHECK(e.big_h == 8);
  }
  // option "expected_clients" (tests/test_batch_gpu.py: test_expected_clients_reserves_the_side_kernels_cus_once pins 8 -> 16 CUs
  // for 500 -> 700 clients and 16 from the start for 1024 announced ones, at 2 blocks of 131072 bytes per call)
  for (uint32_t expect : {0u, 1024u}) {
    Eng e;
    e.o = default_opts(65536, 2);
    e.o.expected_clients = expect;
    e.with_taps = false;
    std::vector<bool> kept;
    for (uint32_t i = 0; i < 500; ++i) e.clients[e.add(42, 505)].consumed = 100000u;
    e.plan(&kept);
    const XlReserve r0 = reserve_of(e, -1, false, false, -1);
    for (uint32_t i = 500; i < 700; ++i) e.clients[e.add(42, 505)].consumed = 100000u;
    e.plan(&kept);
    const XlReserve r1 = reserve_of(e, r0.band, false, false, -1);
    CHECK(8u * r0.want == (expect ? 16u : 8u) && 8u * r1.want == 16u);
  }
  {  // no clients, and a direct-only plan: light launches take one CU per chain workgroup, heavy ones none
    Eng e;
    e.o = default_opts(131072, 8);
    e.with_taps = false;
    std::vector<bool> kept;
    e.plan(&kept);
    CHECK(reserve_of(e, -1, false, false, -1).want == 0u && e.big_h == 8);
    for (uint32_t i = 0; i < 20; ++i) e.clients[e.add(42, 505)].consumed = 100000u;
    e.plan(&kept);
    CHECK(e.poly.empty() && reserve_of(e, -1, false, false, -1).want == 1u);
    e.o.poly_mode = 0;
    for (uint32_t i = 20; i < 1024; ++i) e.clients[e.add(42, 505)].consumed = 100000u;
    e.plan(&kept);
    CHECK(e.poly.empty() && reserve_of(e, -1, false, false, -1).want == 0u);
    e.o.nco_side = 1;
    CHECK(reserve_of(e, -1, false, false, -1).want == 2u);
  }
  // the stream pair: grown at once, shrunk only when two CUs per XCD too many are held, dropped at once
  CHECK(xl_reserve_recreate(1, 0) && xl_reserve_recreate(3, 2) && !xl_reserve_recreate(2, 2) && !xl_reserve_recreate(2, 3));
  CHECK(xl_reserve_recreate(2, 4) && xl_reserve_recreate(0, 1) && !xl_reserve_recreate(0, 0));
}

// ---- the per-call side / fused rule (xl_side_call) at its edges
static void side_rule(void) {
  const size_t at = XL_SIDE_ONE_BLOCK_MAX;
  // arguments: q15, nco_side, G, use_poly, nclients, light, masked_pair, engine_stream
  for (int nco_side = -1; nco_side <= 1; ++nco_side)  // Q15 calls: never
    for (unsigned G : {1u, 2u, 8u})
      for (int bits = 0; bits < 16; ++bits)
        CHECK(!xl_side_call(true, nco_side, G, (bits & 1) != 0, (bits & 2) ? at + 1 : 64, (bits & 4) != 0, (bits & 8) != 0, true));
  for (unsigned G : {1u, 2u, 8u})
    for (int bits = 0; bits < 32; ++bits) {
      const bool poly = (bits & 1) != 0, light = (bits & 2) != 0, pair = (bits & 4) != 0, eng = (bits & 8) != 0;
      const size_t n = (bits & 16) ? at + 1 : at;
      CHECK(!xl_side_call(false, 0, G, poly, n, light, pair, eng));  // option 0: never
      CHECK(xl_side_call(false, 1, G, poly, n, light, pair, eng));   // option 1: every float call
    }
  // option -1, polyphase calls: several blocks always, one block up to XL_SIDE_ONE_BLOCK_MAX clients, whatever the stream
  for (int bits = 0; bits < 8; ++bits) {
    const bool light = (bits & 1) != 0, pair = (bits & 2) != 0, eng = (bits & 4) != 0;
    CHECK(xl_side_call(false, -1, 2, true, at + 1, light, pair, eng));
    CHECK(xl_side_call(false, -1, 1, true, at, light, pair, eng));
    CHECK(!xl_side_call(false, -1, 1, true, at + 1, light, pair, eng));
    CHECK(!xl_side_call(false, -1, 1, false, at, light, pair, eng));  // (a one-block direct call: never)
  }
  // option -1, direct-only calls of several blocks: light ones, with the masked pair, on the engine's stream only
  for (int bits = 0; bits < 8; ++bits) {
    const bool light = (bits & 1) != 0, pair = (bits & 2) != 0, eng = (bits & 4) != 0;
    CHECK(xl_side_call(false, -1, 2, false, 64, light, pair, eng) == (light && pair && eng));
  }
  CHECK(xl_direct_is_light(249.9e6) && !xl_direct_is_light(250e6));
}

int main(void) {
  side_rule();
  XlPlanOpts o = default_opts(16384, 4);
  churn(o, CHURN_STEPS);  // the size rule: classes of 32 members and more
  o.poly_mode = 1;
  churn(o, CHURN_STEPS);  // every class that fits: many small classes beside each other
  recycled_id();
  rider_split();
  size_rule_edges();
  rows();
  height_and_reservation();
  printf("ok %lu %lu\n", g_plans, g_checks);
  return 0;
}
