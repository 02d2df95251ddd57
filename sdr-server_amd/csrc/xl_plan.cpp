// xl_plan.cpp -- the host logic of the batch engine's plan (xl_plan.h): no HIP runtime call, no device.
#include "xl_plan.h"

#include <errno.h>
#include <math.h>
#include <string.h>

#include <algorithm>
#include <tuple>

#include "xl_common.h"
#include "xl_mixf_layout.h"

// Output rows.  A client's row (its outputs of a call, and 1/16 of that in the phase tables) is reserved when it joins and
// stays where it is until it leaves: re-plans never move anybody's outputs.  First fit over the free extents, else the end.
uint32_t xl_row_alloc(std::map<uint32_t, uint32_t> &free_rows, uint32_t &rows_end, uint32_t len) {
  for (auto it = free_rows.begin(); it != free_rows.end(); ++it) {
    if (it->second < len) continue;
    const uint32_t off = it->first, rest = it->second - len;
    free_rows.erase(it);
    if (rest) free_rows[off + len] = rest;
    return off;
  }
  const uint32_t off = rows_end;
  rows_end += len;
  return off;
}

void xl_row_free(std::map<uint32_t, uint32_t> &free_rows, uint32_t &rows_end, uint32_t off, uint32_t len) {
  if (len == 0) return;
  auto it = free_rows.emplace(off, len).first;
  auto nx = std::next(it);
  if (nx != free_rows.end() && it->first + it->second == nx->first) {
    it->second += nx->second;
    free_rows.erase(nx);
  }
  if (it != free_rows.begin()) {
    auto pv = std::prev(it);
    if (pv->first + pv->second == it->first) {
      pv->second += it->second;
      free_rows.erase(it);
      it = pv;
    }
  }
  if (it->first + it->second == rows_end) {  // the last extent gives the space back
    rows_end = it->first;
    free_rows.erase(it);
  }
}

// NCO riders (xl_kernels.hip) pay in a window: the launch is one round of workgroups (all resident at once -- in a
// multi-round launch the dispatcher evens things out by itself and riders, which sit in one XCD's share of the work
// list, measured 5-12 % slower), and the FIR work of a SIMD clearly outlasts the chain (~18.5 ns per output; when the
// chain is the critical path -- short filters, few clients -- it is quicker alone in workgroups of its own: no
// staging first, 16 lanes).  Measured at 505 taps, D = 42: 384..1024 clients 3-8 % faster with riders; 101 taps
// 25 % slower.
bool xl_riders_window(size_t wgs, int nw, uint32_t Tpad, int ct, uint32_t K, size_t lds, int min_wgs) {
  const size_t cap = 256 * std::max<size_t>(1, std::min<size_t>((160 * 1024) / std::max<size_t>(lds, 1), 7));
  const double fir_us = (double)wgs * nw / 1024.0 * (double)Tpad * ct * 8.0 / 2000.0;  // 4-cycle packed FMAs at ~2 GHz
  const double chain_us = 0.0185 * (double)K;
  return min_wgs <= 1 || (wgs >= (size_t)min_wgs && wgs <= cap && fir_us >= 1.3 * chain_us);
}

const int kHeights[XL_NLAUNCH] = {12, 10, 9, 8, 4, 2, 1};

// Direct classes over the clients selected by `use`: key (D, T, consumed mod D, valid history).  A mature client's
// windows never reach below its join point, so all mature clients of one grid share a class whatever their age.
void xl_direct_classes(const std::vector<Client> &clients, const std::vector<bool> &use, std::vector<DirectClass> *out) {
  out->clear();
  std::map<std::tuple<uint32_t, uint32_t, uint32_t, uint32_t>, size_t> cls_of;
  for (size_t i = 0; i < clients.size(); ++i) {
    const Client &c = clients[i];
    if (!c.alive || !use[i]) continue;
    const uint32_t rem = (uint32_t)(c.consumed % c.D);
    const uint32_t hv = xl_mature(c) ? XL_HCAP : (uint32_t)c.consumed;
    auto key = std::make_tuple(c.D, c.T, rem, hv);
    auto it = cls_of.find(key);
    if (it == cls_of.end()) {
      it = cls_of.emplace(key, out->size()).first;
      out->push_back(DirectClass{c.D, c.T, rem, hv, {}});
    }
    (*out)[it->second].members.push_back((int)i);
  }
}

// Builds one set of direct-FIR launches over `classes`: tiles, groups, tap image rows (appended to `image`).
int xl_build_launches(const XlPlanOpts &o, const std::vector<Client> &clients, Launch *Ls, const std::vector<DirectClass> &classes,
                      int big_h, std::vector<float> *image, std::vector<double> *imageq) {
  struct TileDesc {
    size_t cls;
    std::vector<int> ids;
  };
  std::vector<TileDesc> tiles_of[XL_NLAUNCH];
  const uint32_t cap_samples = o.max_samples * o.gcap;
  for (int li = 0; li < XL_NLAUNCH; ++li) {
    Ls[li].ct = kHeights[li];
    Ls[li].lds = 0;
    Ls[li].nw = XL_NW_DEFAULT;
    Ls[li].all_wide = true;
    Ls[li].maxD = 1;
    Ls[li].minD = 0xFFFFFFFFu;
  }
  for (size_t k = 0; k < classes.size(); ++k) {
    const std::vector<int> &m = classes[k].members;
    int h = big_h;
    if (m.size() < 8) h = m.size() > 4 ? 8 : (m.size() > 2 ? 4 : (m.size() > 1 ? 2 : 1));
    int li = 0;
    while (kHeights[li] != h) ++li;
    for (size_t next = 0; next < m.size(); next += (size_t)h) {
      const size_t cnt = std::min<size_t>((size_t)h, m.size() - next);
      tiles_of[li].push_back(TileDesc{k, std::vector<int>(m.begin() + next, m.begin() + next + cnt)});
    }
  }

  for (int li = 0; li < XL_NLAUNCH; ++li) {
    Launch &L = Ls[li];
    if (tiles_of[li].empty()) continue;
    const int ct = L.ct;
    int gi = -1;
    size_t gcls = 0;
    for (const TileDesc &td : tiles_of[li]) {
      const DirectClass &cs = classes[td.cls];
      const uint32_t Tpad = xl_roundup(cs.T, xl_tap_step(ct));
      if (gi < 0 || gcls != td.cls || L.groups[gi].ntiles == (uint32_t)L.nw) {
        L.groups.emplace_back();
        gi = (int)L.groups.size() - 1;
        gcls = td.cls;
        XlGroup *g = &L.groups[gi];
        memset(g, 0, sizeof(*g));
        g->D = cs.D;
        g->T = cs.T;
        g->Tpad = Tpad;
        g->rem0 = cs.rem0;
        g->hv0 = cs.hv0;
        g->wide = (cs.D % 2 == 0) ? 1u : 0u;
        if (!g->wide) L.all_wide = false;
        L.lds = std::max(L.lds, xl_fir_lds_bytes_ota(cs.D, Tpad, 64));
        L.maxD = std::max(L.maxD, cs.D);
        L.minD = std::min(L.minD, cs.D);
      }
      XlGroup *g = &L.groups[gi];
      XlTile &t = g->tiles[g->ntiles++];
      const uint32_t real_off = (uint32_t)(image->size() / 2);
      t.tap_off = real_off;
      t.nclients = (uint32_t)td.ids.size();  // a partial last tile keeps zero taps for the missing clients
      image->resize(image->size() + (size_t)2 * Tpad * ct, 0.0f);
      if (imageq) imageq->resize(image->size(), 0.0);
      float *dst = image->data() + (size_t)2 * real_off;
      for (size_t j = 0; j < td.ids.size(); ++j) {
        const Client &c = clients[td.ids[j]];
        t.out_off[j] = c.out_off;
        t.incr[j] = make_float2(c.incr[0], c.incr[1]);
        t.qincr[j] = (uint32_t)(uint16_t)c.qincr[0] | ((uint32_t)(uint16_t)c.qincr[1] << 16);
        for (uint32_t i = 0; i < cs.T; ++i) {
          dst[((size_t)i * ct + j) * 2] = c.rt[2 * i];
          dst[((size_t)i * ct + j) * 2 + 1] = c.rt[2 * i + 1];
          if (imageq) {
            (*imageq)[(size_t)2 * real_off + ((size_t)i * ct + j) * 2] = (double)c.rtq[2 * i];
            (*imageq)[(size_t)2 * real_off + ((size_t)i * ct + j) * 2 + 1] = (double)c.rtq[2 * i + 1];
          }
        }
      }
    }
  }
  // ---- spare waves for the NCO riders (xl_kernels.hip): groups with fewer tiles than the launch has waves.  The
  // launch that carries the role (the first one with groups) gets a spare wave by splitting its last full group
  // into 3 + 1 tiles when it has none and the engine is big enough for the balance to matter.
  {
    bool first = true;
    for (int lq = 0; lq < XL_NLAUNCH; ++lq) {
      Launch &L = Ls[lq];
      if (L.groups.empty()) continue;
      uint32_t idle = 0;
      for (const XlGroup &g : L.groups) idle += (uint32_t)L.nw - g.ntiles;
      const uint32_t kest = cap_samples / L.groups[0].D + 1;
      if (first && idle == 0 && o.riders && L.nw == XL_NW_MAX &&
          xl_riders_window((L.groups.size() + 1) * ((kest + 63) / 64), L.nw, L.groups[0].Tpad, L.ct, kest, L.lds,
                           o.riders_min_wgs)) {
        XlGroup &last = L.groups.back();
        XlGroup extra = last;
        extra.ntiles = 1;
        extra.tiles[0] = last.tiles[XL_NW_MAX - 1];
        last.ntiles = XL_NW_MAX - 1;
        L.groups.push_back(extra);
      }
      // (riders are only used in one-round launches -- xl_riders_window -- where every workgroup is dispatched within
      // ~10 us of the start, so the groups with spare waves can stay where they are: last, which suits the tail)
      idle = 0;
      for (XlGroup &g : L.groups) {
        g.idle_before = idle;
        idle += (uint32_t)L.nw - g.ntiles;
      }
      L.idle_waves = idle;
      first = false;
    }
  }
  for (int lq = 0; lq < XL_NLAUNCH; ++lq) {
    Launch &L = Ls[lq];
    L.ota = 64;
    if (L.lds > 160 * 1024) {  // huge decimation: fewer active lanes per wave so that the window image fits
      for (L.ota = 32; L.ota >= 8; L.ota >>= 1) {
        size_t need = 0;
        for (const XlGroup &g : L.groups) need = std::max(need, xl_fir_lds_bytes_ota(g.D, g.Tpad, L.ota));
        if (need <= 160 * 1024) {
          L.lds = need;
          break;
        }
      }
      if (L.ota < 8) return -EINVAL;  // (add_client already refused such a shape)
    }
  }
  return 0;
}

// The matrix-core Q15 launch: one tile per 32 eligible members of a direct class (one grid: clients of one (D, T) that joined at other
// stream positions are tiles of their own).  Eligibility is proved here, per client, before anything reaches the device.
void xl_build_q15mm(const XlPlanOpts &o, const std::vector<Client> &clients, const std::vector<DirectClass> &classes, XlQmmPlan *plan,
                    std::vector<bool> *rest_use) {
  *plan = XlQmmPlan();
  uint64_t frags = 0;
  std::vector<std::pair<size_t, std::vector<int>>> tiles;  // (class, members)
  for (size_t k = 0; k < classes.size(); ++k) {
    const DirectClass &cs = classes[k];
    const uint32_t ksteps = xl_q15mm_ksteps(cs.T);
    const bool fits = xl_q15mm_pick_nc(cs.D, ksteps) != 0u && xl_q15mm_acc_bounded(ksteps);  // proof (b)
    std::vector<int> ok;
    for (int id : cs.members) {
      if (!fits)
        plan->fb_window++;
      else if (!clients[id].qmm_digits)  // proof (a), taken when the client joined
        plan->fb_digits++;
      else
        ok.push_back(id);
    }
    for (size_t next = 0; next < ok.size(); next += XL_QMM_ROWS) {
      const size_t cnt = std::min<size_t>(XL_QMM_ROWS, ok.size() - next);
      tiles.emplace_back(k, std::vector<int>(ok.begin() + next, ok.begin() + next + cnt));
      frags += xl_q15mm_image_bytes(cs.D, ksteps) / XL_QMM_FRAG;
    }
  }
  plan->image.assign((size_t)frags * XL_QMM_FRAG, 0);
  uint32_t frag_off = 0;
  for (const auto &td : tiles) {
    const DirectClass &cs = classes[td.first];
    XlQmmTile t;
    memset(&t, 0, sizeof(t));
    t.D = cs.D, t.T = cs.T, t.ksteps = xl_q15mm_ksteps(cs.T);
    t.rem0 = cs.rem0, t.hv0 = cs.hv0;
    t.nc = xl_q15mm_pick_nc(cs.D, t.ksteps);
    t.nclients = (uint32_t)td.second.size();
    t.frag_off = frag_off;
    int8_t *img = plan->image.data() + (size_t)frag_off * XL_QMM_FRAG;
    for (size_t j = 0; j < td.second.size(); ++j) {
      const Client &c = clients[td.second[j]];
      t.out_off[j] = c.out_off;
      t.qincr[j] = (uint32_t)(uint16_t)c.qincr[0] | ((uint32_t)(uint16_t)c.qincr[1] << 16);
      t.corr_r[j] = xl_q15mm_correction(c.rtq.data(), cs.T, 0);
      t.corr_i[j] = xl_q15mm_correction(c.rtq.data(), cs.T, 1);
      xl_q15mm_fill_row(img, (uint32_t)j, c.rtq.data(), cs.T, cs.D, t.ksteps);
      (*rest_use)[td.second[j]] = false;
    }
    frag_off += (uint32_t)(xl_q15mm_image_bytes(cs.D, t.ksteps) / XL_QMM_FRAG);
    plan->lds = std::max(plan->lds, xl_q15mm_lds_bytes(t, o.fmt));
    plan->nclients += t.nclients;
    plan->tiles.push_back(t);
  }
}

// complex MACs per sample of a block of the direct launches over `classes`
double xl_direct_macs(const std::vector<DirectClass> &classes) {
  double macs = 0.0;
  for (const DirectClass &cs : classes) macs += (double)cs.members.size() * cs.T / cs.D;
  return macs;
}

// Register-tile height of the large direct classes (chosen over the plan's all-clients classes).  Every wave does the
// same work (64 outputs x H clients x T taps) and a CU holds floor(160 KiB / window image) workgroups of 4 waves (6 at the server-default shape).  A launch whose workgroups
// do not all fit runs the surplus in a second round almost alone -- latency-bound, about one lone-workgroup
// duration (measured 48 us of a 161 us launch at 1024 clients with H = 8: 32 x 49 = 1568 workgroups on 1536
// slots).  Taller tiles trade a little per-wave time for fewer workgroups: pick the height whose launch costs
// least in (waves on the busiest SIMD) x (work per wave).  Classes with fewer than 8 clients use one small
// tile.
int xl_pick_tile_height(const XlPlanOpts &o, const std::vector<DirectClass> &classes) {
  int big_h = 8;
  size_t lds1 = 0;
  for (const DirectClass &cs : classes)
    if (cs.members.size() >= 8) lds1 = std::max(lds1, xl_fir_lds_bytes_ota(cs.D, xl_roundup(cs.T, 12), 64));
  if (lds1 > 0) {
    const long slots = std::max<long>(1, std::min<long>((long)(160 * 1024 / lds1), 7));
    const long cap = slots * 256;
    long best = -1;
    static const int cand[4] = {8, 9, 10, 12};
    for (int h : cand) {
      long wgs = 0;
      for (const DirectClass &cs : classes) {
        const long n = (long)cs.members.size();
        if (n < 8) continue;
        const long kest = o.max_samples / cs.D + 1;
        wgs += (((n + h - 1) / h + XL_NW_MAX - 1) / XL_NW_MAX) * ((kest + 63) / 64);
      }
      const long full = wgs / cap, rem = wgs % cap;
      long cost = full * slots * h;
      if (rem) cost += std::max<long>((rem + 255) / 256, 3) * h;
      if (best < 0 || cost < best) {
        best = cost;
        big_h = h;
      }
    }
  }
  if (o.exp_h == 8 || o.exp_h == 9 || o.exp_h == 10 || o.exp_h == 12) big_h = o.exp_h;
  return big_h;
}

// Transform length of a polyphase class: the mix launch streams D x M branch-spectrum values per client and call from HBM,
// which is what bounds it with many clients and one block per call; M = 128 halves that for ~5-10 % more arithmetic
// (valid outputs per segment M - A + 1) while the filter is short against the segment.  Measured at D = 42, 505 taps, one
// block per call: x1.17 at 4096 clients, x1.08 at 2048, x1.015 at 1024, x0.99 at 512 and below.
// M = 64 (round 6): classes of more than 64 branches (9+ k-blocks of 8: the wide two-half mix, D = 65 .. 112; the float32 mixes above
// that or on request) with up to 8 taps per branch (57+ of 64 outputs per segment valid).  A wide workgroup holds 104 KB of operands for ONE bin of 128 columns, and half the bins is half the workgroups
// and half the operand stream (config 5 at 1024 clients: 512 workgroups = ONE round instead of two): config 5 (cf32, D = 100, 3 taps
// per branch) 8 blocks per call at 1024 / 2048 / 4096 clients 16.9 / 29.1 / 51.0 -> 16.0 / 26.2 / 47.4 us per block, ONE block per call
// 48.4 -> 40.8 (4096 clients: 138 -> 94); D = 72 / 100 off cu8 streams with 3 / 5 / 8 taps per branch: ahead or level at 1024 and 4096
// clients; at 128-768 clients level with 128 and ahead of 256 (which the rule above picked there: 12.0 / 39.4 against 11.9 / 29.1 us
// per block at 256 clients x 8 / 1 blocks per call).  Narrow classes (D <= 64) LOSE with 64 points (D = 64, 4096 clients: 59.4 -> 65.6):
// their workgroups hold less and the inverse launch, whose tiles stay 32 KB, gains nothing.  The float32 mixes gain too (config 5 with
// mix_kernel = 3: -4 %; D = 128 / 200 on the streamed kernel: -9 / -17 % at 1024 clients, -6 / -11 % at 256); 10-13 taps per branch: level
// (not taken).  profiles/r06_transform_length_64.txt
uint32_t xl_poly_pick_m(const XlPlanOpts &o, uint32_t A, size_t members, uint32_t D) {
  if (A > 64) return 256u;
  if (o.poly_m) return A > 32 && o.poly_m == 64u ? 128u : o.poly_m;  // (forced; a class needs A <= M / 2)
  const uint32_t nkb = (D + 7u) / 8u;
  if (nkb > XLP_NKB_4W && A <= 8) return 64u;
  return A <= 32 && members >= 768 ? 128u : 256u;
}

// Which mix launch a class of D branches takes (PolyClass::mix_kind): the two-half kernel (1) carries the spectra as pairs of halves
// -- bounded by the input format, or (cf32 streams) scaled per segment by what the forward launch found (PolyClass::d_segmax) -- and
// holds at most XLP_NKB_MAX k-blocks of 8 branches (D <= 112); the float32 matrix instruction (3) has no such condition: it is what
// D > 112 takes, and every class on request (option "mix_kernel" = 3: all-float32 products).
uint32_t xl_poly_mix_kind(const XlPlanOpts &o, uint32_t D) {
  const bool halves_ok = D <= 8u * XLP_NKB_MAX;
  return (o.mix_kernel == 3u || !halves_ok) ? 3u : 1u;
}

// Whether a class's shared spectra are kept in the two-half mix's operand form (PolyClass::ximg, option "mix_operand_image"): where
// the form exists (xlp_ximg_eligible: a constant scale and xlp_mix_mfma_kernel as the only reader) and, unless the option forces it,
// where it measured ahead (xlp_ximg_pays, xl_plan_rules.h).
bool xl_poly_ximg(const XlPlanOpts &o, uint32_t D, uint32_t M, size_t members) {
  if (o.mix_img == 0 || !xlp_ximg_eligible((uint32_t)o.fmt, xl_poly_mix_kind(o, D), (D + 7u) / 8u, M)) return false;
  return o.mix_img > 0 || xlp_ximg_pays((uint32_t)members, o.gcap);
}

// Power-of-two scale of a column's branch spectra for the matrix-core mix: every component of R_b[m] = sum_a r_b[a] e^{..} is at
// most L = max_b sum_a |r_b[a]| (the same for the delayed taps: a delay permutes the branches); scale = 2^floor(log2(RMAX / L)).
float xl_poly_col_scale(const Client &c, uint32_t D, uint32_t T) {
  std::vector<double> l1(D, 0.0);
  for (uint32_t i = 0; i < T; ++i) l1[i % D] += hypot((double)c.rt[2 * i], (double)c.rt[2 * i + 1]);
  double L = 0.0;
  for (double v : l1) L = std::max(L, v);
  if (!(L > 0.0) || !std::isfinite(L)) return 1.0f;
  int e = (int)floor(log2((double)XLP_H_RMAX / L));
  e = std::max(-100, std::min(100, e));
  return (float)ldexp(1.0, e);
}

// Polyphase classes (optimized mode): all mature clients of one (D, T) -- many clients (its lanes are client
// columns and its cost per client does not depend on the tap count) with a filter long enough to be worth it
void xl_poly_form_classes(const XlPlanOpts &o, const std::vector<Client> &clients, std::vector<PolyClass> &prev, uint32_t advanced,
                          std::vector<PolyClass> *next, std::vector<XlPolyPending> *pending, std::vector<bool> *rest_use) {
  for (PolyClass &pc : prev) pc.keep = false;
  std::map<std::tuple<uint32_t, uint32_t, uint32_t>, std::vector<int>> by_shape;
  for (size_t i = 0; i < clients.size(); ++i) {
    const Client &c = clients[i];
    if (c.alive && !c.wide) by_shape[std::make_tuple(c.D, c.T, c.planned_mature ? XL_HCAP : (uint32_t)c.consumed)].push_back((int)i);
  }
  for (auto &kv : by_shape) {
    const uint32_t D = std::get<0>(kv.first), T = std::get<1>(kv.first), hv0 = std::get<2>(kv.first);
    const std::vector<int> &m = kv.second;
    std::vector<uint32_t> rems;
    for (int id : m) rems.push_back((uint32_t)(clients[id].consumed % D));
    std::vector<uint32_t> distinct(rems);
    std::sort(distinct.begin(), distinct.end());
    distinct.erase(std::unique(distinct.begin(), distinct.end()), distinct.end());
    // An existing class of this shape whose members are (mostly) still here: same (D, T), same kind (mature), or the
    // immature class these very clients formed when they joined together.  Its shared grid moved with the stream.
    PolyClass *old = nullptr;
    for (PolyClass &oc : prev) {
      if (oc.keep || oc.D != D || oc.T != T) continue;
      const bool same_kind = oc.hv0 == hv0 || (hv0 == XL_HCAP && oc.hv0 != XL_HCAP && !m.empty() && oc.col_of.count(m[0]));
      if (same_kind) {
        old = &oc;
        break;
      }
    }
    uint32_t ref = 0, dmax = 0;
    bool reuse = false;
    if (old != nullptr) {
      ref = (old->rem_ref0 + advanced % D) % D;
      for (uint32_t r : distinct) dmax = std::max(dmax, (ref + D - r) % D);
      const uint32_t A = (T + dmax + D - 1) / D;
      reuse = A == old->A && xl_poly_pick_m(o, A, m.size(), D) == old->M && xl_poly_mix_kind(o, D) == old->mix_kind &&
              xl_poly_ximg(o, D, old->M, m.size()) == old->ximg;
    }
    if (!reuse) {
      // the shared grid's reference: the member offset that keeps the largest delay of a member smallest
      uint32_t best_ref = distinct[0], best_dmax = 0xFFFFFFFFu;
      for (uint32_t cand : distinct) {
        uint32_t dm = 0;
        for (uint32_t r : distinct) dm = std::max(dm, (cand + D - r) % D);  // delta = (j0_c - j0_ref) mod D = (rem_ref - rem_c) mod D
        if (dm < best_dmax) best_dmax = dm, best_ref = cand;
      }
      ref = best_ref, dmax = best_dmax;
    }
    const uint32_t A = (T + dmax + D - 1) / D;
    const uint32_t M = xl_poly_pick_m(o, A, m.size(), D);
    const bool fits = A >= 2 && A <= M / 2 && D <= 504;
    // crossover: with the mix on the matrix cores the path costs the same whatever the filter length and little beside the
    // recurrence in small classes (A/B at 8 blocks per call, direct kernel -> polyphase, us per block: 101 taps 37.3 -> 28.2 at
    // 1024 clients, 124.8 -> 88.7 at 4096, 23.3 -> 22.9 at 128; 505 taps 24.8 -> 22.9 at 96 clients, 23.1 -> 22.7 at 32; cf32 10
    // Msps, D = 100, 257 taps: 38.4 -> 23.4 at 1024 clients, 12.8 -> 11.8 at 256, 11.4 -> 11.3 at 64): 2 taps per branch, 32 clients
    // Classes of more than XLMF_NB8_MAX k-blocks (D > 112: float32 operands re-streamed every pass, xlp_mix_f32_stream_kernel): the
    // same 2 taps per branch from 128 clients on -- measured in round 6 at D = 128 / 200 / 400, 1.2 / 2.4 / 4.8 / 12 taps per branch,
    // 32 .. 1024 clients (profiles/r06_plan_rules_other_shapes.txt): the path costs 10.6-11.5 us per block up to 128 clients whatever
    // the filter, the direct kernel 11.4-11.9 at 128 clients x 2.4 taps per branch (1.04-1.07 x) and 47-62 at 1024 (1.6-2.1 x; rounds
    // 4-5 sent those to the direct kernel: 4.5 taps per branch was the only crossover a measurement of that kernel stood behind);
    // at 64 clients the direct kernel is still ahead up to 4.8 taps per branch.
    const bool streamed = (D + 7u) / 8u > XLMF_NB8_MAX;
    const size_t min_clients = o.poly_min_set ? o.poly_min_clients : (streamed ? 128u : 32u);
    const bool pays = m.size() >= min_clients && T >= 2 * D;
    if (o.poly_mode == 0 || !fits || (o.poly_mode < 0 && !pays)) continue;
    PolyClass pc;
    XlPolyPending pd;
    pd.fresh = !reuse;
    if (reuse) {
      pc = std::move(*old);
      old->keep = true;
      old->d_X = old->d_Y = nullptr;
      old->d_segmax = nullptr;
      old->d_cols = nullptr;
      old->d_Rh = nullptr;
      old->d_cscale = nullptr;
      // members that left give their columns back
      std::vector<bool> here(clients.size(), false);
      for (int id : m) here[id] = true;
      for (auto it = pc.col_of.begin(); it != pc.col_of.end();) {
        if (!here[it->first]) {
          pc.col_client[it->second] = -1;
          it = pc.col_of.erase(it);
        } else {
          ++it;
        }
      }
      while (!pc.col_client.empty() && pc.col_client.back() < 0) {  // (trailing free columns shrink the class)
        pc.col_client.pop_back();
        pc.col_delta.pop_back();
        pc.col_uid.pop_back();
      }
      pc.col_scale.resize(pc.col_client.size(), 1.0f);
    } else {
      pc.D = D;
      pc.Dpad = xl_roundup(D, XLP_BSTEP);
      pc.T = T;
      pc.A = A;
      pc.M = M;
      pc.V = M - A + 1;
      pc.mix_kind = xl_poly_mix_kind(o, D);
      pc.nkb = (D + 7u) / 8u;
      pc.ximg = xl_poly_ximg(o, D, M, m.size());
    }
    pc.keep = false;
    pc.rem_ref0 = ref;
    pc.hv0 = hv0;
    pc.dmax = dmax;
    pc.members = m;
    // newcomers (and, for a recycled client id, a changed delay) take the free columns first, then new ones
    size_t next_free = 0;
    for (int id : m) {
      const uint32_t delta = (ref + D - (uint32_t)(clients[id].consumed % D)) % D;
      auto it = pc.col_of.find(id);
      if (it != pc.col_of.end() && pc.col_delta[it->second] == delta && pc.col_uid[it->second] == clients[id].uid) continue;
      uint32_t col;
      if (it != pc.col_of.end()) {
        col = it->second;
      } else {
        while (next_free < pc.col_client.size() && pc.col_client[next_free] >= 0) ++next_free;
        if (next_free == pc.col_client.size()) {
          pc.col_client.push_back(-1);
          pc.col_delta.push_back(0);
          pc.col_uid.push_back(0);
        }
        col = (uint32_t)next_free;
        pc.col_client[col] = id;
        pc.col_of[id] = col;
      }
      pc.col_delta[col] = delta;
      pc.col_uid[col] = clients[id].uid;
      pd.new_cols.push_back(col);
    }
    pc.ncols = (uint32_t)pc.col_client.size();
    pd.idx = next->size();
    next->push_back(std::move(pc));
    pending->push_back(std::move(pd));
    for (int id : m) (*rest_use)[id] = false;
  }
}

// CU reservation for the side-stream chain kernel (64 clients per workgroup = per CU, dealt round-robin to the 8 XCDs): how many
// CUs per XCD the plan wants, and the band of the rule it is in.
XlReserve xl_reserve_want(const XlPlanOpts &o, size_t nclients, const std::vector<DirectClass> &classes_rest,
                          const std::vector<PolyClass> &poly, double macs_all, double macs_rest, int last_band, bool exp_nomask,
                          bool exp_rounds1, int exp_reserve) {
  const uint32_t nwg = ((uint32_t)nclients + 63u) / 64u;
  const bool light = xl_direct_is_light(macs_all * o.max_samples) || (!poly.empty() && xl_direct_is_light(macs_rest * o.max_samples));
  // (one-block calls of a polyphase plan take the side stream too, up to XL_SIDE_ONE_BLOCK_MAX clients: xl_side_call, xl_plan.h)
  const bool one_block_side = !poly.empty() && nclients <= XL_SIDE_ONE_BLOCK_MAX;
  // (a server that knows how many clients it admits says so -- option "expected_clients" --, and the reservation is made for
  // that many at once: the 25 ms of a stream re-creation then never fall on a call between two joins)
  const uint32_t nwg_res = std::max(nwg, (o.expected_clients + 63u) / 64u);
  // (one CU per chain workgroup while the recurrence bounds the call, none in a band above that, beyond it the chain launch runs in
  // rounds on fewer CUs -- by the plan's load: launch time per unit of chain time, in clients of the measured shape: xl_plan_rules.h)
  uint32_t load_wgs = nwg_res;
  if (!poly.empty() && o.gcap >= 2) {  // (engines of one-block calls: the bands as measured by client count -- their calls are short, and nothing else was measured)
    double ps = macs_rest * (double)o.max_samples * 72.0;  // (direct-kernel clients of an optimized call: ~0.072 ns per complex MAC)
    uint32_t kmax = 1u;
    for (const PolyClass &pc : poly) {
      const uint32_t K = (o.max_samples + pc.D - 1u) / pc.D;
      ps += (double)pc.members.size() * xl_client_launch_ps(pc.M, K, pc.V, 8u * pc.nkb, pc.mix_kind, o.gcap);
      kmax = std::max(kmax, K);
    }
    for (const DirectClass &cs : classes_rest) kmax = std::max(kmax, (o.max_samples + cs.D - 1u) / cs.D);
    // (scaled to the population the CUs are reserved for: option "expected_clients")
    load_wgs = xl_plan_load_wgs(ps * (double)nwg_res / (double)std::max(nwg, 1u), kmax);
  }
  // (the bands have edges where the reservation jumps: stay in the band of the previous plan until the load is two workgroups past one)
  load_wgs = xl_chain_load_with_hysteresis(load_wgs, last_band);
  const bool side_plan = (o.gcap >= 2 || one_block_side) && (!poly.empty() || light || o.nco_side > 0) && o.nco_side != 0;
  // (the no-reservation band and the rounds were measured on polyphase plans only; a direct-only plan -- whose side-stream chain needs
  // the masked pair, see xl_side_call -- keeps one CU per chain workgroup, up to half the chip)
  uint32_t want = !side_plan ? 0u : (poly.empty() ? ((nwg_res + 7u) / 8u <= 16u ? (nwg_res + 7u) / 8u : 0u) : xl_chain_reserve_per_xcd(nwg_res, load_wgs));
  // A wide two-half class (9 .. 14 k-blocks: xl_mixh2.hip) runs two workgroups per CU and launches M x column groups of them -- a
  // multiple of 512 at every 512 clients: on the 240 CUs a reservation of 16 leaves, BASELINE config 5 at 1024 clients took a third,
  // quarter-full round of workgroups (56 us per mix launch; the launch's own timeline: profiles/r06_mix_wide_timeline.txt) -- and its
  // forward and inverse launches lose a sixteenth of the chip as well.  No reservation for such plans: the chain workgroups take CUs as
  // the launches' tails free them (as in the 33..47 band of the rule).
  for (const PolyClass &pc : poly)
    if (pc.mix_kind == 1u && pc.nkb > XLP_NKB_4W) want = 0u;
  if (exp_nomask) want = 0u;
  if (want > 0u && exp_rounds1) want = std::min(16u, (nwg_res + 7u) / 8u);  // (tuning: round 3's rule, one CU per chain workgroup)
  if (want > 0u && exp_reserve >= 0) want = std::min(want, (uint32_t)exp_reserve);  // (tuning: fewer CUs, more rounds)
  return XlReserve{want, xl_chain_band(load_wgs)};
}

// Whether the masked stream pair is re-created for `want` CUs per XCD when `reserve_r` are held
// (creating a masked stream pair takes ~25 ms: grow at once, shrink only when two CUs per XCD too many are held, so that
// a client count hovering around a multiple of 512 does not recreate the streams at every join and leave)
bool xl_reserve_recreate(uint32_t want, uint32_t reserve_r) {
  return want > reserve_r || want + 2u <= reserve_r || (want == 0u && reserve_r != 0u);
}
