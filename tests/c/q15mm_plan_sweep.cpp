// A stand-alone sweep over xl_build_q15mm (sdr-server_amd/csrc/xl_plan.cpp): the host plan of the matrix-core Q15 launch, built by
// tests/test_q15_matrix_cpu.py with ASan and UBSan like tests/c/plan_sweep.cpp and run as a process of its own.  Random populations of
// clients over the shapes of the GPU tests and a few large decimations, some with a tap that has no int8 digit pair, some wide: after
// every plan the tiles partition exactly the eligible clients class by class, the image holds every tile's fragments and nothing
// else, every window image fits the launch's LDS budget, the float64 side keeps exactly the others, and a tile's rows carry the
// digits of ITS clients (spot-checked through xl_q15mm_entry).  Prints "ok <plans> <checks>".
#include <stdio.h>
#include <stdlib.h>

#include <set>

#include "xl_plan.h"

static unsigned long checks = 0;
#define CHECK(c)                                              \
  do {                                                        \
    ++checks;                                                 \
    if (!(c)) {                                               \
      printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);     \
      exit(1);                                                \
    }                                                         \
  } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(uint32_t n) {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return (uint32_t)((rng_state >> 11) % n);
}

size_t xl_fir_lds_bytes_ota(uint32_t D, uint32_t Tpad, uint32_t ota) { return ((size_t)(ota - 1u) * D + Tpad) * 8u; }  // (xl_kernels.hip's)

int main() {
  static const uint32_t shapes[][2] = {{42, 505}, {21, 253}, {7, 81}, {2, 7}, {3, 16}, {1, 1}, {64, 505}, {8, 81}, {1000, 12049}, {2900, 40}, {155, 9}};
  const size_t nshapes = sizeof shapes / sizeof shapes[0];
  unsigned long plans = 0;
  for (int round = 0; round < 60; ++round) {
    std::vector<Client> clients(1 + rnd(140));
    std::vector<bool> use(clients.size(), true);
    uint32_t row = 0;
    for (size_t i = 0; i < clients.size(); ++i) {
      Client &c = clients[i];
      const uint32_t *s = shapes[rnd((uint32_t)nshapes)];
      c.alive = rnd(10) != 0;
      c.D = s[0], c.T = s[1], c.Tpad = (c.T + 3u) & ~3u;
      c.wide = rnd(12) == 0;
      c.consumed = rnd(3) == 0 ? rnd(5) * 1000u : 1000000u + rnd(4);
      c.rtq.resize(2 * (size_t)c.T);
      for (int16_t &q : c.rtq) q = (int16_t)((int)rnd(65279) - 32639);
      if (rnd(6) == 0) c.rtq[rnd(2 * c.T)] = 32767;
      c.qmm_digits = xl_q15mm_admits_taps(c.rtq.data(), c.T) != 0;
      c.qincr[0] = (int16_t)rnd(32768), c.qincr[1] = (int16_t)rnd(32768);
      c.out_off = row;
      row += 64;
      if (c.wide) use[i] = false;
    }
    std::vector<DirectClass> classes;
    xl_direct_classes(clients, use, &classes);
    for (int fmt = XLF_CU8; fmt <= XLF_CS16; ++fmt) {
      XlPlanOpts o = {};
      o.fmt = fmt, o.max_samples = 131072, o.gcap = 8, o.q15_kernel = 1;
      XlQmmPlan plan;
      std::vector<bool> rest(use);
      xl_build_q15mm(o, clients, classes, &plan, &rest);
      ++plans;
      // who rides: alive, not wide, digits proved -- everybody else stays where they were
      uint32_t want = 0, digits = 0;
      for (size_t i = 0; i < clients.size(); ++i) {
        const bool elig = clients[i].alive && !clients[i].wide && clients[i].qmm_digits;
        want += elig;
        digits += clients[i].alive && !clients[i].wide && !clients[i].qmm_digits;
        CHECK(rest[i] == (use[i] && !elig));
      }
      CHECK(plan.nclients == want && plan.fb_digits == digits && plan.fb_window == 0);
      uint64_t frags = 0;
      uint32_t carried = 0;
      std::set<uint32_t> rows;
      for (const XlQmmTile &t : plan.tiles) {
        CHECK(t.nclients >= 1 && t.nclients <= XL_QMM_ROWS && t.frag_off == frags);
        CHECK(t.ksteps == xl_q15mm_ksteps(t.T) && xl_q15mm_acc_bounded(t.ksteps));
        CHECK(t.nc >= 1 && t.nc <= XL_QMM_COLS && (t.nc & (t.nc - 1)) == 0 && xl_q15mm_span(t.D, t.ksteps, t.nc) <= XL_QMM_LDS_SAMPLES);
        CHECK(t.nc == XL_QMM_COLS || xl_q15mm_span(t.D, t.ksteps, 2 * t.nc) > XL_QMM_LDS_SAMPLES);
        CHECK(xl_q15mm_lds_bytes(t, fmt) <= plan.lds && plan.lds <= 160 * 1024);
        frags += xl_q15mm_image_bytes(t.D, t.ksteps) / XL_QMM_FRAG;
        carried += t.nclients;
        for (uint32_t j = 0; j < t.nclients; ++j) {
          CHECK(rows.insert(t.out_off[j]).second);  // a client rides once
          const Client &c = clients[t.out_off[j] / 64];
          CHECK(c.alive && !c.wide && c.qmm_digits && c.D == t.D && c.T == t.T);
          CHECK(t.corr_r[j] == xl_q15mm_correction(c.rtq.data(), c.T, 0) && t.corr_i[j] == xl_q15mm_correction(c.rtq.data(), c.T, 1));
          // one entry of the row's image per residue and part: the digits of this client's delayed taps
          const uint32_t P = xl_q15mm_residues(t.D), r = rnd(P), kk = rnd(t.ksteps), h = rnd(2), e = rnd(16);
          const int part = (int)rnd(2);
          int32_t hi, lo;
          xl_q15mm_entry_digits(xl_q15mm_entry(c.rtq.data(), c.T, xl_q15mm_shift(t.D, r), part, 32u * kk + 16u * h + e), &hi, &lo);
          const uint64_t at = ((uint64_t)kk * 64u + (j + 32u * h)) * 16u + e;
          const int8_t *img = plan.image.data() + (size_t)t.frag_off * XL_QMM_FRAG;
          CHECK(img[(((uint64_t)r * 4u + 2u * (uint32_t)part) * t.ksteps) * XL_QMM_FRAG + at] == hi);
          CHECK(img[(((uint64_t)r * 4u + 2u * (uint32_t)part + 1u) * t.ksteps) * XL_QMM_FRAG + at] == lo);
        }
      }
      CHECK(carried == want && plan.image.size() == frags * XL_QMM_FRAG && frags <= 0xFFFFFFFFull);
    }
  }
  printf("ok %lu %lu\n", plans, checks);
  return 0;
}
