// tests/c/direct_plan_probe.cpp -- stand-alone host program (its own main; tests/test_direct_fir_cases_cpu.py builds it with ASan + UBSan,
// links csrc/xl_plan.cpp alone and runs it): the direct-FIR launch set the planner builds for a population, printed.
//
//   direct_plan_probe <exp_h> <max_samples> <gcap>  D:T:count:consumed ...
//
// Every class D:T:count:consumed is `count` clients of decimation D and T taps that have seen `consumed` samples.  The program runs
// xl_direct_classes, xl_pick_tile_height (exp_h = XL_EXP_H, 0: the planner's own pick) and xl_build_launches, and prints per launch
// with groups
//   launch ct=<h> groups=<n> ota=<lanes> wide=<0|1> idle=<spare waves>
//   group D=<D> T=<T> Tpad=<Tpad> rem0=<r> hv0=<h> ntiles=<n> idle_before=<i> tiles=<c0,c1,..>
// and "ok <launches>" at the end.  The tap image is checked on the way: the row of client j of a tile holds that client's taps at
// [tap][client j] and zeros from T to Tpad and in the rows of a partial tile's missing clients.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "xl_plan.h"
#include "xl_common.h"
#include "xl_wide.h"

// (Defined beside the kernels in the library, xl_kernels.hip; this program links xl_plan.cpp alone: a second copy of the window
// image's size, as in plan_sweep.cpp, which tests/test_plan_cpu.py holds against the library's own function.)
size_t xl_fir_lds_bytes_ota(uint32_t D, uint32_t Tpad, uint32_t ota) { return ((size_t)(ota - 1u) * D + Tpad) * 8u; }

#define CHECK(cond)                                                  \
  do {                                                               \
    if (!(cond)) {                                                   \
      fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      exit(1);                                                       \
    }                                                                \
  } while (0)

int main(int argc, char **argv) {
  if (argc < 5) {
    fprintf(stderr, "usage: %s exp_h max_samples gcap D:T:count:consumed ...\n", argv[0]);
    return 2;
  }
  XlPlanOpts o;  // xlating_batch_t's defaults, polyphase off (the direct kernel carries every client)
  o.fmt = XLF_CU8, o.max_samples = (uint32_t)strtoul(argv[2], nullptr, 10), o.gcap = (uint32_t)strtoul(argv[3], nullptr, 10);
  o.poly_mode = 0, o.poly_min_set = false, o.poly_min_clients = 32, o.poly_m = 0, o.mix_kernel = 1, o.mix_img = -1;
  o.riders = true, o.riders_min_wgs = 512, o.exp_h = atoi(argv[1]), o.nco_side = -1, o.expected_clients = 0;
  o.q15_kernel = 0;

  std::vector<Client> clients;
  uint32_t rows_end = 0;
  for (int k = 4; k < argc; ++k) {
    unsigned D = 0, T = 0, count = 0;
    unsigned long long consumed = 0;
    if (sscanf(argv[k], "%u:%u:%u:%llu", &D, &T, &count, &consumed) != 4 || D == 0 || T == 0 || count == 0) {
      fprintf(stderr, "bad class '%s'\n", argv[k]);
      return 2;
    }
    CHECK(!xl_fir_needs_wide(D, T, 12u) && T - 1u + D <= XL_HCAP);  // a narrow client: the direct kernel's
    for (unsigned j = 0; j < count; ++j) {
      Client c;
      c.alive = true;
      c.uid = clients.size() + 1;
      c.D = D, c.T = T, c.Tpad = xl_roundup(T, XL_TAP_UNROLL);
      c.consumed = consumed;
      c.rt.assign(2 * (size_t)c.Tpad, 0.0f);
      for (uint32_t i = 0; i < T; ++i) c.rt[2 * i] = (float)c.uid, c.rt[2 * i + 1] = (float)(i + 1u);
      c.out_cap = o.gcap * (o.max_samples / D + 1);
      c.row_len = xl_roundup(c.out_cap, 2 * XL_PH_STRIDE);
      c.out_off = rows_end;
      rows_end += c.row_len;
      clients.push_back(c);
    }
  }

  std::vector<DirectClass> classes;
  xl_direct_classes(clients, std::vector<bool>(clients.size(), true), &classes);
  const int big_h = xl_pick_tile_height(o, classes);
  Launch Ls[XL_NLAUNCH];
  std::vector<float> image;
  CHECK(xl_build_launches(o, clients, Ls, classes, big_h, &image, nullptr) == 0);

  int nl = 0;
  size_t seen = 0;
  for (int li = 0; li < XL_NLAUNCH; ++li) {
    const Launch &L = Ls[li];
    if (L.groups.empty()) continue;
    ++nl;
    printf("launch ct=%d groups=%zu ota=%u wide=%d idle=%u\n", L.ct, L.groups.size(), L.ota, L.all_wide ? 1 : 0, L.idle_waves);
    CHECK(xl_fir_lds_bytes_ota(L.maxD, L.groups[0].Tpad, L.ota) > 0 && L.lds <= 160u * 1024u);
    for (const XlGroup &g : L.groups) {
      printf("group D=%u T=%u Tpad=%u rem0=%u hv0=%u ntiles=%u idle_before=%u tiles=", g.D, g.T, g.Tpad, g.rem0, g.hv0, g.ntiles,
             g.idle_before);
      CHECK(g.ntiles >= 1 && g.ntiles <= (uint32_t)L.nw && xl_fir_lds_bytes_ota(g.D, g.Tpad, L.ota) <= L.lds);
      for (uint32_t w = 0; w < g.ntiles; ++w) {
        const XlTile &t = g.tiles[w];
        printf("%s%u", w ? "," : "", t.nclients);
        CHECK(t.nclients >= 1 && t.nclients <= (uint32_t)L.ct);
        CHECK((size_t)2 * t.tap_off + (size_t)2 * g.Tpad * L.ct <= image.size());
        const float *img = image.data() + (size_t)2 * t.tap_off;
        for (uint32_t i = 0; i < g.Tpad; ++i)
          for (uint32_t j = 0; j < (uint32_t)L.ct; ++j) {
            const float re = img[((size_t)i * L.ct + j) * 2], im = img[((size_t)i * L.ct + j) * 2 + 1];
            if (i < g.T && j < t.nclients) {
              CHECK(im == (float)(i + 1u) && re >= 1.0f && re <= (float)clients.size());
              const Client &c = clients[(size_t)re - 1];
              CHECK(c.out_off == t.out_off[j] && c.D == g.D && c.T == g.T);
            } else {
              CHECK(re == 0.0f && im == 0.0f);  // pad taps and the rows of missing clients
            }
          }
        seen += t.nclients;
      }
      printf("\n");
    }
  }
  CHECK(seen == clients.size());
  printf("ok %d\n", nl);
  return 0;
}
