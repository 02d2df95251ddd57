// tests/c/chain_cover8_sweep.cpp -- stand-alone host program (its own main; tests/test_chain_cover8_cpu.py builds it with ASan + UBSan
// and runs it): the chain wave's cover of a region with aligned 8-entry runs in its head and tail (xl_chain_plan8, csrc/xl_chain_plan.h)
// for every first entry e in 0 .. 191 and every length 0 .. 300, replayed the way the kernel walks it -- any-slot entries, 8-entry runs,
// 32-entry blocks, 8-entry runs, any-slot entries -- into a ring of 64 slots.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "xl_chain_plan.h"

static const uint32_t RING = 64u, BLOCK = 32u, RUN = 8u, E_END = 192u, LEN_MAX = 300u;

#define CHECK(cond)                                                                                                             \
  do {                                                                                                                          \
    if (!(cond)) {                                                                                                              \
      fprintf(stderr, "FAIL %s (e %u len %u: head1 %u head8 %u blocks %u tail8 %u tail1 %u)\n", #cond, e, len, pl.head1, pl.head8, \
              pl.blocks, pl.tail8, pl.tail1);                                                                                   \
      return 1;                                                                                                                 \
    }                                                                                                                           \
  } while (0)

int main(void) {
  unsigned long cases = 0;
  for (uint32_t e = 0; e < E_END; ++e) {
    for (uint32_t len = 0; len <= LEN_MAX; ++len, ++cases) {
      const uint32_t e_stop = e + len;
      const XlChainPlan8 pl = xl_chain_plan8(e, e_stop, RING, BLOCK, RUN);
      const XlChainPlan old = xl_chain_plan(e, e_stop, RING, BLOCK);
      CHECK(pl.head1 + RUN * pl.head8 + BLOCK * pl.blocks + RUN * pl.tail8 + pl.tail1 == len);  // the five parts are the region
      CHECK(pl.head1 < RUN && pl.tail1 < RUN && pl.head8 <= 3u && pl.tail8 <= 3u);
      CHECK(pl.head1 + RUN * pl.head8 < BLOCK && RUN * pl.tail8 + pl.tail1 < BLOCK);  // head and tail: one drain check each covers them
      CHECK(pl.blocks == old.blocks && pl.head1 + RUN * pl.head8 + RUN * pl.tail8 + pl.tail1 == old.head + old.tail);  // the blocks are xl_chain_plan's
      // replay: `order` receives the entries in the order they are written; `slots` is the ring (a write past it is ASan's to see)
      std::vector<uint32_t> order, slots(RING, 0xFFFFFFFFu);
      uint32_t ee = e;
      const auto singles = [&](uint32_t n) {
        for (uint32_t i = 0; i < n; ++i, ++ee) {
          slots[ee & (RING - 1u)] = ee;
          order.push_back(ee);
        }
      };
      const auto runs = [&](uint32_t n, uint32_t width, bool &ok) {
        for (uint32_t b = 0; b < n; ++b) {
          const uint32_t slot = ee & (RING - 1u);
          ok = ok && slot % width == 0u && slot + width <= RING;  // starts at a multiple of its width, immediates stay inside the ring
          for (uint32_t i = 0; i < width; ++i, ++ee) {
            slots.at(slot + i) = ee;
            order.push_back(ee);
          }
        }
      };
      bool ok = true;
      singles(pl.head1);
      runs(pl.head8, RUN, ok);
      runs(pl.blocks, BLOCK, ok);
      runs(pl.tail8, RUN, ok);
      singles(pl.tail1);
      CHECK(ok);
      CHECK(ee == e_stop && order.size() == (size_t)len);  // every entry once ...
      for (size_t i = 0; i < order.size(); ++i) CHECK(order[i] == e + (uint32_t)i);  // ... and in order
      // the any-slot entries run to the next multiple of 8 slots and no further; behind a block the runs come first
      if (pl.head8 + pl.blocks + pl.tail8 != 0u) CHECK(pl.head1 == ((RUN - (e & (RUN - 1u))) & (RUN - 1u)));
      if (len == 0u) CHECK(pl.head1 + pl.head8 + pl.blocks + pl.tail8 + pl.tail1 == 0u);
    }
  }
  printf("ok %lu\n", cases);
  return 0;
}
