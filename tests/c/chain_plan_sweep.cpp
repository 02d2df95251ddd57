// tests/c/chain_plan_sweep.cpp -- stand-alone host program (its own main; tests/test_chain_plan_cpu.py builds it with ASan + UBSan and
// runs it): the chain wave's cover of a region (csrc/xl_chain_plan.h) for every (e, e_stop) with 0 <= e <= e_stop <= 400, replayed the
// way the kernel walks it -- head of any-slot entries, 32-entry blocks, tail -- into a ring of 64 slots.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "xl_chain_plan.h"

static const uint32_t RING = 64u, BLOCK = 32u, EMAX = 400u;

#define CHECK(cond)                                                                                        \
  do {                                                                                                     \
    if (!(cond)) {                                                                                         \
      fprintf(stderr, "FAIL %s (e %u e_stop %u head %u blocks %u tail %u)\n", #cond, e, e_stop, pl.head, pl.blocks, pl.tail); \
      return 1;                                                                                            \
    }                                                                                                      \
  } while (0)

int main(void) {
  unsigned long cases = 0;
  for (uint32_t e = 0; e <= EMAX; ++e) {
    for (uint32_t e_stop = e; e_stop <= EMAX; ++e_stop, ++cases) {
      const XlChainPlan pl = xl_chain_plan(e, e_stop, RING, BLOCK);
      if (e == e_stop) CHECK(pl.head == 0u && pl.blocks == 0u && pl.tail == 0u);
      CHECK(pl.head < BLOCK && pl.tail < BLOCK);
      // replay: `order` receives the entries in the order they are written; `slots` is the ring (a write past it is ASan's to see)
      std::vector<uint32_t> order, slots(RING, 0xFFFFFFFFu);
      uint32_t ee = e;
      for (uint32_t i = 0; i < pl.head; ++i, ++ee) {
        slots[ee & (RING - 1u)] = ee;
        order.push_back(ee);
      }
      for (uint32_t b = 0; b < pl.blocks; ++b) {
        const uint32_t slot = ee & (RING - 1u);
        CHECK(slot == 0u || slot == 32u);       // a block starts at ring slot 0 or 32 only ...
        CHECK(slot + BLOCK <= RING);            // ... and its immediate offsets stay inside the ring
        for (uint32_t i = 0; i < BLOCK; ++i, ++ee) {
          slots.at(slot + i) = ee;
          order.push_back(ee);
        }
      }
      CHECK(pl.blocks == 0u || pl.head == ((BLOCK - (e & (BLOCK - 1u))) & (BLOCK - 1u)));  // the head is no longer than the way to the boundary
      for (uint32_t i = 0; i < pl.tail; ++i, ++ee) {
        slots[ee & (RING - 1u)] = ee;
        order.push_back(ee);
      }
      CHECK(ee == e_stop && order.size() == (size_t)(e_stop - e));  // every entry once ...
      for (size_t i = 0; i < order.size(); ++i) CHECK(order[i] == e + (uint32_t)i);  // ... and in order
      // a region shorter than head + one block has no block
      if (e_stop - e < BLOCK) CHECK(pl.blocks == 0u);
    }
  }
  printf("ok %lu\n", cases);
  return 0;
}
