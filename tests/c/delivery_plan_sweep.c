/* tests/c/delivery_plan_sweep.c -- the delivery batch's layout (csrc/xl_delivery_plan.h) held to its contract, compiled by
 * tests/test_delivery_cpu.py with -fsanitize=address,undefined and run as a process of its own.  Over row sizes 0 .. 80 bytes in steps
 * of 4 at source residues 0, 4, 8, 12 mod 16 (every row alone, every ordered pair), rows of chunk - 4, chunk, chunk + 4 and
 * 2 chunk + 4 bytes at every residue and between short rows, empty rows first, last and in runs, and n = 0, 1, 2 and 1025, it asserts:
 * a row's offset is congruent to its source mod 16 and lies 0 .. 12 bytes behind its predecessor's end (rows do not overlap); the image
 * is as long as the last row's end, the rows plus at most 12 bytes each; the runs are the non-empty rows in order with s16 = off / 16,
 * nondecreasing from 0 (what xl_ragged_find needs); and walking every chunk the way the kernel does -- the search, xl_dlv_first, then
 * xl_dlv_span of every run up to the chunk's end -- touches every dword of every row exactly once, no dword outside a row, and never
 * more than XL_DLV_CHUNK / 16 slots of one run in one chunk, all inside the chunk.  Prints "ok <batches checked>". */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "xl_delivery_plan.h"

#define CHECK(c)                                                              \
  do {                                                                        \
    if (!(c)) {                                                               \
      fprintf(stderr, "line %d: %s (batch %ld)\n", __LINE__, #c, g_batches);  \
      exit(1);                                                                \
    }                                                                         \
  } while (0)

static long g_batches = 0;

/* xl_ragged.h's search, in C: the last run whose sum is <= key */
static uint32_t find(const XlDlvRun *runs, uint32_t nruns, uint32_t key) {
  uint32_t hi = nruns, lo = 0u;
  while (hi - lo > 1u) {
    const uint32_t mid = (lo + hi) / 2u;
    if (runs[mid].s16 <= key) lo = mid;
    else hi = mid;
  }
  return lo;
}

static void check(size_t n, const uint64_t *src, const uint64_t *bytes) {
  uint64_t *off = malloc((n + 1) * sizeof(*off));
  XlDlvRun *runs = malloc((n + 1) * sizeof(*runs));
  size_t nruns = 0;
  uint64_t total = 0, end = 0, sum = 0;
  CHECK(off && runs);
  CHECK(xl_dlv_plan(n, src, bytes, off, runs, &nruns, &total) == 0);
  size_t k = 0;
  for (size_t i = 0; i < n; ++i) {
    if (bytes[i] == 0) {
      CHECK(off[i] == ~(uint64_t)0);
      continue;
    }
    CHECK(off[i] % 16 == src[i] % 16);
    CHECK(off[i] >= end && off[i] - end <= 12);
    CHECK(k < nruns && runs[k].src == src[i] && runs[k].off == off[i] && runs[k].bytes == bytes[i] && runs[k].s16 == off[i] / 16);
    CHECK(k == 0 ? runs[k].s16 == 0 : runs[k].s16 >= runs[k - 1].s16);
    ++k;
    end = off[i] + bytes[i];
    sum += bytes[i];
  }
  CHECK(k == nruns && total == end && total <= sum + 12 * nruns);
  /* the kernel's walk */
  const uint64_t words = total / 4;
  CHECK(total % 4 == 0);
  uint8_t *cover = calloc(words + 1, 1);
  int32_t *owner = malloc((words + 1) * sizeof(*owner));
  CHECK(cover && owner);
  memset(owner, 0xff, (words + 1) * sizeof(*owner));
  for (size_t r = 0; r < nruns; ++r)
    for (uint64_t q = runs[r].off; q < runs[r].off + runs[r].bytes; q += 4) owner[q / 4] = (int32_t)r;
  const uint32_t chunks = xl_dlv_chunks(total);
  CHECK((uint64_t)chunks * XL_DLV_CHUNK >= total && (chunks == 0 || (uint64_t)(chunks - 1) * XL_DLV_CHUNK < total));
  for (uint32_t c = 0; c < chunks && nruns > 0; ++c) {
    const uint64_t lo = (uint64_t)c * XL_DLV_CHUNK, hi = lo + XL_DLV_CHUNK;
    for (uint32_t r = xl_dlv_first(runs, find(runs, (uint32_t)nruns, c * (XL_DLV_CHUNK / 16u)), c); r < nruns; ++r) {
      if (runs[r].off >= hi) break;
      uint64_t a, b;
      if (!xl_dlv_span(&runs[r], c, &a, &b)) continue;
      const uint64_t sa = a & ~(uint64_t)15, sb = (b + 15) & ~(uint64_t)15;
      CHECK(sa >= lo && sb <= hi && (sb - sa) / 16 <= (uint64_t)XL_DLV_THREADS * XL_DLV_SLOTS_PER_THREAD);
      CHECK(a >= runs[r].off && b <= runs[r].off + runs[r].bytes && a % 4 == 0 && b % 4 == 0);
      for (uint64_t q = a; q < b; q += 4) {
        CHECK(owner[q / 4] == (int32_t)r);
        cover[q / 4]++;
      }
    }
  }
  for (uint64_t w = 0; w < words; ++w) CHECK(cover[w] == (owner[w] >= 0 ? 1 : 0));
  free(owner), free(cover), free(runs), free(off);
  ++g_batches;
}

static uint64_t g_lcg = 12345;
static uint32_t rnd(void) {
  g_lcg = g_lcg * 6364136223846793005ull + 1442695040888963407ull;
  return (uint32_t)(g_lcg >> 33);
}

int main(void) {
  const uint64_t base = 0x7f0000000000ull, C = XL_DLV_CHUNK;
  const uint64_t edge[4] = {C - 4, C, C + 4, 2 * C + 4};
  uint64_t src[1025], bytes[1025];
  CHECK(XL_DLV_CHUNK % 16 == 0 && XL_DLV_CHUNK / 16 == XL_DLV_THREADS * XL_DLV_SLOTS_PER_THREAD);
  check(0, src, bytes); /* n = 0 */
  /* n = 1 and n = 2: every size at every residue, every ordered pair */
  for (uint64_t s0 = 0; s0 <= 80; s0 += 4)
    for (uint64_t r0 = 0; r0 < 16; r0 += 4) {
      src[0] = base + 4096 + r0, bytes[0] = s0;
      check(1, src, bytes);
      for (uint64_t s1 = 0; s1 <= 80; s1 += 4)
        for (uint64_t r1 = 0; r1 < 16; r1 += 4) {
          src[1] = base + 65536 + r1, bytes[1] = s1;
          check(2, src, bytes);
        }
    }
  /* the chunk's edges: alone, behind and in front of a short row of every size, at every residue */
  for (int e = 0; e < 4; ++e)
    for (uint64_t r0 = 0; r0 < 16; r0 += 4) {
      src[0] = base + r0, bytes[0] = edge[e];
      check(1, src, bytes);
      for (uint64_t s1 = 0; s1 <= 80; s1 += 4)
        for (uint64_t r1 = 0; r1 < 16; r1 += 4) {
          src[0] = base + r0, bytes[0] = edge[e], src[1] = base + (1 << 20) + r1, bytes[1] = s1;
          check(2, src, bytes);
          src[0] = base + (1 << 20) + r1, bytes[0] = s1, src[1] = base + r0, bytes[1] = edge[e];
          check(2, src, bytes);
          /* three: short, edge, short -- the edge row ends wherever the short one pushed it */
          src[2] = base + (2 << 20) + r1, bytes[2] = s1;
          check(3, src, bytes);
        }
    }
  /* empty rows first, last and in runs; short rows that share slots across a chunk's start; n = 1025 */
  for (int round = 0; round < 200; ++round) {
    const size_t n = round % 4 == 0 ? 1025 : 1 + rnd() % 1025;
    const int mode = round % 5;
    for (size_t i = 0; i < n; ++i) {
      src[i] = base + (uint64_t)i * (1 << 18) + 4 * (rnd() % 4);
      const uint32_t x = rnd() % 100;
      if (mode == 0) bytes[i] = 4 * (rnd() % 21);                                /* 0 .. 80 */
      else if (mode == 1) bytes[i] = x < 30 ? 0 : 4 * (1 + rnd() % 4);            /* tiny rows and runs of empty ones */
      else if (mode == 2) bytes[i] = x < 5 ? edge[rnd() % 4] : 4 * (rnd() % 21);  /* an edge row now and then */
      else if (mode == 3) bytes[i] = 4 * (1 + rnd() % 1000);                      /* a few KB */
      else bytes[i] = x < 50 ? 0 : 4;                                             /* half empty, the rest one dword */
    }
    if (round % 3 == 0) bytes[0] = 0, bytes[n - 1] = 0;
    if (round % 3 == 1 && n > 40)
      for (size_t i = 10; i < 40; ++i) bytes[i] = 0;
    check(n, src, bytes);
  }
  /* all rows empty */
  for (size_t i = 0; i < 1025; ++i) bytes[i] = 0;
  check(1025, src, bytes);
  /* refusals: alignment of the address and of the length */
  {
    uint64_t off[1];
    XlDlvRun run[1];
    size_t nr;
    uint64_t tot;
    src[0] = base + 2, bytes[0] = 8;
    CHECK(xl_dlv_plan(1, src, bytes, off, run, &nr, &tot) == -1);
    src[0] = base, bytes[0] = 6;
    CHECK(xl_dlv_plan(1, src, bytes, off, run, &nr, &tot) == -1);
    bytes[0] = XL_DLV_ROW_MAX + 4;
    CHECK(xl_dlv_plan(1, src, bytes, off, run, &nr, &tot) == -1);
  }
  printf("ok %ld\n", g_batches);
  return 0;
}
