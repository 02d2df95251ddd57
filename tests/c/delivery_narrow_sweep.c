/* tests/c/delivery_narrow_sweep.c -- the narrowing delivery's two headers held to their contracts by a program of its own, compiled by
 * tests/test_delivery_narrow_cpu.py with gcc (with -fsanitize=address,undefined for the layout and for part of the rule).
 *
 *   delivery_narrow_sweep rule E0 E1
 *     csrc/xl_dlv_narrow.h against its libm restatement -- NaN -> 0, otherwise nearbyint((double)y * 32768.0) (the product is exact,
 *     the rounding mode is the default: to nearest, ties to even) clamped to -32768 .. 32767 -- on EVERY bit pattern whose exponent
 *     field lies in E0 .. E1: both signs, all 2^23 fractions.  The test covers the fields 0 .. 255 between its child processes: all
 *     2^32 patterns.  Prints "ok <patterns>".
 *   delivery_narrow_sweep layout
 *     csrc/xl_delivery_plan.h's narrowed layout (xl_dlv_plan_narrow) against brute force, in the way of delivery_plan_sweep.c: rows of
 *     0 .. 9 samples at source residues 0, 8, 16, 24 mod 32 (every row alone, every ordered pair), rows that end before, on and behind
 *     a chunk's end (4095, 4096, 4097 and 3 * 4096 + 5 samples) at every residue and between short rows, and random batches of up to
 *     1025 rows with empty rows first, last and in runs.  It asserts: a row's offset is congruent to (source mod 32) / 2 mod 16 and lies
 *     0 .. 12 bytes behind its predecessor's end; the image ends with the last row; the runs are the non-empty rows in order with
 *     s16 = off / 16 nondecreasing from 0; xl_dlv_first gives the first run that reaches into the chunk (found by a linear scan), or the run before it when that
 *     one ends in the padding in front of the chunk;
 *     walking every chunk the way the kernel does claims every image byte of every row for exactly one (chunk, run) span and no byte
 *     outside a row; xl_dlv_narrow_src of a claimed dword is the sample it came from, inside the source row, and of a whole slot is
 *     32-byte aligned; and the refusals (a source at 8k + 4, a row above the maximum).  Prints "ok <batches checked>". */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "xl_delivery_plan.h"
#include "xl_dlv_narrow.h"

static long g_batches = 0;

#define CHECK(c)                                                              \
  do {                                                                        \
    if (!(c)) {                                                               \
      fprintf(stderr, "line %d: %s (batch %ld)\n", __LINE__, #c, g_batches);  \
      exit(1);                                                                \
    }                                                                         \
  } while (0)

/* ------------------------------------------------------------------------------------------------------------------ the rule */
static int32_t want(uint32_t bits) {
  float y;
  memcpy(&y, &bits, 4);
  if (y != y) return 0;
  const double r = nearbyint((double)y * 32768.0);
  return r > 32767.0 ? 32767 : (r < -32768.0 ? -32768 : (int32_t)r);
}

static int rule(uint32_t e0, uint32_t e1) {
  unsigned long long n = 0;
  for (uint32_t e = e0; e <= e1; ++e)
    for (uint32_t sign = 0; sign < 2u; ++sign)
      for (uint32_t frac = 0; frac < (1u << 23); ++frac) {
        const uint32_t bits = (sign << 31) | (e << 23) | frac;
        const int32_t got = xl_dlv_narrow(bits), exp = want(bits);
        if (got != exp) {
          fprintf(stderr, "bits 0x%08x: got %d, expected %d\n", (unsigned)bits, (int)got, (int)exp);
          return 1;
        }
        ++n;
      }
  printf("ok %llu\n", n);
  return 0;
}

/* ---------------------------------------------------------------------------------------------------------------- the layout */
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

static void check(size_t n, const uint64_t *src, const uint64_t *cnt) {
  uint64_t *off = malloc((n + 1) * sizeof(*off));
  XlDlvRun *runs = malloc((n + 1) * sizeof(*runs));
  size_t nruns = 0;
  uint64_t total = 0, end = 0, sum = 0;
  CHECK(off && runs);
  CHECK(xl_dlv_plan_narrow(n, src, cnt, off, runs, &nruns, &total) == 0);
  size_t k = 0;
  for (size_t i = 0; i < n; ++i) {
    if (cnt[i] == 0) {
      CHECK(off[i] == ~(uint64_t)0);
      continue;
    }
    CHECK(off[i] % 16 == (src[i] % 32) / 2);
    CHECK(off[i] >= end && off[i] - end <= 12);
    CHECK(k < nruns && runs[k].src == src[i] && runs[k].off == off[i] && runs[k].bytes == 4 * cnt[i] && runs[k].s16 == off[i] / 16);
    CHECK(k == 0 ? runs[k].s16 == 0 : runs[k].s16 >= runs[k - 1].s16);
    ++k;
    end = off[i] + 4 * cnt[i];
    sum += 4 * cnt[i];
  }
  CHECK(k == nruns && total == end && total >= sum && total <= sum + 12 * nruns);
  /* the kernel's walk */
  const uint64_t words = total / 4;
  CHECK(total % 4 == 0);
  uint8_t *cover = calloc(words + 1, 1);
  int32_t *owner = malloc((words + 1) * sizeof(*owner));
  CHECK(cover && owner);
  memset(owner, 0xff, (words + 1) * sizeof(*owner));
  for (size_t r = 0; r < nruns; ++r)
    for (uint64_t q = runs[r].off; q < runs[r].off + runs[r].bytes; q += 4) {
      CHECK(owner[q / 4] < 0); /* (rows do not overlap) */
      owner[q / 4] = (int32_t)r;
    }
  const uint32_t chunks = xl_dlv_chunks(total);
  CHECK((uint64_t)chunks * XL_DLV_CHUNK >= total && (chunks == 0 || (uint64_t)(chunks - 1) * XL_DLV_CHUNK < total));
  for (uint32_t c = 0; c < chunks && nruns > 0; ++c) {
    const uint64_t lo = (uint64_t)c * XL_DLV_CHUNK, hi = lo + XL_DLV_CHUNK;
    const uint32_t first = xl_dlv_first(runs, find(runs, (uint32_t)nruns, c * (XL_DLV_CHUNK / 16u)), c);
    uint32_t brute = 0; /* the first run that ends behind the chunk's start: every chunk below the image's end has one */
    while (brute < nruns && runs[brute].off + runs[brute].bytes <= lo) ++brute;
    CHECK(brute < nruns && first <= brute); /* (no run with bytes in the chunk is skipped ...) */
    CHECK(first == brute || (first + 1 == brute && runs[brute].off >= lo + 16)); /* (... and at most one without is walked: the one
                                                                                    that ends in the padding before the chunk) */
    for (uint32_t r = first; r < nruns; ++r) {
      if (runs[r].off >= hi) break;
      uint64_t a, b;
      if (!xl_dlv_span(&runs[r], c, &a, &b)) continue;
      const uint64_t sa = a & ~(uint64_t)15, sb = (b + 15) & ~(uint64_t)15;
      CHECK(sa >= lo && sb <= hi && (sb - sa) / 16 <= (uint64_t)XL_DLV_THREADS * XL_DLV_SLOTS_PER_THREAD);
      CHECK(a >= runs[r].off && b <= runs[r].off + runs[r].bytes && a % 4 == 0 && b % 4 == 0);
      for (uint64_t q = a; q < b; q += 4) {
        CHECK(owner[q / 4] == (int32_t)r);
        cover[q / 4]++;
        const uint64_t at = xl_dlv_narrow_src(&runs[r], q);
        CHECK(at == runs[r].src + 8 * ((q - runs[r].off) / 4) && at + 8 <= runs[r].src + 2 * (uint64_t)runs[r].bytes);
      }
      for (uint64_t p = sa; p < sb; p += 16)
        if (p >= a && p + 16 <= b) CHECK(xl_dlv_narrow_src(&runs[r], p) % 32 == 0); /* a whole slot: one aligned 32-byte span */
    }
  }
  for (uint64_t w = 0; w < words; ++w) CHECK(cover[w] == (owner[w] >= 0 ? 1 : 0));
  free(owner), free(cover), free(runs), free(off);
  ++g_batches;
}

static uint64_t g_lcg = 54321;
static uint32_t rnd(void) {
  g_lcg = g_lcg * 6364136223846793005ull + 1442695040888963407ull;
  return (uint32_t)(g_lcg >> 33);
}

static int layout(void) {
  const uint64_t base = 0x7f0000000000ull, S = XL_DLV_CHUNK / 4u; /* samples of a chunk */
  const uint64_t edge[4] = {S - 1, S, S + 1, 3 * S + 5};
  static uint64_t src[1025], cnt[1025];
  CHECK(XL_DLV_CHUNK % 16 == 0 && XL_DLV_CHUNK / 16 == XL_DLV_THREADS * XL_DLV_SLOTS_PER_THREAD && S == 4096);
  check(0, src, cnt);
  /* n = 1 and n = 2: 0 .. 9 samples at every residue, every ordered pair; n = 3 behind a row of every short size */
  for (uint64_t s0 = 0; s0 <= 9; ++s0)
    for (uint64_t r0 = 0; r0 < 32; r0 += 8) {
      src[0] = base + 4096 + r0, cnt[0] = s0;
      check(1, src, cnt);
      for (uint64_t s1 = 0; s1 <= 9; ++s1)
        for (uint64_t r1 = 0; r1 < 32; r1 += 8) {
          src[1] = base + 65536 + r1, cnt[1] = s1;
          check(2, src, cnt);
          for (uint64_t r2 = 0; r2 < 32; r2 += 8) {
            src[2] = base + 131072 + r2, cnt[2] = 1 + (s0 + s1) % 9;
            check(3, src, cnt);
          }
        }
    }
  /* four one-sample rows sharing one slot */
  for (int i = 0; i < 4; ++i) src[i] = base + 32 * 100 * (uint64_t)i + 8 * (uint64_t)i, cnt[i] = 1;
  check(4, src, cnt);
  /* the chunk's edges: alone, behind and in front of a short row of every size, at every residue */
  for (int e = 0; e < 4; ++e)
    for (uint64_t r0 = 0; r0 < 32; r0 += 8) {
      src[0] = base + r0, cnt[0] = edge[e];
      check(1, src, cnt);
      for (uint64_t s1 = 0; s1 <= 9; ++s1)
        for (uint64_t r1 = 0; r1 < 32; r1 += 8) {
          src[0] = base + r0, cnt[0] = edge[e], src[1] = base + (1 << 20) + r1, cnt[1] = s1;
          check(2, src, cnt);
          src[0] = base + (1 << 20) + r1, cnt[0] = s1, src[1] = base + r0, cnt[1] = edge[e];
          check(2, src, cnt);
          src[2] = base + (2 << 20) + r1, cnt[2] = s1; /* short, edge, short */
          check(3, src, cnt);
        }
    }
  /* random batches: empty rows first, last and in runs; short rows sharing slots across a chunk's start; n = 1025 */
  for (int round = 0; round < 1200; ++round) {
    const size_t n = round % 8 == 0 ? 1025 : 1 + rnd() % (round % 2 ? 1025 : 40);
    const int mode = round % 5;
    for (size_t i = 0; i < n; ++i) {
      src[i] = base + (uint64_t)i * (1 << 18) + 8 * (rnd() % 4);
      const uint32_t x = rnd() % 100;
      if (mode == 0) cnt[i] = rnd() % 10;                                        /* 0 .. 9 */
      else if (mode == 1) cnt[i] = x < 30 ? 0 : 1 + rnd() % 4;                    /* tiny rows and runs of empty ones */
      else if (mode == 2) cnt[i] = x < 5 ? edge[rnd() % 4] : rnd() % 10;          /* an edge row now and then */
      else if (mode == 3) cnt[i] = 1 + rnd() % 1000;                              /* a few KB */
      else cnt[i] = x < 50 ? 0 : 1;                                               /* half empty, the rest one sample */
    }
    if (round % 3 == 0) cnt[0] = 0, cnt[n - 1] = 0;
    if (round % 3 == 1 && n > 40)
      for (size_t i = 10; i < 40; ++i) cnt[i] = 0;
    check(n, src, cnt);
  }
  for (size_t i = 0; i < 1025; ++i) cnt[i] = 0; /* all rows empty */
  check(1025, src, cnt);
  /* refusals: a source that is only 4-byte aligned, no source, a row above the maximum; the largest row is taken */
  {
    uint64_t off[1], tot;
    XlDlvRun run[1];
    size_t nr;
    src[0] = base + 8 * 5 + 4, cnt[0] = 8;
    CHECK(xl_dlv_plan_narrow(1, src, cnt, off, run, &nr, &tot) == -1);
    src[0] = 0;
    CHECK(xl_dlv_plan_narrow(1, src, cnt, off, run, &nr, &tot) == -1);
    src[0] = base, cnt[0] = XL_DLV_ROW_MAX / 4 + 1;
    CHECK(xl_dlv_plan_narrow(1, src, cnt, off, run, &nr, &tot) == -1);
    cnt[0] = ~(uint64_t)0 / 4 + 2; /* (4 * count would wrap) */
    CHECK(xl_dlv_plan_narrow(1, src, cnt, off, run, &nr, &tot) == -1);
    cnt[0] = XL_DLV_ROW_MAX / 4;
    CHECK(xl_dlv_plan_narrow(1, src, cnt, off, run, &nr, &tot) == 0 && nr == 1 && run[0].bytes == XL_DLV_ROW_MAX && tot == XL_DLV_ROW_MAX);
  }
  printf("ok %ld\n", g_batches);
  return 0;
}

int main(int argc, char **argv) {
  if (argc == 2 && strcmp(argv[1], "layout") == 0) return layout();
  if (argc == 4 && strcmp(argv[1], "rule") == 0) {
    const long e0 = strtol(argv[2], NULL, 10), e1 = strtol(argv[3], NULL, 10);
    if (e0 >= 0 && e0 <= e1 && e1 <= 255) return rule((uint32_t)e0, (uint32_t)e1);
  }
  fprintf(stderr, "usage: %s layout | rule E0 E1\n", argv[0]);
  return 2;
}
