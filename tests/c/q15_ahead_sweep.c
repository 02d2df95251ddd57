/* A stand-alone sweep over sdr-server_amd/csrc/xl_q15_ahead.h (engine option "q15_nco"), built by tests/test_q15_nco_cpu.py with gcc
 * alone under ASan and UBSan and run as a process of its own.  Stream positions up to the 2^31 edge, block lengths, block counts,
 * immature counts, client counts, pending or not:
 *   - a pending record serves a call if and only if trel, S and G all match (the flags word of the position is not the Q15 family's);
 *     nothing serves without a pending record;
 *   - "launch allowed" is false exactly when the plan holds immature clients, the engine has no clients, or the position would reach
 *     2^31 within two more calls of this size -- stated here in 64-bit arithmetic of its own;
 *   - whenever a launch is allowed, the predicted position xl_grid_next(pos) is the exact sum: no 32-bit product or sum wrapped, the
 *     next call at it does not re-base (xl_call_begin's test), and a call there is served by the record.
 * Prints "ok <checks>" or the first failure; exit status 0 or 1. */
#include <stdint.h>
#include <stdio.h>

#include "xl_q15_ahead.h"

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

int main(void) {
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
  printf("ok %lu\n", n);
  return 0;
}
