/* A stand-alone sweep over sdr-server_amd/csrc/xl_resample_cut.h, built by tests/test_resample_cpu.py with
 * -fsanitize=address,undefined and run as a process of its own: for every (L, M) of the list and random feed sequences (counts of 0, 1,
 * Q - 2 .. Q among them, starting points up to 2^40), each cut against a brute-force walk over the outputs' positions n_m = m M / L,
 * p_m = m M % L, the carry bookkeeping, and the sum of the output counts against ceil(N L / M).  Prints "ok <cuts>" or the first
 * difference; exit status 0 or 1. */
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>

#include "xl_resample_cut.h"

static uint64_t rng_state = 88172645463325252ull;
static uint64_t rnd(void) {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return rng_state;
}

static int fail(const char *what, uint32_t L, uint32_t M, uint32_t Q, uint64_t P, uint64_t n) {
  printf("FAIL %s: L %u M %u Q %u P0 %" PRIu64 " n %" PRIu64 "\n", what, L, M, Q, P, n);
  return 1;
}

int main(void) {
  static const uint32_t LM[][2] = {{1, 1}, {1, 3}, {3, 1}, {2, 3}, {7, 8}, {624, 625}, {4096, 4095}, {3, 5}, {441, 500}, {1, 2147483647}};
  static const uint32_t QS[] = {1, 2, 3, 14, 21, 1024};
  uint64_t cuts = 0;
  for (size_t r = 0; r < sizeof LM / sizeof LM[0]; ++r) {
    const uint32_t L = LM[r][0], M = LM[r][1];
    for (size_t qi = 0; qi < sizeof QS / sizeof QS[0]; ++qi) {
      const uint32_t Q = QS[qi];
      for (int start = 0; start < 4; ++start) {
        const uint64_t P_start = start == 0 ? 0 : (start == 1 ? rnd() % 1000 : (start == 2 ? ((uint64_t)1 << 40) - rnd() % 5000 : rnd() % ((uint64_t)1 << 40)));
        uint64_t P = P_start, total = 0;
        /* the brute-force walk: the first output not produced by P_start samples */
        uint64_t m = xl_resample_produced(L, M, P_start);
        if (m > 0 && (m - 1) * M / L >= P_start) return fail("produced too many", L, M, Q, P, 0);
        if (m * M / L < P_start) return fail("produced too few", L, M, Q, P, 0);
        for (int f = 0; f < 40; ++f) {
          uint64_t n;
          switch (rnd() % 8) {
            case 0: n = 0; break;
            case 1: n = 1; break;
            case 2: n = Q >= 2 ? Q - 2 : 0; break;
            case 3: n = Q - 1; break;
            case 4: n = Q; break;
            case 5: n = rnd() % 5000; break;
            case 6: n = rnd() % (3 * (uint64_t)M / L + 2); break;
            default: n = rnd() % 300; break;
          }
          const XlResampleCut c = xl_resample_cut(L, M, Q, P, n);
          cuts++;
          if (c.m_first != m) return fail("m_first", L, M, Q, P, n);
          uint64_t k = 0;
          while ((m + k) * M / L < P + n && k < 200000) k++;  /* outputs whose n_m has been consumed */
          if (c.count != k) return fail("count", L, M, Q, P, n);
          if (k > 0 || n > 0) {
            if ((uint64_t)c.n_first + P != m * M / L || c.p_first != m * M % L) return fail("first position", L, M, Q, P, n);
            if (c.n_first < 0) return fail("n_first < 0", L, M, Q, P, n);
          }
          if (k > 0 && (uint64_t)c.n_first >= n) return fail("n_first >= n", L, M, Q, P, n);
          if (c.carry_new + c.carry_old != Q - 1 || c.carry_new != (n < Q - 1 ? n : Q - 1)) return fail("carry", L, M, Q, P, n);
          m += k, P += n, total += k;
        }
        if (total != xl_resample_produced(L, M, P) - xl_resample_produced(L, M, P_start)) return fail("sum", L, M, Q, P, 0);
        if (P_start == 0 && total != (P * L + M - 1) / M) return fail("ceil", L, M, Q, P, 0);
      }
    }
  }
  printf("ok %" PRIu64 "\n", cuts);
  return 0;
}
