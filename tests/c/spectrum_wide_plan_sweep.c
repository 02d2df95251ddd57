/* A stand-alone sweep over sdr-server_amd/csrc/xl_spectrum_wide_plan.h, built by tests/test_spectrogram_wide_cpu.py with
 * -fsanitize=address,undefined and run as a process of its own: for every width at and around each power of two of 8193 .. 1048576 and
 * random widths between, the transform length (a power of two; W itself, or >= 2 W - 1 and the smallest such), the split (N1 N2 = N,
 * N2 <= 8192, a pack run of at least 16 that divides N2), the chunk count for scratch sizes from 0 to 2^40, the refusal of widths
 * outside the range; and for the plain widths the bin order: positions marked in an array of exactly N entries (an index outside it is
 * what ASan reports), each hit once, and the finishing pass's column order against the half swap done by hand.
 * Prints "ok <widths>" or the first difference; exit status 0 or 1. */
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "xl_spectrum_wide_plan.h"

static uint64_t rng_state = 88172645463325252ull;
static uint64_t rnd(void) {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return rng_state;
}

static int fail(const char *what, uint32_t W) {
  printf("FAIL %s: W %u\n", what, W);
  return 1;
}

static int check_width(uint32_t W) {
  XlSpecWidePlan p;
  memset(&p, 0xEE, sizeof p);
  if (xl_specw_plan(W, &p) != 0) return fail("refused", W);
  const int pow2 = (W & (W - 1u)) == 0u;
  if (p.W != W || (p.N & (p.N - 1u)) != 0u) return fail("length is no power of two", W);
  if (pow2 ? (p.N != W || p.blue != 0) : (p.blue != 1 || (uint64_t)p.N < 2ull * W - 1ull || (uint64_t)(p.N / 2u) >= 2ull * W - 1ull))
    return fail("length", W);
  if (p.N < (1u << 14) || p.N > (1u << 21)) return fail("length outside 2^14 .. 2^21", W);
  if ((uint64_t)p.N1 * p.N2 != p.N || p.N2 > 8192u || p.N2 != XL_SPECW_N2(p.N)) return fail("split", W);
  if (p.N1 != 64u && p.N1 != 128u && p.N1 != 256u) return fail("N1", W);
  if (p.pack < 16u || p.pack * p.N1 != XL_SPECW_PACK_POINTS || p.N2 % p.pack != 0u) return fail("pack", W);
  if (p.N1 % 16u != 0u) return fail("a pack of rows leaves its transform", W);
  static const uint64_t SCR[] = {0, 1, 8, 131071, 131072, 131073, (uint64_t)64 << 20, ((uint64_t)64 << 20) - 1, (uint64_t)1 << 40};
  for (size_t i = 0; i < sizeof SCR / sizeof SCR[0]; ++i) {
    const uint64_t c = xl_specw_chunk(SCR[i], p.N);
    if (c < 1 || (c > 1 && c * 8ull * p.N > SCR[i]) || (c + 1) * 8ull * p.N <= SCR[i]) return fail("chunk", W);
  }
  return 0;
}

static int check_order(uint32_t W) { /* a plain width */
  XlSpecWidePlan p;
  if (xl_specw_plan(W, &p) != 0 || p.blue) return fail("plain plan", W);
  uint8_t *seen = calloc(p.N, 1);
  uint32_t *col = malloc(sizeof(uint32_t) * W);
  if (seen == NULL || col == NULL) return fail("memory", W);
  for (uint32_t k = 0; k < W; ++k) {
    const uint32_t pos = xl_specw_bin_pos(p.N1, p.N2, k);
    if (pos / p.N2 != k % p.N1 || pos % p.N2 != k / p.N1) return fail("bin position", W);
    if (seen[pos]++) return fail("bin position twice", W);
  }
  /* the half swap by hand: bins half .. 2 half - 1 first, then 0 .. half - 1 */
  const uint32_t half = W / 2u;
  for (uint32_t j = 0; j < half; ++j) col[j] = half + j, col[half + j] = j;
  for (uint32_t j = 0; j < W; ++j) {
    if (xl_specw_shift_src(j, W) != col[j]) return fail("half swap", W);
    const uint32_t pos = xl_specw_col_pos(p.N1, p.N2, W, j);
    if (pos != xl_specw_bin_pos(p.N1, p.N2, col[j])) return fail("column position", W);
    if (seen[pos] != 1) return fail("column position not a bin's", W);
    seen[pos] = 2;
  }
  for (uint32_t i = 0; i < p.N; ++i)
    if (seen[i] != 2) return fail("a position is never read", W);
  free(seen);
  free(col);
  return 0;
}

int main(void) {
  uint64_t widths = 0;
  XlSpecWidePlan p;
  static const uint32_t OUT[] = {0, 1, 64, 8191, 8192, 1048577, 2097152, 0x7FFFFFFFu, 0xFFFFFFFFu};
  for (size_t i = 0; i < sizeof OUT / sizeof OUT[0]; ++i)
    if (xl_specw_plan(OUT[i], &p) != -1) return fail("accepted", OUT[i]);
  for (uint32_t e = 13; e <= 20; ++e) {
    const uint32_t c = 1u << e;
    for (int32_t d = -3; d <= 3; ++d) {
      const uint32_t W = (uint32_t)((int32_t)c + d);
      if (W < XL_SPECW_MIN_W || W > XL_SPECW_MAX_W) continue;
      if (check_width(W)) return 1;
      ++widths;
    }
    /* W with 2 W - 1 at and around a power of two: where the Bluestein length steps */
    for (int32_t d = -2; d <= 2; ++d) {
      const uint32_t W = (uint32_t)((int32_t)(c / 2u + c) + d), V = (uint32_t)((int32_t)(c + 1u) / 2 + (int32_t)c / 2 + d);
      if (W >= XL_SPECW_MIN_W && W <= XL_SPECW_MAX_W && check_width(W)) return 1;
      if (V >= XL_SPECW_MIN_W && V <= XL_SPECW_MAX_W && check_width(V)) return 1;
      widths += 2;
    }
  }
  for (int i = 0; i < 20000; ++i) {
    const uint32_t W = XL_SPECW_MIN_W + (uint32_t)(rnd() % (XL_SPECW_MAX_W - XL_SPECW_MIN_W + 1u));
    if (check_width(W)) return 1;
    ++widths;
  }
  for (uint32_t e = 14; e <= 20; ++e)
    if (check_order(1u << e)) return 1;
  for (uint32_t W = 1; W < 70; ++W) { /* the half swap alone, odd widths among them */
    uint32_t hits = 0;
    for (uint32_t j = 0; j < W; ++j) {
      const uint32_t s = xl_specw_shift_src(j, W);
      if (s >= W) return fail("half swap leaves the row", W);
      hits += s == ((W & 1u) && j == W - 1u ? j : (j + W / 2u) % (2u * (W / 2u)));
    }
    if (hits != W) return fail("half swap of a small width", W);
  }
  printf("ok %" PRIu64 "\n", widths);
  return 0;
}
