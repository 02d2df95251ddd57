/* A stand-alone sweep over sdr-server_amd/csrc/xl_spectrum_bank_plan.h (with xl_spectrum_cut.h and xl_spectrum_wide_plan.h), built by
 * tests/test_spectrum_bank_wide_cpu.py with -fsanitize=address,undefined and run as a process of its own:
 *   - chunks: for transform counts 0 .. 70 and seeded large ones, and scratch sizes that hold 1, 2, 3, ... transforms (through
 *     xl_specw_chunk, sizes below one transform among them), the chunks mark every transform of the round exactly once in an array of
 *     exactly T entries (an index outside it is what ASan reports), in order, none empty, none longer than the scratch;
 *   - rounds: seeded banks of streams (width, rates with and without a skip, row slots 1 .. 3, staging sizes that hold 1, 2, 3 and many
 *     rows) consume seeded feeds round by round as xl_spectrum_bank.cpp's round does: every round consumes something, completes at most
 *     the staging's rows, touches at most `slots` rows per stream; the rows completed over the feed are those of the whole feed's cut,
 *     and the transforms are the stream's, each once and in order;
 *   - the staging's rows (at least one, never more bytes than given unless one) and the first capacity (1 .. 64).
 * Prints "ok <rounds>" or the first difference; exit status 0 or 1. */
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "xl_spectrum_bank_plan.h"
#include "xl_spectrum_wide_plan.h"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd(void) {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return rng_state;
}

static int fail(const char *what, uint64_t a, uint64_t b) {
  printf("FAIL %s: %" PRIu64 " %" PRIu64 "\n", what, a, b);
  return 1;
}

static int check_chunks(uint64_t T, uint64_t per) {
  uint8_t *seen = calloc(T ? T : 1, 1);
  if (seen == NULL) return fail("memory", T, per);
  const uint64_t chunks = xl_bankw_chunks(T, per);
  uint64_t next = 0;
  for (uint64_t i = 0; i < chunks; ++i) {
    const uint64_t base = i * per, len = xl_bankw_chunk_len(T, per, i);
    if (len == 0 || len > per) return fail("chunk length", T, per);
    if (base != next) return fail("chunk order", T, per);
    for (uint64_t t = 0; t < len; ++t)
      if (seen[base + t]++) return fail("transform twice", T, per);
    next = base + len;
  }
  if (next != T) return fail("transforms left out", T, per);
  for (uint64_t t = 0; t < T; ++t)
    if (seen[t] != 1) return fail("transform not once", T, per);
  free(seen);
  return 0;
}

#define MAX_STREAMS 6

static uint64_t rounds_total = 0;

static int check_bank(void) {
  static const int64_t WIDTHS[] = {8193, 9000, 16384, 20000, 48000, 1048576};
  const int64_t W = WIDTHS[rnd() % 6];
  const int64_t slots = 1 + (int64_t)(rnd() % 3);
  static const uint64_t HOLD[] = {1, 2, 3, 1000};
  const uint64_t hold = HOLD[rnd() % 4];
  /* a staging that holds `hold` rows, and one a byte short of a row: still one row */
  const uint64_t stage = rnd() % 8 == 0 ? 5ull * (uint64_t)W - 1u : hold * 5ull * (uint64_t)W + rnd() % 5u;
  const int64_t stage_rows = (int64_t)xl_bankw_stage_rows(stage, (uint32_t)W);
  if (stage_rows < 1 || (stage_rows > 1 && (uint64_t)stage_rows * 5ull * (uint64_t)W > stage) ||
      ((uint64_t)stage_rows + 1u) * 5ull * (uint64_t)W <= stage)
    return fail("staging rows", stage, (uint64_t)W);
  const int n = 1 + (int)(rnd() % MAX_STREAMS);
  int64_t sr[MAX_STREAMS], P[MAX_STREAMS], rows[MAX_STREAMS], next_g[MAX_STREAMS], carry[MAX_STREAMS];
  for (int i = 0; i < n; ++i) {
    const int64_t F = 1 + (int64_t)(rnd() % 4);
    sr[i] = F * W + (rnd() % 2 ? (int64_t)(rnd() % (uint64_t)W) : 0);
    P[i] = rows[i] = next_g[i] = carry[i] = 0;
  }
  for (int feed = 0; feed < 6; ++feed) {
    int64_t rem[MAX_STREAMS], P0[MAX_STREAMS];
    for (int i = 0; i < n; ++i) {
      static const int64_t PART[] = {0, 1, 2, 3, 7};
      const int64_t k = PART[rnd() % 5];
      rem[i] = k * sr[i] / 2 + (int64_t)(rnd() % (uint64_t)W) * (int64_t)(rnd() % 2);
      P0[i] = P[i];
    }
    for (;;) {
      int any = 0;
      for (int i = 0; i < n; ++i) any |= rem[i] > 0;
      if (!any) break;
      int64_t budget = stage_rows, consumed = 0, done_round = 0;
      for (int i = 0; i < n; ++i) {
        if (rem[i] == 0) continue;
        const int64_t lim = xl_bankw_round_limit(sr[i], W, P[i], slots, budget);
        if (budget > 0 && lim <= 0) return fail("no limit under a budget", (uint64_t)sr[i], (uint64_t)P[i]);
        if (budget <= 0 && lim != 0) return fail("a limit without a budget", (uint64_t)sr[i], (uint64_t)P[i]);
        if (lim == 0) continue;
        if (lim > xl_spec_round_limit(sr[i], P[i], slots)) return fail("beyond the row slots", (uint64_t)sr[i], (uint64_t)P[i]);
        const int64_t c = rem[i] < lim ? rem[i] : lim;
        const XlSpecCut cut = xl_spec_cut(sr[i], W, P[i], c);
        if (xl_bankw_rows_before(sr[i], W, P[i]) != rows[i]) return fail("rows before", (uint64_t)sr[i], (uint64_t)P[i]);
        const int64_t done = cut.rows_done - rows[i];
        if (done < 0 || done > budget || done > slots) return fail("rows of a stream's round", (uint64_t)done, (uint64_t)budget);
        /* the transforms, each once and in order; the carry continued */
        if (cut.carry_app > 0) {
          if (cut.carry_have != carry[i]) return fail("carry", (uint64_t)sr[i], (uint64_t)P[i]);
          carry[i] += cut.carry_app;
          if (cut.carry_done) {
            if (carry[i] != W || cut.carry_g != next_g[i]) return fail("carry transform", (uint64_t)sr[i], (uint64_t)P[i]);
            next_g[i]++, carry[i] = 0;
          }
        }
        if (cut.T > 0) {
          if (cut.g_first != next_g[i]) return fail("transform order", (uint64_t)sr[i], (uint64_t)P[i]);
          next_g[i] += cut.T;
        }
        if (cut.save_n > 0) carry[i] = cut.save_n;
        budget -= done, done_round += done, consumed += c;
        rows[i] = cut.rows_done, P[i] += c, rem[i] -= c;
      }
      if (consumed <= 0) return fail("empty round", (uint64_t)W, (uint64_t)stage_rows);
      if (done_round > stage_rows) return fail("round beyond the staging", (uint64_t)done_round, (uint64_t)stage_rows);
      ++rounds_total;
    }
    for (int i = 0; i < n; ++i) { /* the whole feed in one cut */
      if (P[i] == P0[i]) continue;
      const XlSpecCut whole = xl_spec_cut(sr[i], W, P0[i], P[i] - P0[i]);
      if (whole.rows_done != rows[i]) return fail("rows of the feed", (uint64_t)sr[i], (uint64_t)P[i]);
    }
  }
  for (int i = 0; i < n; ++i) { /* every transform that lies wholly below P has been run */
    const int64_t F = sr[i] / W, row = P[i] / sr[i], pos = P[i] % sr[i];
    const int64_t total = row * F + (pos / W < F ? pos / W : F);
    if (next_g[i] != total) return fail("transform count", (uint64_t)next_g[i], (uint64_t)total);
  }
  return 0;
}

int main(void) {
  /* chunks: scratch sizes that hold 1, 2, 3, ... transforms of every length, through xl_specw_chunk */
  for (uint32_t e = 14; e <= 21; ++e) {
    const uint32_t N = 1u << e;
    for (uint64_t hold = 0; hold <= 12; ++hold) {
      const uint64_t per = xl_specw_chunk(hold * 8ull * N + (hold ? rnd() % (8ull * N) : 0), N);
      if (per != (hold ? hold : 1)) return fail("transforms per chunk", hold, per);
      for (uint64_t T = 0; T <= 70; ++T)
        if (check_chunks(T, per)) return 1;
    }
    if (check_chunks(21, 5) || check_chunks(21, 3) || check_chunks(21, 1) || check_chunks(21, 7) || check_chunks(21, 21) || check_chunks(21, 22))
      return 1;
  }
  for (int i = 0; i < 200; ++i)
    if (check_chunks(1 + rnd() % 100000, 1 + rnd() % 300)) return 1;
  for (int i = 0; i < 4000; ++i)
    if (check_bank()) return 1;
  for (uint64_t b = 0; b < 40; ++b) {
    const uint64_t bytes = b < 2 ? b : ((uint64_t)1 << b) - (b & 1u);
    const uint32_t f = xl_bankw_first_streams(bytes);
    if (f < 1 || f > 64 || (bytes > 0 && f > 1 && (uint64_t)f * bytes > XL_BANKW_FIRST_BYTES)) return fail("first capacity", bytes, f);
  }
  printf("ok %" PRIu64 "\n", rounds_total);
  return 0;
}
