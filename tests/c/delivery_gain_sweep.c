/* tests/c/delivery_gain_sweep.c -- the headers of the delivery's gain and level meter held to their contracts by a program of its own,
 * compiled by tests/test_delivery_gain_cpu.py with gcc (with -fsanitize=address,undefined for the plan, the policy and part of the rule).
 *
 *   delivery_gain_sweep zero E0 E1
 *     csrc/xl_dlv_gain.h at g = 0 against csrc/xl_dlv_narrow.h, an integer compare, on EVERY bit pattern whose exponent field lies in
 *     E0 .. E1 (both signs, all 2^23 fractions).  Prints "ok <patterns>".
 *   delivery_gain_sweep rule G E0 E1
 *     xl_dlv_gain_narrow(bits, G) and its clamp flag against the libm statement -- NaN -> 0 and no clamp, otherwise
 *     r = nearbyint(ldexp((double)y, 15 + G)) (exact product, one rounding to nearest even), clamped to -32768 .. 32767, the flag set
 *     where r lay outside -- on every bit pattern of the fields E0 .. E1; also xl_dlv_gain_nan and xl_dlv_gain_mag.
 *   delivery_gain_sweep edges
 *     the same compare for EVERY g in -48 .. 48 on all 256 exponent fields x both signs x the fractions 0, 1, half - 1, half, half + 1
 *     and 0x7FFFFF, half being that of the shift in force (k = 135 - (e + g) where that is 8 .. 24, else 16), each of the three around
 *     the half also with the quotient's lowest bit set (the tie that rounds up), and the all-ones fraction with its low 8 bits clear.
 *   delivery_gain_sweep plan
 *     csrc/xl_delivery_plan.h's xl_dlv_plan_gain against brute force: the offsets and the image are xl_dlv_plan_narrow's for the same
 *     rows; run k is the k-th non-empty row with its XlDlvRun, its gain and level index k; lvl[i] names it (XL_DLV_NO_LEVEL for an empty
 *     row); the level table begins at the image's end rounded up to 16 and holds 12 bytes a run; xl_dlv_gain_first equals xl_dlv_first
 *     on the plain records for every chunk and every `found`; refusals (a gain of 49, of -49, of an empty row; the narrowed plan's).
 *   delivery_gain_sweep policy
 *     csrc/xl_serve_gain.h driven with sequences of (peak, clipped), the clipped count taken from the rule itself at the gain a call
 *     was packed with, a call being answered one call later (overlap = 0) and two calls later (overlap = 1).
 * Every mode prints "ok <count>". */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "xl_delivery_plan.h"
#include "xl_dlv_gain.h"
#include "xl_dlv_narrow.h"
#include "xl_serve_gain.h"

static long g_count = 0;

#define CHECK(c)                                                            \
  do {                                                                      \
    if (!(c)) {                                                             \
      fprintf(stderr, "line %d: %s (count %ld)\n", __LINE__, #c, g_count);  \
      exit(1);                                                              \
    }                                                                       \
  } while (0)

/* ------------------------------------------------------------------------------------------------------------------ the rule */
static int32_t want(uint32_t bits, int g, uint32_t *clamped) {
  float y;
  memcpy(&y, &bits, 4);
  *clamped = 0;
  if (y != y) return 0;
  const double r = nearbyint(ldexp((double)y, 15 + g));
  *clamped = (r > 32767.0 || r < -32768.0) ? 1u : 0u;
  return r > 32767.0 ? 32767 : (r < -32768.0 ? -32768 : (int32_t)r);
}

static int one(uint32_t bits, int g) {
  uint32_t cg, cw;
  const int32_t got = xl_dlv_gain_narrow(bits, g, &cg), exp = want(bits, g, &cw);
  float y;
  memcpy(&y, &bits, 4);
  const uint32_t nan = y != y ? 1u : 0u;
  if (got != exp || cg != cw || xl_dlv_gain_nan(bits) != nan || xl_dlv_gain_mag(bits) != (nan ? 0u : bits & 0x7FFFFFFFu)) {
    fprintf(stderr, "bits 0x%08x gain %d: got %d clamped %u, expected %d clamped %u\n", (unsigned)bits, g, (int)got, (unsigned)cg,
            (int)exp, (unsigned)cw);
    return 1;
  }
  return 0;
}

static int rule(int g, uint32_t e0, uint32_t e1) {
  unsigned long long n = 0;
  for (uint32_t e = e0; e <= e1; ++e)
    for (uint32_t sign = 0; sign < 2u; ++sign)
      for (uint32_t frac = 0; frac < (1u << 23); ++frac, ++n)
        if (one((sign << 31) | (e << 23) | frac, g)) return 1;
  printf("ok %llu\n", n);
  return 0;
}

static int zero(uint32_t e0, uint32_t e1) {
  unsigned long long n = 0;
  for (uint32_t e = e0; e <= e1; ++e)
    for (uint32_t sign = 0; sign < 2u; ++sign)
      for (uint32_t frac = 0; frac < (1u << 23); ++frac, ++n) {
        const uint32_t bits = (sign << 31) | (e << 23) | frac;
        uint32_t c;
        if (xl_dlv_gain_narrow(bits, 0, &c) != xl_dlv_narrow(bits)) {
          fprintf(stderr, "bits 0x%08x: %d at gain 0, xl_dlv_narrow %d\n", (unsigned)bits, (int)xl_dlv_gain_narrow(bits, 0, &c),
                  (int)xl_dlv_narrow(bits));
          return 1;
        }
      }
  printf("ok %llu\n", n);
  return 0;
}

static int edges(void) {
  unsigned long long n = 0;
  for (int g = XL_DLV_GAIN_MIN; g <= XL_DLV_GAIN_MAX; ++g)
    for (uint32_t e = 0; e < 256u; ++e) {
      const int kk = 135 - ((int)e + g);
      const uint32_t k = kk >= 8 && kk <= 24 ? (uint32_t)kk : 16u, h = 1u << (k - 1u), odd = 1u << k;
      const uint32_t fr[11] = {0u, 1u, h - 1u, h, h + 1u, odd | (h - 1u), odd | h, odd | (h + 1u), 0x7FFFFFu, 0x7FFF00u, 0x7FFEFFu};
      for (uint32_t sign = 0; sign < 2u; ++sign)
        for (int i = 0; i < 11; ++i, ++n)
          if (one((sign << 31) | (e << 23) | (fr[i] & 0x7FFFFFu), g)) return 1;
    }
  printf("ok %llu\n", n);
  return 0;
}

/* ------------------------------------------------------------------------------------------------------------------ the plan */
static uint64_t g_lcg = 97531;
static uint32_t rnd(void) {
  g_lcg = g_lcg * 6364136223846793005ull + 1442695040888963407ull;
  return (uint32_t)(g_lcg >> 33);
}

static void check_plan(size_t n, const uint64_t *src, const uint64_t *cnt, const int8_t *gain) {
  uint64_t *off = malloc((n + 1) * sizeof(*off)), *off0 = malloc((n + 1) * sizeof(*off0));
  uint32_t *lvl = malloc((n + 1) * sizeof(*lvl));
  XlDlvRun *scratch = malloc((n + 1) * sizeof(*scratch)), *plain = malloc((n + 1) * sizeof(*plain));
  XlDlvGainRun *runs = malloc((n + 1) * sizeof(*runs));
  size_t nruns = 0, nplain = 0;
  uint64_t total = 0, total0 = 0, lvl_off = 1, full = 1;
  CHECK(off && off0 && lvl && scratch && plain && runs);
  CHECK(xl_dlv_plan_narrow(n, src, cnt, off0, plain, &nplain, &total0) == 0);
  CHECK(xl_dlv_plan_gain(n, src, cnt, gain, off, lvl, scratch, runs, &nruns, &total, &lvl_off, &full) == 0);
  CHECK(nruns == nplain && total == total0);
  size_t k = 0;
  for (size_t i = 0; i < n; ++i) {
    CHECK(off[i] == off0[i]);
    if (cnt[i] == 0) {
      CHECK(lvl[i] == XL_DLV_NO_LEVEL);
      continue;
    }
    CHECK(k < nruns && lvl[i] == k && runs[k].lvl == k && runs[k].gain == gain[i]);
    CHECK(runs[k].r.src == src[i] && runs[k].r.off == off[i] && runs[k].r.bytes == 4 * cnt[i] && runs[k].r.s16 == off[i] / 16);
    CHECK(memcmp(&runs[k].r, &plain[k], sizeof(XlDlvRun)) == 0);
    ++k;
  }
  CHECK(k == nruns);
  if (nruns == 0) CHECK(lvl_off == 0 && full == 0);
  else CHECK(lvl_off % 16 == 0 && lvl_off >= total && lvl_off < total + 16 && full == lvl_off + 12 * nruns);
  const uint32_t chunks = xl_dlv_chunks(total);
  for (uint32_t c = 0; c < chunks; ++c)
    for (uint32_t found = 0; found < nruns; found += 1u + (nruns > 64 ? rnd() % 7u : 0u))
      CHECK(xl_dlv_gain_first(runs, found, c) == xl_dlv_first(plain, found, c));
  free(runs), free(plain), free(scratch), free(lvl), free(off0), free(off);
  ++g_count;
}

static int plan(void) {
  const uint64_t base = 0x7f0000000000ull, S = XL_DLV_CHUNK / 4u;
  const uint64_t edge[4] = {S - 1, S, S + 1, 2 * S + 1};
  static uint64_t src[1025], cnt[1025];
  static int8_t gain[1025];
  CHECK(XL_DLV_GAIN_LO == XL_DLV_GAIN_MIN && XL_DLV_GAIN_HI == XL_DLV_GAIN_MAX && XL_SERVE_GAIN_MIN == XL_DLV_GAIN_MIN &&
        XL_SERVE_GAIN_MAX == XL_DLV_GAIN_MAX);
  CHECK(sizeof(XlDlvGainRun) == 32 && XL_DLV_LEVEL_WORDS == 3u);
  check_plan(0, src, cnt, gain);
  for (uint64_t s0 = 0; s0 <= 9; ++s0)
    for (uint64_t r0 = 0; r0 < 32; r0 += 8)
      for (uint64_t s1 = 0; s1 <= 9; ++s1)
        for (uint64_t r1 = 0; r1 < 32; r1 += 8) {
          src[0] = base + 4096 + r0, cnt[0] = s0, gain[0] = (int8_t)(-48 + (int)(s0 + r1));
          src[1] = base + 65536 + r1, cnt[1] = s1, gain[1] = (int8_t)(48 - (int)(s1 + r0));
          check_plan(1, src, cnt, gain);
          check_plan(2, src, cnt, gain);
        }
  for (int e = 0; e < 4; ++e)
    for (uint64_t r0 = 0; r0 < 32; r0 += 8)
      for (uint64_t s1 = 0; s1 <= 9; ++s1) {
        src[0] = base + (1 << 20) + 8 * (s1 % 4), cnt[0] = s1, gain[0] = 48;
        src[1] = base + r0, cnt[1] = edge[e], gain[1] = -48;
        src[2] = base + (2 << 20) + r0, cnt[2] = s1, gain[2] = 0;
        check_plan(3, src, cnt, gain);
      }
  for (int round = 0; round < 600; ++round) {
    const size_t n = round % 8 == 0 ? 1025 : 1 + rnd() % (round % 2 ? 1025 : 40);
    const int mode = round % 5;
    for (size_t i = 0; i < n; ++i) {
      src[i] = base + (uint64_t)i * (1 << 18) + 8 * (rnd() % 4);
      gain[i] = (int8_t)((int)(rnd() % 97u) - 48);
      const uint32_t x = rnd() % 100;
      if (mode == 0) cnt[i] = rnd() % 10;
      else if (mode == 1) cnt[i] = x < 30 ? 0 : 1 + rnd() % 4;
      else if (mode == 2) cnt[i] = x < 5 ? edge[rnd() % 4] : rnd() % 10;
      else if (mode == 3) cnt[i] = 1 + rnd() % 1000;
      else cnt[i] = x < 50 ? 0 : 1;
    }
    if (round % 3 == 0) cnt[0] = 0, cnt[n - 1] = 0;
    check_plan(n, src, cnt, gain);
  }
  for (size_t i = 0; i < 1025; ++i) cnt[i] = 0;
  check_plan(1025, src, cnt, gain);
  { /* refusals */
    uint64_t off[2], tot, lo, fu;
    uint32_t lvl[2];
    XlDlvRun sc[2];
    XlDlvGainRun run[2];
    size_t nr;
    src[0] = base, cnt[0] = 8, src[1] = base + 4096, cnt[1] = 0;
    const int bad[4] = {49, -49, 127, -128};
    for (int b = 0; b < 4; ++b) {
      gain[0] = (int8_t)bad[b], gain[1] = 0;
      CHECK(xl_dlv_plan_gain(2, src, cnt, gain, off, lvl, sc, run, &nr, &tot, &lo, &fu) == -1);
      gain[0] = 0, gain[1] = (int8_t)bad[b]; /* (an empty row's gain is checked too) */
      CHECK(xl_dlv_plan_gain(2, src, cnt, gain, off, lvl, sc, run, &nr, &tot, &lo, &fu) == -1);
    }
    gain[0] = 48, gain[1] = -48;
    CHECK(xl_dlv_plan_gain(2, src, cnt, gain, off, lvl, sc, run, &nr, &tot, &lo, &fu) == 0 && nr == 1 && tot == 32 && lo == 32 && fu == 44);
    src[0] = base + 4;
    CHECK(xl_dlv_plan_gain(2, src, cnt, gain, off, lvl, sc, run, &nr, &tot, &lo, &fu) == -1);
    src[0] = 0;
    CHECK(xl_dlv_plan_gain(2, src, cnt, gain, off, lvl, sc, run, &nr, &tot, &lo, &fu) == -1);
    src[0] = base, cnt[0] = XL_DLV_ROW_MAX / 4 + 1;
    CHECK(xl_dlv_plan_gain(2, src, cnt, gain, off, lvl, sc, run, &nr, &tot, &lo, &fu) == -1);
  }
  printf("ok %ld\n", g_count);
  return 0;
}

/* ---------------------------------------------------------------------------------------------------------------- the policy */
static uint32_t clips(uint32_t peak_bits, int g) { /* a row whose largest float is +peak: does it clip under g? */
  uint32_t c = 0;
  if (peak_bits != 0u) (void)xl_dlv_gain_narrow(peak_bits, g, &c);
  return c;
}

/* a constant level from gain g0 on, every call answered `lag` calls later; checks the properties, returns the final gain */
static int constant(uint32_t peak, int g0, int lag) {
  XlServeGainState st = {0};
  int g = g0, hist[1000], calls_since_clip = -1, steps_after_clip = 0;
  const uint32_t e = peak >> 23, frac = peak & 0x7FFFFFu;
  const int rounds_up = e != 0u && e != 255u && frac >= 0x7FFF00u; /* 16-bit rounding reaches the next power of two */
  for (int call = 0; call < 1000; ++call) {
    hist[call] = g; /* the gain this call is packed with */
    if (call + 1 < lag) continue;
    const int gp = hist[call + 1 - lag];
    const uint32_t c = clips(peak, gp);
    const int before = g;
    g = xl_serve_gain_step(&st, peak, c, gp, g);
    CHECK(g >= XL_SERVE_GAIN_MIN && g <= XL_SERVE_GAIN_MAX);
    CHECK(g <= before + 1);
    if (lag == 1) {
      /* one call after a clipped call nothing clips -- unless the gain stands at its lower end, or the level is one whose 16-bit
         rounding reaches 32768 at top = 0 (the fraction's top 15 bits set): that one takes one more step of 1, and no third */
      if (calls_since_clip == 0 && c > 0u) {
        CHECK(gp == XL_SERVE_GAIN_MIN || (rounds_up && steps_after_clip == 0 && before - g == 1) || e == 255u);
        ++steps_after_clip;
      }
      if (c > 0u) calls_since_clip = 0;
      else calls_since_clip = -1, steps_after_clip = 0;
    }
    ++g_count;
  }
  for (int call = 900; call < 1000; ++call) CHECK(hist[call] == g); /* a fixed gain, no oscillation */
  if (peak != 0u && g > XL_SERVE_GAIN_MIN && g < XL_SERVE_GAIN_MAX) {
    const int top = xl_serve_gain_top(peak, g);
    CHECK(top <= 0 && top > XL_SERVE_GAIN_LOW_TOP && clips(peak, g) == 0u); /* |peak| * 2^g in [1/8, 1) */
    /* xl_serve_gain_top against libm */
    float y;
    memcpy(&y, &peak, 4);
    int ex;
    (void)frexp(ldexp((double)y, g), &ex); /* in [2^(ex - 1), 2^ex) */
    CHECK(ex == top);
  }
  if (peak == 0u) CHECK(g == g0); /* silence holds the gain */
  return g;
}

static int policy(void) {
  const uint32_t fr[8] = {0u, 1u, 0x3FFFFFu, 0x400000u, 0x7FFEFFu, 0x7FFF00u, 0x7FFF80u, 0x7FFFFFu};
  const int start[6] = {-48, -20, 0, 1, 13, 48};
  for (int lag = 1; lag <= 2; ++lag)
    for (int s = 0; s < 6; ++s) {
      for (uint32_t e = 1; e < 255u; ++e)
        for (int f = 0; f < 8; ++f) (void)constant((e << 23) | fr[f], start[s], lag);
      for (uint32_t d = 1; d < (1u << 23); d = d * 2u + (d % 3u == 0u)) (void)constant(d, start[s], lag); /* denormals */
      (void)constant(0x007FFFFFu, start[s], lag);
      (void)constant(0x7F800000u, start[s], lag); /* an Inf in every call: down to the lower end */
      CHECK(constant(0u, start[s], lag) == start[s]);
    }
  { /* silence neither moves the gain nor restarts the count; a call above the low mark restarts it */
    XlServeGainState st = {0};
    const uint32_t low = (uint32_t)(127 - 6) << 23, mid = (uint32_t)(127 - 2) << 23; /* 2^-6: top = -5; 2^-2: top = -1 */
    int g = 0;
    for (int i = 0; i < XL_SERVE_GAIN_QUIET_CALLS - 1; ++i) CHECK((g = xl_serve_gain_step(&st, low, 0, g, g)) == 0);
    for (int i = 0; i < 20; ++i) CHECK((g = xl_serve_gain_step(&st, 0u, 0, g, g)) == 0);
    CHECK((g = xl_serve_gain_step(&st, low, 0, g, g)) == 1);
    for (int i = 0; i < XL_SERVE_GAIN_QUIET_CALLS - 1; ++i) CHECK((g = xl_serve_gain_step(&st, low, 0, g, g)) == 1);
    CHECK((g = xl_serve_gain_step(&st, mid, 0, g, g)) == 1);
    for (int i = 0; i < XL_SERVE_GAIN_QUIET_CALLS - 1; ++i) CHECK((g = xl_serve_gain_step(&st, low, 0, g, g)) == 1);
    CHECK((g = xl_serve_gain_step(&st, low, 0, g, g)) == 2);
    /* a step of 2^6 up from a settled level: one decision takes the whole step */
    CHECK(xl_serve_gain_step(&st, (uint32_t)(127 + 5) << 23, 7, 2, 2) == 2 - (5 + 1 + 2));
  }
  { /* random sequences: the gain never leaves its range, never rises by more than 1, and rises only on a full count */
    XlServeGainState st = {0};
    int g = 0, low_run = 0;
    for (int i = 0; i < 2000000; ++i, ++g_count) {
      const uint32_t kind = rnd() % 8u;
      const uint32_t peak = kind == 0u ? 0u : (kind == 1u ? 0x7F800000u : ((rnd() % 255u) << 23) | (rnd() & 0x7FFFFFu));
      const uint32_t c = kind == 2u ? rnd() % 5u : clips(peak, g);
      const int before = g;
      g = xl_serve_gain_step(&st, peak, c, g, g);
      CHECK(g >= XL_SERVE_GAIN_MIN && g <= XL_SERVE_GAIN_MAX && g <= before + 1);
      if (peak != 0u && c == 0u && xl_serve_gain_top(peak, before) <= XL_SERVE_GAIN_LOW_TOP) ++low_run;
      else if (peak != 0u || c != 0u) low_run = 0;
      if (g == before + 1) CHECK(low_run == XL_SERVE_GAIN_QUIET_CALLS);
      if (low_run == XL_SERVE_GAIN_QUIET_CALLS) low_run = 0;
    }
  }
  { /* the log: the latest 64 changes, oldest first; two changes at one sample leave the later */
    XlServeGainLog l;
    uint64_t f[80];
    int8_t gg[80];
    memset(&l, 0, sizeof(l));
    CHECK(xl_serve_gain_log_read(&l, 80, f, gg) == 0);
    for (int i = 0; i < 100; ++i) xl_serve_gain_log_add(&l, 10u * (uint64_t)i, i % 40 - 20);
    xl_serve_gain_log_add(&l, 990u, 33);
    CHECK(xl_serve_gain_log_read(&l, 80, f, gg) == XL_SERVE_GAIN_LOG);
    for (int i = 0; i < XL_SERVE_GAIN_LOG; ++i) CHECK(f[i] == 10u * (uint64_t)(36 + i) && gg[i] == (i == 63 ? 33 : (36 + i) % 40 - 20));
    CHECK(xl_serve_gain_log_read(&l, 3, f, gg) == 3 && f[0] == 970u && f[2] == 990u && gg[2] == 33);
  }
  printf("ok %ld\n", g_count);
  return 0;
}

int main(int argc, char **argv) {
  if (argc == 2 && strcmp(argv[1], "edges") == 0) return edges();
  if (argc == 2 && strcmp(argv[1], "plan") == 0) return plan();
  if (argc == 2 && strcmp(argv[1], "policy") == 0) return policy();
  if (argc == 4 && strcmp(argv[1], "zero") == 0) {
    const long e0 = strtol(argv[2], NULL, 10), e1 = strtol(argv[3], NULL, 10);
    if (e0 >= 0 && e0 <= e1 && e1 <= 255) return zero((uint32_t)e0, (uint32_t)e1);
  }
  if (argc == 5 && strcmp(argv[1], "rule") == 0) {
    const long g = strtol(argv[2], NULL, 10), e0 = strtol(argv[3], NULL, 10), e1 = strtol(argv[4], NULL, 10);
    if (g >= XL_DLV_GAIN_MIN && g <= XL_DLV_GAIN_MAX && e0 >= 0 && e0 <= e1 && e1 <= 255) return rule((int)g, (uint32_t)e0, (uint32_t)e1);
  }
  fprintf(stderr, "usage: %s zero E0 E1 | rule G E0 E1 | edges | plan | policy\n", argv[0]);
  return 2;
}
