/* tests/c/tune_rule_sweep.c -- the tuner bank's rule (csrc/xl_tune_rule.h, and csrc/xl_tune_hz.h for the steps from Hz) held to its
 * contract by a program of its own, compiled by tests/tune_ref.py under ASan and UBSan (tests/test_tune_cpu.py):
 *   cs A B   xl_tune_cs over the phases [A 2^24, (B + 1) 2^24), 0 <= A <= B <= 255: against libm's double cos and sin of the same
 *            32-bit phase, the exact points, both symmetries bit for bit as values.  Prints "ok <phases> <E> <circle>": the largest
 *            absolute error of c and s, and the largest |c^2 + s^2 - 1|, both as %a; fails unless E <= 2^-22.
 *   phase    the phase arithmetic against 128-bit integers: the closed form against stepwise addition, the stride, advance(n1) then
 *            advance(n2) against advance(n1 + n2); F and R in 0, +-1, +-(2^63 - 1), INT64_MIN and random; n up to 2^30.
 *   hz       xl_tune_from_hz against the stated double expression, and its refusals.
 * Each prints "ok <checks> ..." and exits 0, or names the first failure and exits 1. */
#include <inttypes.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "xl_tune_hz.h"
#include "xl_tune_rule.h"

__extension__ typedef __int128 i128;

#define CHECK(cond, ...)                                    \
  do {                                                      \
    if (!(cond)) {                                          \
      printf("FAILED %s:%d: %s: ", __FILE__, __LINE__, #cond); \
      printf(__VA_ARGS__);                                  \
      printf("\n");                                         \
      exit(1);                                              \
    }                                                       \
  } while (0)

static const double TWO_PI = 6.283185307179586476925286766559;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rng(void) { /* splitmix64 */
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

static int sweep_cs(uint32_t A, uint32_t B) {
  double E = 0.0, circle = 0.0;
  uint64_t count = 0;
  for (uint64_t p64 = (uint64_t)A << 24; p64 < ((uint64_t)B + 1u) << 24; ++p64) {
    const uint32_t p = (uint32_t)p64;
    float c, s, c1, s1, c2, s2;
    xl_tune_cs(p, &c, &s);
    const double t = TWO_PI * ((double)p / 4294967296.0);
    const double ec = fabs((double)c - cos(t)), es = fabs((double)s - sin(t));
    E = ec > E ? ec : E, E = es > E ? es : E;
    const double r = fabs((double)c * (double)c + (double)s * (double)s - 1.0);
    circle = r > circle ? r : circle;
    xl_tune_cs(p + 0x40000000u, &c1, &s1);
    CHECK(c1 == -s && s1 == c, "quarter turn at p = %" PRIu32, p);
    xl_tune_cs(0u - p, &c2, &s2);
    CHECK(c2 == c && s2 == -s, "negation at p = %" PRIu32, p);
    if ((p & 0x3FFFFFFFu) == 0u) {
      const uint32_t k = p >> 30;
      const float wc = k == 0u ? 1.0f : (k == 2u ? -1.0f : 0.0f), ws = k == 1u ? 1.0f : (k == 3u ? -1.0f : 0.0f);
      CHECK(c == wc && s == ws, "exact point k = %" PRIu32 ": %a %a", k, (double)c, (double)s);
    }
    ++count;
  }
  CHECK(E <= ldexp(1.0, -22), "E = %a", E);
  printf("ok %" PRIu64 " %a %a\n", count, E, circle);
  return 0;
}

static uint64_t ref_phase(uint64_t P, int64_t F, int64_t R, uint64_t j) {
  const i128 tri = ((i128)j * ((i128)j - 1)) / 2;
  return (uint64_t)((i128)P + (i128)j * (i128)F + tri * (i128)R); /* (to unsigned: modulo 2^64) */
}

static int sweep_phase(void) {
  const int64_t fixed[] = {0, 1, -1, INT64_MAX, -INT64_MAX, INT64_MIN};
  const uint64_t counts[] = {0, 1, 2, 3, 255, 256, 257, 2047, 2048, 2049, 65535, 1u << 20, (1u << 30) - 1u, 1u << 30};
  const size_t NF = sizeof(fixed) / sizeof(fixed[0]), NC = sizeof(counts) / sizeof(counts[0]);
  int64_t vals[6 + 10];
  for (size_t i = 0; i < NF; ++i) vals[i] = fixed[i];
  for (size_t i = NF; i < NF + 10; ++i) vals[i] = (int64_t)rng();
  const size_t NV = NF + 10;
  uint64_t checks = 0;
  for (size_t a = 0; a < NV; ++a)
    for (size_t b = 0; b < NV; ++b) {
      const int64_t F = vals[a], R = vals[b];
      const uint64_t P = (a + b) % 3 == 0 ? UINT64_MAX : rng();
      /* stepwise addition against the closed form and the 128-bit reference */
      uint64_t phi = P, f = (uint64_t)F;
      for (uint64_t j = 0; j < 5000; ++j) {
        CHECK(xl_tune_phase(P, F, R, j) == phi && ref_phase(P, F, R, j) == phi, "phase j = %" PRIu64 " F = %" PRId64 " R = %" PRId64, j, F, R);
        phi += f, f += (uint64_t)R;
        ++checks;
      }
      for (size_t c = 0; c < NC; ++c) {
        const uint64_t n = counts[c];
        CHECK(xl_tune_phase(P, F, R, n) == ref_phase(P, F, R, n), "phase n = %" PRIu64, n);
        /* the stride a kernel steps by: S samples on, and its own step */
        for (uint64_t S = 1; S <= 256; S *= 4) {
          const uint64_t d = xl_tune_stride(F, R, n, S);
          CHECK(xl_tune_phase(P, F, R, n) + d == ref_phase(P, F, R, n + S), "stride n = %" PRIu64 " S = %" PRIu64, n, S);
          CHECK(d + S * S * (uint64_t)R == xl_tune_stride(F, R, n + S, S), "stride step n = %" PRIu64 " S = %" PRIu64, n, S);
          checks += 2;
        }
        /* advance(n1) then advance(n2) against advance(n1 + n2), n1 + n2 = n */
        const uint64_t n1 = n == 0 ? 0 : rng() % (n + 1u), n2 = n - n1;
        uint64_t Pa = P, Pb = P;
        int64_t Fa = F, Fb = F;
        xl_tune_advance(&Pa, &Fa, R, n1);
        xl_tune_advance(&Pa, &Fa, R, n2);
        xl_tune_advance(&Pb, &Fb, R, n);
        CHECK(Pa == Pb && Fa == Fb, "advance %" PRIu64 " + %" PRIu64, n1, n2);
        CHECK(Pb == ref_phase(P, F, R, n) && (uint64_t)Fb == (uint64_t)((i128)F + (i128)n * (i128)R), "advance n = %" PRIu64, n);
        /* the sample after a split is the sample of the whole */
        CHECK(xl_tune_phase(Pa, Fa, R, 3) == ref_phase(P, F, R, n + 3u), "continuity at n = %" PRIu64, n);
        checks += 4;
      }
    }
  printf("ok %" PRIu64 "\n", checks);
  return 0;
}

static int sweep_hz(void) {
  uint64_t checks = 0;
  const double rates[] = {48000.0, 44100.0, 2016000.0 / 42.0, 2016000.0 * 160.0 / (42.0 * 147.0), 1.0, 3.0e9};
  const double shifts[] = {0.0, 1.0, -1.0, 1234.5, -10000.0, 0.1, 1e-9, 23999.999, -23999.999};
  for (size_t r = 0; r < sizeof(rates) / sizeof(rates[0]); ++r)
    for (size_t a = 0; a < sizeof(shifts) / sizeof(shifts[0]); ++a)
      for (size_t b = 0; b < sizeof(shifts) / sizeof(shifts[0]); ++b) {
        const double rate = rates[r], sh = shifts[a], ra = shifts[b];
        const double qf = sh / rate, qr = ra / rate / rate;
        const int want = isfinite(qf) && isfinite(qr) && fabs(qf) < 0.5 && fabs(qr) < 0.5 ? 0 : -22;
        int64_t F = 7, R = 7;
        const int rc = xl_tune_from_hz(sh, ra, rate, &F, &R);
        CHECK(rc == want, "from_hz(%g, %g, %g) = %d", sh, ra, rate, rc);
        if (rc == 0)
          CHECK(F == (int64_t)llrint(ldexp(sh / rate, 64)) && R == (int64_t)llrint(ldexp(ra / rate / rate, 64)), "from_hz(%g, %g, %g)", sh, ra, rate);
        else
          CHECK(F == 7 && R == 7, "a refusal wrote");
        ++checks;
      }
  /* the refusals by name */
  const double bad[][3] = {{24000.0, 0.0, 48000.0}, {-24000.0, 0.0, 48000.0}, {0.0, 0.5, 1.0},     {0.0, -0.5, 1.0}, {1.0, 0.0, 0.0},
                           {0.0, 1.0, 0.0},         {NAN, 0.0, 48000.0},      {0.0, NAN, 48000.0}, {INFINITY, 0.0, 48000.0},
                           {0.0, -INFINITY, 48000.0}, {1.0, 1.0, NAN}};
  for (size_t i = 0; i < sizeof(bad) / sizeof(bad[0]); ++i) {
    int64_t F = 7, R = 7;
    CHECK(xl_tune_from_hz(bad[i][0], bad[i][1], bad[i][2], &F, &R) == -22 && F == 7 && R == 7, "refusal %zu", i);
    ++checks;
  }
  /* the edge that passes: the largest double below a half */
  int64_t F = 0, R = 0;
  CHECK(xl_tune_from_hz(nextafter(0.5, 0.0), nextafter(-0.5, 0.0), 1.0, &F, &R) == 0, "below a half");
  CHECK(F == INT64_MAX - 1023 && R == -(INT64_MAX - 1023), "below a half: %" PRId64 " %" PRId64, F, R);
  CHECK(xl_tune_from_hz(12000.0, 0.0, 48000.0, &F, &R) == 0 && F == (int64_t)1 << 62 && R == 0, "a quarter");
  checks += 3;
  printf("ok %" PRIu64 "\n", checks);
  return 0;
}

int main(int argc, char **argv) {
  if (argc == 4 && strcmp(argv[1], "cs") == 0) {
    const long A = strtol(argv[2], NULL, 10), B = strtol(argv[3], NULL, 10);
    if (A < 0 || B < A || B > 255) return 2;
    return sweep_cs((uint32_t)A, (uint32_t)B);
  }
  if (argc == 2 && strcmp(argv[1], "phase") == 0) return sweep_phase();
  if (argc == 2 && strcmp(argv[1], "hz") == 0) return sweep_hz();
  fprintf(stderr, "usage: %s cs A B | phase | hz\n", argv[0]);
  return 2;
}
