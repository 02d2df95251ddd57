/* A stand-alone sweep over sdr-server_amd/csrc/xl_q15_narrow.h, built by tests/test_q15_extremes_cpu.py with gcc alone and run as a
 * process of its own: xl_q15_narrow_sum(double) of an int64 sum held in a double against the reference's own line in plain integer
 * arithmetic, saturate_to_int16((int32_t)(sum >> 15)) (xlating.c:85-90, 118-119) -- at +-(2^46 - 1) and +-2^46 (the shifted sum on
 * both sides of +-2^31), at the sums whose shifted value is 2^31 - 1, 2^31, -2^31 and -2^31 - 1 with the lowest 15 bits clear and
 * set, around every multiple of 2^47 (where the cut to 32 bits comes back to 0), at the edges of int16, and on random sums below
 * 2^52.  Prints "ok <sums>" or the first difference; exit status 0 or 1. */
#include <stdint.h>
#include <stdio.h>

#include "xl_q15_narrow.h"

static uint64_t rng_state = 88172645463325252ull;
static uint64_t rnd(void) {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return rng_state;
}

/* the reference's line: >> of a negative int64 is the arithmetic shift on every compiler this project builds with (the reference relies
 * on it too); the cut to 32 bits is written on unsigned values */
static int32_t want(int64_t sum) {
  const int64_t q = sum >> 15;
  const int32_t v = (int32_t)(uint32_t)(uint64_t)q;
  return v > 32767 ? 32767 : (v < -32768 ? -32768 : v);
}

static int one(int64_t sum, unsigned long *n) {
  const double acc = (double)sum; /* |sum| < 2^53: exact */
  if ((int64_t)acc != sum) {
    printf("FAIL the sweep's own sum %lld is not a double\n", (long long)sum);
    return 1;
  }
  const int32_t got = xl_q15_narrow_sum(acc), exp = want(sum);
  ++*n;
  if (got != exp) {
    printf("FAIL sum %lld (>> 15 = %lld): got %d, expected %d\n", (long long)sum, (long long)(sum >> 15), got, exp);
    return 1;
  }
  return 0;
}

int main(void) {
  unsigned long n = 0;
  const int64_t p46 = (int64_t)1 << 46, p31 = (int64_t)1 << 31;
  const int64_t shifted[] = {p31 - 1, p31, -p31, -p31 - 1, p31 + 1, -p31 + 1, 32767, 32768, -32768, -32769, 0, -1, 1,
                             2 * p31 - 1, 2 * p31, -2 * p31, -2 * p31 - 1, 2 * p31 + 32767, 2 * p31 + 32768, 3 * p31, -3 * p31 - 1};
  const int64_t direct[] = {p46 - 1, -(p46 - 1), p46, -p46, p46 + 1, -p46 - 1, 0, -1, 1, 32767, 32768, -32768, -32769};
  for (size_t i = 0; i < sizeof direct / sizeof direct[0]; ++i)
    if (one(direct[i], &n)) return 1;
  for (size_t i = 0; i < sizeof shifted / sizeof shifted[0]; ++i) {
    const int64_t lo = shifted[i] * 32768; /* the smallest sum with this shifted value, then the largest, then one in between */
    if (one(lo, &n) || one(lo + 32767, &n) || one(lo + 12345, &n)) return 1;
  }
  /* the fixed point of xl_q15_narrow.h's header: 65700 taps of 32764 over samples of 32767 */
  {
    const int64_t sum = (int64_t)65700 * 32764 * 32767;
    if ((sum >> 15) != 2152529108ll || want(sum) != -32768 || one(sum, &n)) {
      printf("FAIL the 65700-tap window: sum >> 15 = %lld\n", (long long)(sum >> 15));
      return 1;
    }
  }
  for (int i = 0; i < 200000; ++i) { /* uniform below 2^52, both signs */
    const int64_t mag = (int64_t)(rnd() >> 12);
    if (one((rnd() & 1u) ? mag : -mag, &n)) return 1;
  }
  for (int i = 0; i < 200000; ++i) { /* every magnitude: a random number of leading bits dropped */
    const int64_t mag = (int64_t)((rnd() >> 12) >> (rnd() % 52u));
    if (one((rnd() & 1u) ? mag : -mag, &n)) return 1;
  }
  printf("ok %lu\n", n);
  return 0;
}
