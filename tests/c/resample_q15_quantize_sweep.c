/* A stand-alone sweep over sdr-server_amd/csrc/xl_resample_q15_quant.h, built by tests/test_resample_q15_cpu.py with
 * -fsanitize=address,undefined and run as a process of its own: the edges of the range (-1.0 -> -32768, 1.0 refused, the float below
 * 1.0 -> 32767, the floats around -1.0 - 2^-15, tiny and denormal taps -> 0), what is not finite, float32's extremes (whose product
 * overflows), NULL and length 0, and random taps against a double-precision truncation decided without a cast of an out-of-range
 * value.  The out-of-range conversion the header must avoid is what UBSan (float-cast-overflow) reports.  Prints "ok <taps>" or the
 * first difference; exit status 0 or 1. */
#include <errno.h>
#include <float.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include "xl_resample_q15_quant.h"

static uint64_t rng_state = 88172645463325252ull;
static uint64_t rnd(void) {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return rng_state;
}

/* the expected answer: 0 and *c, or -ERANGE */
static int want(float h, int16_t *c) {
  const double v = trunc((double)h * 32768.0); /* (exact in double for every float32 h) */
  if (!(v >= -32768.0 && v <= 32767.0)) return -ERANGE;
  *c = (int16_t)v;
  return 0;
}

static int one(float h, unsigned long *n) {
  int16_t got = 12345, exp = 12345;
  const int rg = xl_resample_q15_quantize(&h, 1, &got), re = want(h, &exp);
  ++*n;
  if (rg != re || (rg == 0 && got != exp)) {
    printf("FAIL h %a: code %d value %d, expected code %d value %d\n", (double)h, rg, got, re, exp);
    return 1;
  }
  return 0;
}

int main(void) {
  unsigned long n = 0;
  int16_t c[4];
  const float edges[] = {-1.0f, 1.0f, nextafterf(1.0f, 0.0f), nextafterf(1.0f, 2.0f), -1e-9f, 1e-9f, 0.0f, -0.0f,
                         nextafterf(-1.0f, 0.0f), nextafterf(-1.0f, -2.0f), -1.0f - 0x1p-15f, nextafterf(-1.0f - 0x1p-15f, 0.0f),
                         nextafterf(-1.0f - 0x1p-15f, -2.0f), 0x1p-15f, nextafterf(0x1p-15f, 0.0f), -0x1p-15f, FLT_MIN, -FLT_MIN,
                         FLT_TRUE_MIN, -FLT_TRUE_MIN, FLT_MAX, -FLT_MAX, 1e30f, -1e30f, 65536.0f, -65536.0f, 2147483648.0f,
                         -2147483904.0f, 4294967296.0f, NAN, -NAN, INFINITY, -INFINITY, 0.5f, -0.5f};
  for (size_t i = 0; i < sizeof edges / sizeof edges[0]; ++i)
    if (one(edges[i], &n)) return 1;
  /* the fixed points of the issue's table */
  {
    const float h[4] = {-1.0f, nextafterf(1.0f, 0.0f), -1e-9f, 0.5f};
    if (xl_resample_q15_quantize(h, 4, c) != 0 || c[0] != -32768 || c[1] != 32767 || c[2] != 0 || c[3] != 16384) {
      printf("FAIL fixed points\n");
      return 1;
    }
    const float bad[3] = {0.25f, 1.0f, 0.25f};
    if (xl_resample_q15_quantize(bad, 3, c) != -ERANGE) {
      printf("FAIL 1.0 inside a prototype\n");
      return 1;
    }
  }
  if (xl_resample_q15_quantize(NULL, 1, c) != -EINVAL || xl_resample_q15_quantize(edges, 0, c) != -EINVAL ||
      xl_resample_q15_quantize(edges, 1, NULL) != -EINVAL) {
    printf("FAIL refusals\n");
    return 1;
  }
  /* random taps: uniform in (-1.25, 1.25), then every bit pattern class through random float bits */
  for (int i = 0; i < 200000; ++i)
    if (one((float)((double)(rnd() >> 11) / 9007199254740992.0 * 2.5 - 1.25), &n)) return 1;
  for (int i = 0; i < 200000; ++i) {
    union { uint32_t u; float f; } b;
    b.u = (uint32_t)rnd();
    if (one(b.f, &n)) return 1;
  }
  /* a heap array of exactly len entries on both sides: ASan sees a step past either end */
  {
    const size_t len = 1927;
    float *h = malloc(len * sizeof *h);
    int16_t *o = malloc(len * sizeof *o);
    if (h == NULL || o == NULL) return 1;
    for (size_t i = 0; i < len; ++i) h[i] = (float)((double)(rnd() >> 11) / 9007199254740992.0 * 1.9 - 0.95);
    if (xl_resample_q15_quantize(h, len, o) != 0) {
      printf("FAIL array\n");
      return 1;
    }
    for (size_t i = 0; i < len; ++i) {
      int16_t e = 0;
      if (want(h[i], &e) != 0 || e != o[i]) {
        printf("FAIL array at %zu\n", i);
        return 1;
      }
    }
    n += len;
    free(h);
    free(o);
  }
  printf("ok %lu\n", n);
  return 0;
}
