/* A stand-alone sweep over sdr-server_amd/csrc/xl_q15_digits.h and the int64 entry of xl_q15_narrow.h, built by
 * tests/test_q15_matrix_cpu.py with gcc alone under ASan and UBSan and run as a process of its own: the host side of the matrix-core
 * Q15 FIR (engine option "q15_kernel") against plain int64 arithmetic.
 *   digits    every entry -32768 .. 32768 (32768 = the negation of a tap of -32768): its digits recombine to it and fit int8, or the
 *             proof rejects it; the edge is exact (32639 accepted, 32640 rejected).  Every cs16 sample: 256 hi + lo + 128.
 *   windows   a tile image built by xl_q15mm_fill_row, then the kernel's own sums in host arithmetic -- per residue class the window
 *             read from the aligned sample below its start, the delayed taps from the image, i32 accumulators checked against 2^31,
 *             the combine -- against the int64 sum of the reference (xlating.c:100-119).  T = 1, 7, 16, 505; D = 1, 2, 3, 7, 8, 42, 64;
 *             samples random, all 32767, all -32768, all 0, missing (the value 0), cu8 / cs8 at 0 / 255 and -128 / 127.
 *   narrowing xl_q15_narrow_sum64 against saturate_to_int16((int32_t)(sum >> 15)) around +-2^30, +-2^46, +-2^47.
 * Prints "ok <checks>" or the first difference; exit status 0 or 1. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "xl_q15_digits.h"

static uint64_t rng_state = 88172645463325252ull;
static uint64_t rnd(void) {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return rng_state;
}

static unsigned long checks = 0;
#define CHECK(c, ...)          \
  do {                         \
    ++checks;                  \
    if (!(c)) {                \
      printf("FAIL %s:%d: ", __FILE__, __LINE__); \
      printf(__VA_ARGS__);     \
      printf("\n");            \
      exit(1);                 \
    }                          \
  } while (0)

static void digits(void) {
  for (int32_t v = -32768; v <= 32768; ++v) {
    int32_t hi, lo;
    xl_q15mm_entry_digits(v, &hi, &lo);
    CHECK(256 * hi + lo == v && lo >= -128 && lo <= 127, "entry %d: hi %d lo %d", v, hi, lo);
    const int fits = hi >= -128 && hi <= 127;
    CHECK(xl_q15mm_entry_ok(v) == fits, "entry %d: proof says %d, digits (%d, %d)", v, xl_q15mm_entry_ok(v), hi, lo);
    CHECK(fits == (v <= XL_QMM_ENTRY_MAX), "entry %d: fits %d", v, fits);
  }
  CHECK(xl_q15mm_entry_ok(32639) && !xl_q15mm_entry_ok(32640) && xl_q15mm_entry_ok(-32768) && !xl_q15mm_entry_ok(32767), "edge");
  for (int32_t x = -32768; x <= 32767; ++x) {
    int32_t hi, lo;
    xl_q15mm_cs16_digits(x, &hi, &lo);
    CHECK(256 * hi + lo + 128 == x && hi >= -128 && hi <= 127 && lo >= -128 && lo <= 127, "sample %d: hi %d lo %d", x, hi, lo);
  }
  /* a client: cr and ci are entries, and so is -ci */
  const int16_t edge[][2] = {{32639, 0}, {32640, 0}, {0, 32639}, {0, 32640}, {0, -32639}, {0, -32640}, {-32768, 0}, {0, -32768}, {32767, 0}};
  const int want[] = {1, 0, 1, 0, 1, 0, 1, 0, 0};
  for (size_t i = 0; i < sizeof want / sizeof want[0]; ++i) {
    int16_t taps[6] = {100, -200, edge[i][0], edge[i][1], -32639, 32639};
    CHECK(xl_q15mm_admits_taps(taps, 3) == want[i], "taps (%d, %d): admitted %d", edge[i][0], edge[i][1], !want[i]);
  }
  /* proof (b) at the longest non-wide filter, and where it would stop holding */
  CHECK(xl_q15mm_acc_bounded(xl_q15mm_ksteps(16384)) && !xl_q15mm_acc_bounded(2048), "accumulator bound");
}

enum { S_RANDOM, S_MAX, S_MIN, S_ZERO, S_MISSING, S_KINDS };

/* one (T, D, format, sample kind): fmt 0 = cu8, 1 = cs8, 2 = cs16 */
static void window(uint32_t T, uint32_t D, int fmt, int kind, int tapkind) {
  const uint32_t ksteps = xl_q15mm_ksteps(T), P = xl_q15mm_residues(D), nc = 2u, nout = XL_QMM_WAVES * nc;
  const uint32_t span = (uint32_t)xl_q15mm_span(D, ksteps, nc);
  const uint32_t row = (uint32_t)(rnd() % XL_QMM_ROWS);
  int16_t *rtq = malloc(2u * T * sizeof *rtq);
  for (uint32_t i = 0; i < 2u * T; ++i) {
    const int32_t lim = (i & 1u) ? 32639 : 32768; /* ci >= -32639; cr >= -32768 */
    int32_t v = tapkind == 0 ? (int32_t)(rnd() % 65279u) - 32639 : (tapkind == 1 ? 32639 : -lim);
    if (tapkind == 3) v = (rnd() & 1u) ? 32639 : -lim;
    rtq[i] = (int16_t)v;
  }
  CHECK(xl_q15mm_admits_taps(rtq, T), "T %u: the sweep's own taps are not admitted", T);
  const size_t bytes = (size_t)xl_q15mm_image_bytes(D, ksteps);
  int8_t *image = calloc(bytes, 1);
  xl_q15mm_fill_row(image, row, rtq, T, D, ksteps);
  /* the window image: values, presence, digit planes as the kernel stages them */
  int32_t *xv = malloc(2u * span * sizeof *xv);
  int8_t *p0 = malloc(2u * span), *p1 = malloc(2u * span);
  for (uint32_t j = 0; j < 2u * span; ++j) {
    int present = kind != S_MISSING && !(kind == S_RANDOM && rnd() % 16u == 0u);
    int32_t raw;
    if (fmt == 2) {
      raw = kind == S_MAX ? 32767 : (kind == S_MIN ? -32768 : (kind == S_ZERO ? 0 : (int32_t)(rnd() % 65536u) - 32768));
      xv[j] = present ? raw : 0;
      int32_t hi, lo;
      xl_q15mm_cs16_digits(xv[j], &hi, &lo); /* a missing sample is the VALUE 0: hi = 0, lo = -128 */
      p0[j] = (int8_t)hi, p1[j] = (int8_t)lo;
    } else {
      const int32_t lo8 = fmt == 0 ? 0 : -128, hi8 = fmt == 0 ? 255 : 127;
      raw = kind == S_MAX ? hi8 : (kind == S_MIN ? lo8 : (kind == S_ZERO ? (fmt == 0 ? 128 : 0) : lo8 + (int32_t)(rnd() % 256u)));
      const int32_t d = present ? (fmt == 0 ? raw - 128 : raw) : 0; /* xlating.c:418, 425 */
      xv[j] = d * 256;
      p0[j] = (int8_t)d, p1[j] = 0;
    }
  }
  const int64_t corr[2] = {xl_q15mm_correction(rtq, T, 0), xl_q15mm_correction(rtq, T, 1)};
  for (uint32_t i = 0; i < nout; ++i) {
    const uint32_t r = i % P, s = xl_q15mm_shift(D, r);
    CHECK((i * D) % 8u == s && i * D >= s, "T %u D %u output %u: residue %u, shift %u", T, D, i, r, s);
    const uint32_t start = i * D - s;
    for (int part = 0; part < 2; ++part) {
      /* the reference: int64 sum over the window of output i */
      int64_t want = 0;
      for (uint32_t t = 0; t < T; ++t) {
        const int64_t xr = xv[2u * (i * D + t)], xi = xv[2u * (i * D + t) + 1u], cr = rtq[2u * t], ci = rtq[2u * t + 1u];
        want += part == 0 ? xr * cr - xi * ci : xr * ci + xi * cr;
      }
      /* the kernel: four (cs16) or two (8-bit) digit sums over K = 32 ksteps entries, operands from the image and the planes */
      int64_t hh = 0, mid = 0, ll = 0;
      for (uint32_t kk = 0; kk < ksteps; ++kk)
        for (uint32_t h = 0; h < 2u; ++h)
          for (uint32_t e = 0; e < 16u; ++e) {
            const uint64_t at = ((uint64_t)kk * 64u + (row + 32u * h)) * 16u + e;
            const int32_t ah = image[(((uint64_t)r * 4u + 2u * (uint32_t)part) * ksteps) * XL_QMM_FRAG + at];
            const int32_t al = image[(((uint64_t)r * 4u + 2u * (uint32_t)part + 1u) * ksteps) * XL_QMM_FRAG + at];
            const uint32_t k = 2u * start + 32u * kk + 16u * h + e;
            CHECK(k < 2u * span, "T %u D %u output %u: window read at %u of %u", T, D, i, k, 2u * span);
            hh += ah * p0[k];
            ll += al * (fmt == 2 ? p1[k] : p0[k]);
            if (fmt == 2) mid += ah * p1[k] + al * p0[k];
          }
      CHECK(llabs(hh) < ((int64_t)1 << 31) && llabs(mid) < ((int64_t)1 << 31) && llabs(ll) < ((int64_t)1 << 31), "T %u: accumulator", T);
      const int64_t got = fmt == 2 ? xl_q15mm_combine16((int32_t)hh, (int32_t)mid, (int32_t)ll, corr[part])
                                   : xl_q15mm_combine8((int32_t)hh, (int32_t)ll);
      CHECK(got == want, "T %u D %u fmt %d kind %d taps %d output %u part %d: got %lld, want %lld", T, D, fmt, kind, tapkind, i, part,
            (long long)got, (long long)want);
      CHECK(xl_q15_narrow_sum64(got) == xl_sat16((int32_t)(uint32_t)(uint64_t)(want >> 15)), "narrowed");
    }
  }
  /* the other rows of the tile stayed zero */
  for (size_t b = 0; b < bytes; ++b)
    if (((b / 16u) % 64u) % 32u != row) CHECK(image[b] == 0, "image byte %zu of another row", b);
  free(rtq), free(image), free(xv), free(p0), free(p1);
}

static int32_t want_narrow(int64_t sum) {
  const int32_t v = (int32_t)(uint32_t)(uint64_t)(sum >> 15);
  return v > 32767 ? 32767 : (v < -32768 ? -32768 : v);
}

static void narrowing(void) {
  const int64_t centres[] = {(int64_t)1 << 30, -((int64_t)1 << 30), (int64_t)1 << 46, -((int64_t)1 << 46), (int64_t)1 << 47,
                             -((int64_t)1 << 47), 0, (int64_t)32767 << 15, -((int64_t)32768 << 15), ((int64_t)1 << 46) - 32768};
  for (size_t c = 0; c < sizeof centres / sizeof centres[0]; ++c)
    for (int64_t off = -70000; off <= 70000; ++off) {
      const int64_t sum = centres[c] + off;
      CHECK(xl_q15_narrow_sum64(sum) == want_narrow(sum), "sum %lld: got %d, want %d", (long long)sum, xl_q15_narrow_sum64(sum), want_narrow(sum));
    }
  for (int i = 0; i < 200000; ++i) {
    const int64_t mag = (int64_t)((rnd() >> 12) >> (rnd() % 52u));
    const int64_t sum = (rnd() & 1u) ? mag : -mag;
    CHECK(xl_q15_narrow_sum64(sum) == want_narrow(sum), "sum %lld", (long long)sum);
  }
}

int main(void) {
  digits();
  const uint32_t Ts[] = {1, 7, 16, 505}, Ds[] = {1, 2, 3, 7, 8, 42, 64};
  for (size_t ti = 0; ti < 4; ++ti)
    for (size_t di = 0; di < 7; ++di)
      for (int fmt = 0; fmt < 3; ++fmt)
        for (int kind = 0; kind < S_KINDS; ++kind) window(Ts[ti], Ds[di], fmt, kind, (int)((ti + di + (size_t)kind) % 4u));
  narrowing();
  printf("ok %lu\n", checks);
  return 0;
}
