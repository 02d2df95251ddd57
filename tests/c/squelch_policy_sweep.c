/* squelch_policy_sweep.c -- the squelch policy and its log (sdr-server_amd/csrc/xl_serve_squelch.h) against a second statement, as a
 * program of its own under ASan and UBSan (tests/test_meter_cpu.py builds and runs it).
 *
 * THE POLICY.  Every sequence of up to MAXLEN calls over four powers -- below the close mark, between the marks, above the open mark,
 * a NaN -- with hang_calls 0 .. 3, the marks apart and equal.  The second statement does not step a state: the gate after call k is
 * open exactly when some call j <= k was not below the open mark and, with j the LAST such call, calls j + 1 .. k hold no run of
 * hang_calls + 1 consecutive calls below the close mark.
 * THE LOG.  The same sequences with row lengths that include 0 (two changes at one stream sample cancel), against the list built from
 * the gates alone; then a run of 65 and more changes through the ring.
 * Prints "sequences N log_checks M" and returns 0, or prints the first difference and returns 1. */
#include <math.h>
#include <stdio.h>
#include <string.h>

#include "xl_serve_squelch.h"

#define MAXLEN 8

static int second_gate(const double *P, int k, double open_power, double close_power, unsigned hang) {
  int j = -1;
  for (int i = 0; i <= k; ++i)
    if (!(P[i] < open_power)) j = i;
  if (j < 0) return 0;
  unsigned run = 0;
  for (int i = j + 1; i <= k; ++i) {
    run = P[i] < close_power ? run + 1u : 0u;
    if (run > hang) return 0;
  }
  return 1;
}

typedef struct {
  uint64_t s, d;
  int open;
} Entry;

int main(void) {
  unsigned long sequences = 0, log_checks = 0;
  for (int equal = 0; equal < 2; ++equal) {
    const double open_power = 1e-3, close_power = equal ? 1e-3 : 2.5e-4;
    if (!xl_serve_squelch_valid(open_power, close_power)) return 1;
    const double sym[4] = {close_power / 2, (open_power + close_power) / 2, open_power * 2, NAN};
    for (unsigned hang = 0; hang <= 3; ++hang)
      for (int len = 1; len <= MAXLEN; ++len)
        for (unsigned long code = 0; code < (1ul << (2 * len)); ++code) {
          double P[MAXLEN];
          uint64_t rows[MAXLEN];
          for (int i = 0; i < len; ++i) {
            P[i] = sym[(code >> (2 * i)) & 3u];
            rows[i] = ((code >> i) ^ (unsigned long)i) % 3u == 0u ? 0u : 100u + (uint64_t)i; /* some calls produce nothing */
          }
          XlServeSquelch q;
          XlServeSquelchLog log;
          memset(&log, 0, sizeof log);
          xl_serve_squelch_init(&q, open_power, close_power, hang);
          Entry want[MAXLEN];
          int nw = 0, prev = 1;
          uint64_t produced = 0, delivered = 0;
          for (int k = 0; k < len; ++k) {
            const int g = xl_serve_squelch_step(&q, P[k]);
            const int w = second_gate(P, k, open_power, close_power, hang);
            if (g != w) {
              printf("policy: equal %d hang %u len %d code %lu call %d: %d, second statement %d\n", equal, hang, len, code, k, g, w);
              return 1;
            }
            xl_serve_squelch_log_note(&log, produced, delivered, g);
            if (w != prev) { /* the second statement of the log: a change, taken back when the previous one is at the same sample */
              if (nw > 0 && want[nw - 1].s == produced) --nw;
              else want[nw].s = produced, want[nw].d = delivered, want[nw].open = w, ++nw;
              prev = w;
            }
            produced += rows[k];
            if (w) delivered += rows[k];
          }
          uint64_t a[XL_SERVE_SQUELCH_LOG], b[XL_SERVE_SQUELCH_LOG];
          uint8_t o[XL_SERVE_SQUELCH_LOG];
          const uint32_t n = xl_serve_squelch_log_read(&log, XL_SERVE_SQUELCH_LOG, a, b, o);
          int bad = n != (uint32_t)nw;
          for (uint32_t i = 0; !bad && i < n; ++i) bad = a[i] != want[i].s || b[i] != want[i].d || o[i] != (uint8_t)want[i].open;
          for (uint32_t i = 1; !bad && i < n; ++i) bad = o[i] == o[i - 1] || a[i] <= a[i - 1];
          if (bad) {
            printf("log: equal %d hang %u len %d code %lu: %u entries, second statement %d\n", equal, hang, len, code, n, nw);
            return 1;
          }
          ++sequences, ++log_checks;
        }
  }
  /* the ring: 64, 65 and 200 changes, every call of one sample, read whole and through a short cap */
  const int changes[3] = {64, 65, 200};
  for (int c = 0; c < 3; ++c) {
    XlServeSquelch q;
    XlServeSquelchLog log;
    memset(&log, 0, sizeof log);
    xl_serve_squelch_init(&q, 1.0, 1.0, 0u);
    uint64_t produced = 0, delivered = 0;
    for (int k = 0; k < changes[c]; ++k) { /* call k: closed for even k (the first change: the log begins open), open for odd k */
      const int g = xl_serve_squelch_step(&q, k % 2 == 0 ? 0.5 : 2.0);
      if (g != k % 2) return 1;
      xl_serve_squelch_log_note(&log, produced, delivered, g);
      produced += 1u, delivered += (uint64_t)g;
    }
    for (uint32_t cap = 0; cap <= 70u; cap += 7u) {
      uint64_t a[80], b[80];
      uint8_t o[80];
      const uint32_t n = xl_serve_squelch_log_read(&log, cap > XL_SERVE_SQUELCH_LOG ? XL_SERVE_SQUELCH_LOG : cap, a, b, o);
      uint32_t have = (uint32_t)changes[c] < XL_SERVE_SQUELCH_LOG ? (uint32_t)changes[c] : XL_SERVE_SQUELCH_LOG;
      if (cap < have) have = cap;
      if (n != have) {
        printf("ring: %d changes, cap %u: %u entries, expected %u\n", changes[c], cap, n, have);
        return 1;
      }
      for (uint32_t i = 0; i < n; ++i) { /* the latest n: change number k = changes - n + i, at stream sample k, k / 2 delivered */
        const uint64_t k = (uint64_t)changes[c] - n + i;
        if (a[i] != k || b[i] != k / 2u || o[i] != (uint8_t)(k % 2u)) {
          printf("ring: %d changes, cap %u, entry %u: (%llu, %llu, %u)\n", changes[c], cap, i, (unsigned long long)a[i],
                 (unsigned long long)b[i], (unsigned)o[i]);
          return 1;
        }
        ++log_checks;
      }
    }
  }
  /* the marks a policy may have */
  if (xl_serve_squelch_valid(1.0, 2.0) || xl_serve_squelch_valid(-1.0, -2.0) || xl_serve_squelch_valid(1.0, -0.5) ||
      xl_serve_squelch_valid(NAN, 0.0) || xl_serve_squelch_valid(1.0, NAN) || xl_serve_squelch_valid(INFINITY, 0.0) ||
      xl_serve_squelch_valid(INFINITY, INFINITY) || !xl_serve_squelch_valid(0.0, 0.0) || !xl_serve_squelch_valid(1e300, 0.0))
    return 1;
  printf("sequences %lu log_checks %lu\n", sequences, log_checks);
  return 0;
}
