/* xl_tune_hz.h -- the tuner bank's steps from Hz (xlating_tune_from_hz).  Plain C for the HOST alone: double arithmetic and libm, which
 * the rule the device runs (xl_tune_rule.h) has none of; xl_tune.hip does not include this.  tests/c/tune_rule_sweep.c holds it to the
 * stated expression and its refusals. */
#ifndef XL_TUNE_HZ_H_
#define XL_TUNE_HZ_H_

#include <math.h>
#include <stdint.h>

/* F = llrint(ldexp(shift_hz / rate, 64)), R = llrint(ldexp(ramp_hz_per_s / rate / rate, 64)) in double; 0, or -22 (-EINVAL) unless both
 * quotients are finite and below 0.5 in magnitude (nothing is written then) */
static inline int xl_tune_from_hz(double shift_hz, double ramp_hz_per_s, double rate, int64_t *F, int64_t *R) {
  const double qf = shift_hz / rate, qr = ramp_hz_per_s / rate / rate;
  if (!(fabs(qf) < 0.5) || !(fabs(qr) < 0.5)) return -22; /* (a NaN and an infinity fail both comparisons) */
  *F = (int64_t)llrint(ldexp(qf, 64));
  *R = (int64_t)llrint(ldexp(qr, 64));
  return 0;
}

#endif /* XL_TUNE_HZ_H_ */
