/* xl_serve_gain.h -- the automatic gain of a client of the serve object (xlating_serve_set_auto_gain) and its gain log.  Plain C, no
 * HIP, integers only: state in, decision out, like xl_ahead.h; tests/c/delivery_gain_sweep.c drives it under the sanitizers.
 *
 * After each delivered call the policy takes the level the delivery reported for the client's row (peak_bits, clipped:
 * xl_dlv_gain.h) and the gain g the row was packed with, and computes top, the exponent with |peak| * 2^g in [2^(top - 1), 2^top):
 *   clipped > 0 or top > 0:   g -= max(1, top)   -- the next row packed peaks in [1/2, 1) of full scale if the level holds;
 *   else peak != 0 and top <= XL_SERVE_GAIN_LOW_TOP in each of the last XL_SERVE_GAIN_QUIET_CALLS delivered calls:  g += 1, and the
 *                             count restarts;
 *   silence (peak == 0) changes nothing, neither the gain nor the count.
 * g is held in XL_SERVE_GAIN_MIN .. XL_SERVE_GAIN_MAX.  A constant level therefore ends with |peak| * 2^g in [1/8, 1) and stays
 * there: top = -2, -1 and 0 move nothing.  (One magnitude band clips at top = 0: a peak whose 16-bit rounding is 32768, the top 15
 * bits of the fraction set; it is taken down one more step, to top = -1.)
 * The constants are policy, not measurements.
 * The gain that packed a call is not the latest decision when calls overlap: `g_packed` is what the levels were measured under, and the
 * decision is relative to the CURRENT gain only through it -- the step is applied to g_packed, and taken only if it lowers the current
 * gain (a drop) or, for a raise, if the current gain is still g_packed (no decision is pending between). */
#ifndef XL_SERVE_GAIN_H_
#define XL_SERVE_GAIN_H_

#include <stdint.h>

#define XL_SERVE_GAIN_MIN (-48)
#define XL_SERVE_GAIN_MAX 48
#define XL_SERVE_GAIN_QUIET_CALLS 8 /* delivered calls in a row below the low mark before the gain rises one step */
#define XL_SERVE_GAIN_LOW_TOP (-3)  /* the low mark: |peak| * 2^g below 2^-3 of full scale */
#define XL_SERVE_GAIN_LOG 64        /* gain changes remembered per client */

typedef struct {
  int32_t quiet; /* delivered calls in a row with top <= XL_SERVE_GAIN_LOW_TOP */
} XlServeGainState;

/* the exponent `top` with |peak| * 2^g in [2^(top - 1), 2^top); peak_bits != 0 */
static inline int32_t xl_serve_gain_top(uint32_t peak_bits, int32_t g) {
  const uint32_t e = (peak_bits >> 23) & 0xFFu, frac = peak_bits & 0x7FFFFFu;
  if (e != 0u) return (int32_t)e - 126 + g; /* 1.f * 2^(e - 127) */
  int32_t b = 0;                            /* a denormal: frac * 2^-149, its highest set bit b */
  while ((frac >> (b + 1)) != 0u) ++b;
  return b - 148 + g;
}

static inline int32_t xl_serve_gain_hold(int32_t g) {
  return g < XL_SERVE_GAIN_MIN ? XL_SERVE_GAIN_MIN : (g > XL_SERVE_GAIN_MAX ? XL_SERVE_GAIN_MAX : g);
}

/* One delivered call: the row's peak_bits and clipped, packed under g_packed; g_now: the client's gain at this moment.  Returns the
 * gain from the next call that is packed (g_now when nothing changes). */
static inline int32_t xl_serve_gain_step(XlServeGainState *st, uint32_t peak_bits, uint32_t clipped, int32_t g_packed, int32_t g_now) {
  if (peak_bits == 0u && clipped == 0u) return g_now; /* silence */
  const int32_t top = peak_bits != 0u ? xl_serve_gain_top(peak_bits, g_packed) : 0;
  if (clipped > 0u || top > 0) {
    const int32_t want = xl_serve_gain_hold(g_packed - (top > 1 ? top : 1));
    st->quiet = 0;
    return want < g_now ? want : g_now;
  }
  if (top > XL_SERVE_GAIN_LOW_TOP) {
    st->quiet = 0;
    return g_now;
  }
  if (++st->quiet < XL_SERVE_GAIN_QUIET_CALLS) return g_now;
  st->quiet = 0;
  return g_now == g_packed ? xl_serve_gain_hold(g_now + 1) : g_now;
}

/* the latest XL_SERVE_GAIN_LOG gain changes of a client, oldest first */
typedef struct {
  uint64_t first_sample[XL_SERVE_GAIN_LOG]; /* index in the client's delivered stream of the first sample under the gain */
  int8_t gain[XL_SERVE_GAIN_LOG];
  uint32_t n;     /* entries held */
  uint32_t head;  /* the oldest */
} XlServeGainLog;

static inline void xl_serve_gain_log_add(XlServeGainLog *l, uint64_t first_sample, int32_t g) {
  /* two changes before any sample was packed between them: the later one stands */
  if (l->n > 0u && l->first_sample[(l->head + l->n - 1u) % XL_SERVE_GAIN_LOG] == first_sample) {
    l->gain[(l->head + l->n - 1u) % XL_SERVE_GAIN_LOG] = (int8_t)g;
    return;
  }
  if (l->n == XL_SERVE_GAIN_LOG) l->head = (l->head + 1u) % XL_SERVE_GAIN_LOG, --l->n;
  const uint32_t at = (l->head + l->n) % XL_SERVE_GAIN_LOG;
  l->first_sample[at] = first_sample, l->gain[at] = (int8_t)g;
  ++l->n;
}

/* copies up to cap entries, the latest ones, oldest first; returns how many */
static inline uint32_t xl_serve_gain_log_read(const XlServeGainLog *l, uint32_t cap, uint64_t *first_sample, int8_t *gain) {
  const uint32_t n = l->n < cap ? l->n : cap;
  for (uint32_t i = 0; i < n; ++i) {
    const uint32_t at = (l->head + (l->n - n) + i) % XL_SERVE_GAIN_LOG;
    first_sample[i] = l->first_sample[at], gain[i] = l->gain[at];
  }
  return n;
}

#endif /* XL_SERVE_GAIN_H_ */
