/* xl_serve_squelch.h -- the squelch of a client of the serve object (xlating_serve_set_squelch) and its log.  Plain C, no HIP: state
 * in, decision out, like xl_serve_gain.h; tests/c/squelch_policy_sweep.c drives it under the sanitizers.
 *
 * Per client: two marks, open_power >= close_power >= 0 (doubles, both finite; mean power as the meter gives it: xl_meter_rule.h), and
 * hang_calls.  State: the gate (closed at first) and `below`, the calls in a row under the close mark while the gate is open.
 * One call with power P:
 *   P is not below open_power (a NaN included):    the gate opens, below = 0;
 *   gate open and P < close_power:                  ++below, and the gate closes once below exceeds hang_calls;
 *   gate open and close_power <= P < open_power:    below = 0, the gate stays open;
 *   gate closed and P < open_power:                 it stays closed.
 * The row of THIS call is delivered exactly when the gate is open after the step: the decision is made on the same call's power, so a
 * transmission's first call is delivered whole, and hang_calls = h still delivers h calls below the close mark.  A power that is not
 * finite opens: a broken stream is never hidden.
 * The constants are policy, not measurements. */
#ifndef XL_SERVE_SQUELCH_H_
#define XL_SERVE_SQUELCH_H_

#include <stdint.h>

#define XL_SERVE_SQUELCH_LOG 64 /* gate changes remembered per client */

typedef struct {
  double open_power, close_power;
  uint32_t hang_calls;
  uint32_t below; /* calls in a row under the close mark, gate open */
  uint8_t open;   /* the gate */
} XlServeSquelch;

/* 1: the marks are a policy's (both finite, open_power >= close_power >= 0) */
static inline int xl_serve_squelch_valid(double open_power, double close_power) {
  /* (a NaN fails every comparison; an infinity fails the last two) */
  return close_power >= 0.0 && open_power >= close_power && open_power <= 1.7976931348623157e308 && close_power <= 1.7976931348623157e308;
}

static inline void xl_serve_squelch_init(XlServeSquelch *q, double open_power, double close_power, uint32_t hang_calls) {
  q->open_power = open_power, q->close_power = close_power, q->hang_calls = hang_calls;
  q->below = 0u, q->open = 0u;
}

/* One call with power P.  Returns the gate after the step: 1 delivers this call's row. */
static inline int xl_serve_squelch_step(XlServeSquelch *q, double P) {
  if (!(P < q->open_power)) {
    q->open = 1u, q->below = 0u;
  } else if (q->open) {
    if (P < q->close_power) {
      if (++q->below > q->hang_calls) q->open = 0u, q->below = 0u;
    } else {
      q->below = 0u;
    }
  }
  return (int)q->open;
}

/* The latest XL_SERVE_SQUELCH_LOG gate changes of a client, oldest first: from sample stream_sample of the stream the client PRODUCED
 * the gate is `open`, and at that point the client had been DELIVERED delivered_sample samples.  A client without a squelch is
 * delivered: the log of a client (zeroed at first) begins in the open state, and xl_serve_squelch_log_note adds an entry only when the
 * gate it is told differs from the state the log is in, so the entries alternate.  Two changes at the same stream sample (calls that
 * produced nothing between them) cancel: the entry is taken back. */
typedef struct {
  uint64_t stream_sample[XL_SERVE_SQUELCH_LOG];
  uint64_t delivered_sample[XL_SERVE_SQUELCH_LOG];
  uint8_t open[XL_SERVE_SQUELCH_LOG];
  uint32_t n;     /* entries held */
  uint32_t head;  /* the oldest */
  uint8_t closed; /* the state the log is in: 0 open (a zeroed log), 1 closed */
} XlServeSquelchLog;

static inline void xl_serve_squelch_log_note(XlServeSquelchLog *l, uint64_t stream_sample, uint64_t delivered_sample, int open) {
  if ((open == 0) == (l->closed != 0u)) return;
  l->closed = (uint8_t)(open == 0);
  if (l->n > 0u && l->stream_sample[(l->head + l->n - 1u) % XL_SERVE_SQUELCH_LOG] == stream_sample) {
    --l->n;
    return;
  }
  if (l->n == XL_SERVE_SQUELCH_LOG) l->head = (l->head + 1u) % XL_SERVE_SQUELCH_LOG, --l->n;
  const uint32_t at = (l->head + l->n) % XL_SERVE_SQUELCH_LOG;
  l->stream_sample[at] = stream_sample, l->delivered_sample[at] = delivered_sample, l->open[at] = (uint8_t)(open != 0);
  ++l->n;
}

/* copies up to cap entries, the latest ones, oldest first; returns how many */
static inline uint32_t xl_serve_squelch_log_read(const XlServeSquelchLog *l, uint32_t cap, uint64_t *stream_sample, uint64_t *delivered_sample,
                                                 uint8_t *open) {
  const uint32_t n = l->n < cap ? l->n : cap;
  for (uint32_t i = 0; i < n; ++i) {
    const uint32_t at = (l->head + (l->n - n) + i) % XL_SERVE_SQUELCH_LOG;
    stream_sample[i] = l->stream_sample[at], delivered_sample[i] = l->delivered_sample[at], open[i] = l->open[at];
  }
  return n;
}

#endif /* XL_SERVE_SQUELCH_H_ */
