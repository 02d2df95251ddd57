/*
 * The Q15 resampler bank: xlating_resample.h's second stage for the cs16 output family.  MANY independent streams of int16 (re, im)
 * pairs -- the batch engine's device rows after an XL_MODE_Q15 call -- each taken by its own rational factor L / M to exactly the
 * rate its client asked for, in exact integer arithmetic, int16 pairs out.  One feed advances every stream with two kernel launches
 * and one table copy, however many streams it carries.  An engine call is one family for all its clients, and so is a bank: a float
 * bank's handle given to a function of this header is -EINVAL, and the other way round.  Plain C ABI, no HIP header: streams are
 * void *.  Library: lib/libxlating_resample.so.
 *
 * Per stream: coprime L, M >= 1, a real float32 prototype h[0 .. P-1] (h[i] = 0 for i >= P), Q = ceil(P / L) taps per phase, and the
 * input x[n], int16 pairs, x[n] = 0 for n < 0.  The taps are quantised as the reference quantises its own (xlating.c:486-487):
 *     c[i] = (int16) trunc(h[i] * 32768)      the product in float32 (exact: a power-of-two scaling), truncation toward zero
 * Nothing is clamped: a prototype with a tap that is not finite, or whose truncated value falls outside [-32768, 32767], is refused
 * with -ERANGE (h = 1.0 is refused, h = -1.0 is accepted).  Output sample m = 0, 1, 2, .. is
 *     t = m * M,  n_m = t / L,  p_m = t % L
 *     s = sum over q < Q of c[p_m + q * L] * x[n_m - q]        an exact integer, re and im separately
 *     y[m] = sat16(s >> 15)                                    arithmetic shift (floor), then saturation to [-32768, 32767]
 * which is the reference's saturate_to_int16(temp >> 15) (xlating.c:92-140).  |s| can reach Q * 2^30 = 2^40: the sum is exact in 64
 * bits; a stream whose every phase has sum_q |c| <= 65535 fits 32 bits (65535 * 32768 < 2^31), and the implementation sums those in
 * 32 bits.  The result is the same number either way, and because it is exact no order of summation is prescribed.  y[m] exists once
 * x[n_m] has been consumed: after N consumed samples a stream has produced ceil(N * L / M) outputs, as in the float bank.  The
 * outputs are BIT-IDENTICAL under any split of the input into feeds and in any company of other streams.
 *
 * Distance to the unquantised filter, derived: |c - h * 2^15| < 1 per tap and |x| <= 2^15, so |s - 2^15 sum h x| < Q * 2^15, and the
 * floor of the shift adds less than one: for an output that did not saturate, |y[m] - sum_q h[p_m + q L] x[n_m - q]| < Q + 1 output
 * LSBs.
 */
#ifndef XLATING_RESAMPLE_Q15_H_
#define XLATING_RESAMPLE_Q15_H_

#include <stddef.h>
#include <stdint.h>

#include "xlating_resample.h" /* XLATING_RESAMPLE_MAX_L, XLATING_RESAMPLE_MAX_Q: the limits are the float bank's */

#ifdef __cplusplus
extern "C" {
#endif

typedef struct xlating_resample_q15_bank xlating_resample_q15_bank;

/* The quantiser add itself uses, host only: out[i] = c[i] for i < len.  0; -EINVAL: taps == NULL, out == NULL or len == 0; -ERANGE
 * as above (out[] is then unspecified). */
int xlating_resample_q15_quantize(const float *taps, size_t len, int16_t *out);

/* 0 on success.  -EINVAL: out == NULL.  -ENODEV (with a "<3>" line on stderr): no usable HIP device -- there is no CPU path.
 * -ENOMEM. */
int xlating_resample_q15_bank_create(xlating_resample_q15_bank **out);

/* A new stream whose sample 0 is the first sample it is fed and whose history before it is zero.  Returns its stream id >= 0 (ids of
 * removed streams are reused), -ENOMEM, or, both decided before the device is touched, -EINVAL (xlating_resample_bank_add's list:
 * L == 0, M == 0, gcd(L, M) != 1, L > XLATING_RESAMPLE_MAX_L, taps == NULL, taps_len == 0,
 * ceil(taps_len / L) > XLATING_RESAMPLE_MAX_Q, M >= 2^31) and then -ERANGE (a tap that does not quantise).  The taps are copied.
 * Streams whose (L, M, float taps) are equal byte for byte share one device table (int16, phase-major, [p][q]), which lives as long
 * as one of them does. */
int xlating_resample_q15_bank_add(xlating_resample_q15_bank *b, uint32_t L, uint32_t M, const float *taps, size_t taps_len);
int xlating_resample_q15_bank_remove(xlating_resample_q15_bank *b, int stream_id);

/* Advance n streams at once: stream ids[i] consumes counts[i] complex samples (int16 pairs, 4 bytes each), read in place from device
 * address dev_samples[i] (4-byte aligned).  Everything else -- host arrays, one id at most once, counts up to 2^30, nothing consumed
 * by a refused call, stream order, -ENOMEM and -EIO -- as xlating_resample_bank_feed_device. */
int xlating_resample_q15_bank_feed_device(xlating_resample_q15_bank *b, size_t n, const int *ids, const void *const *dev_samples,
                                          const size_t *counts, void *hip_stream);

/* The outputs the LATEST feed produced for this stream (n_complex == 0 and a NULL pointer when it produced none or did not name
 * the stream): a device row of int16 pairs, written in the order of the feed's stream, valid until the next feed. */
int xlating_resample_q15_bank_output_device(xlating_resample_q15_bank *b, int stream_id, const void **d_out, size_t *n_complex);

/* One device-to-host copy of every stream's latest outputs into pinned memory; waits for it.  output_host then gives a stream's
 * part (interleaved re, im), valid until the next fetch or destroy. */
int xlating_resample_q15_bank_fetch(xlating_resample_q15_bank *b);
int xlating_resample_q15_bank_output_host(xlating_resample_q15_bank *b, int stream_id, const int16_t **out, size_t *n_complex);

/* Outputs since the stream was added (host state, no waiting); 0 for an id that is not live. */
uint64_t xlating_resample_q15_bank_produced(const xlating_resample_q15_bank *b, int stream_id);

/* What the latest feed issued: kernel launches and memory copies.  A feed that consumes anything is the ragged resampling launch,
 * the carry launch (left out when no stream of the feed has more than one tap per phase) and one table copy. */
int xlating_resample_q15_bank_last_feed_ops(const xlating_resample_q15_bank *b, unsigned *launches, unsigned *copies);

/* Live streams, device tap tables and their bytes (2 per tap: L * Q * 2 a table). */
int xlating_resample_q15_bank_stats(const xlating_resample_q15_bank *b, unsigned *streams, unsigned *tables, size_t *table_bytes);

void xlating_resample_q15_bank_destroy(xlating_resample_q15_bank *b);

#ifdef __cplusplus
}
#endif

#endif /* XLATING_RESAMPLE_Q15_H_ */
