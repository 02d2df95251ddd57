/*
 * The resampler bank: a second stage behind the batch engine that takes MANY independent complex float32 streams, each by its own
 * rational factor L / M, from the rate the engine's integer decimation leaves them at to exactly the rate their client asked for
 * (xlating_wire_admit_any_rate of xlating_wire.h chooses D, L and M).  One feed advances every stream with two kernel launches and
 * one table copy, however many streams it carries.  Plain C ABI, no HIP header: streams are void *.
 * Library: lib/libxlating_resample.so.
 *
 * Per stream: coprime L, M >= 1, a real float32 prototype h[0 .. P-1] (h[i] = 0 for i >= P), Q = ceil(P / L) taps per phase, and the
 * input x[n], complex float32, x[n] = 0 for n < 0.  Output sample m = 0, 1, 2, .. is
 *     t = m * M,  n_m = t / L,  p_m = t % L
 *     y[m] = sum over q = 0 .. Q-1, in this order, of h[p_m + q * L] * x[n_m - q]
 * re and im separately in float32, every term one multiplication and one addition (nothing fused), the sum starting at the first
 * product: upsample by L, filter with h, keep every M-th sample.  y[m] exists once x[n_m] has been consumed: after N consumed
 * samples a stream has produced ceil(N * L / M) outputs.  The order of the sum is fixed, so the outputs are BIT-IDENTICAL under any
 * split of the input into feeds and in any company of other streams.
 */
#ifndef XLATING_RESAMPLE_H_
#define XLATING_RESAMPLE_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define XLATING_RESAMPLE_MAX_L 4096 /* phases */
#define XLATING_RESAMPLE_MAX_Q 1024 /* taps per phase, ceil(taps_len / L) */

typedef struct xlating_resample_bank xlating_resample_bank;

/* 0 on success.  -EINVAL: out == NULL.  -ENODEV (with a "<3>" line on stderr): no usable HIP device -- there is no CPU path.
 * -ENOMEM. */
int xlating_resample_bank_create(xlating_resample_bank **out);

/* A new stream whose sample 0 is the first sample it is fed and whose history before it is zero.  Returns its stream id >= 0 (ids of
 * removed streams are reused), -ENOMEM, or -EINVAL, decided before the device is touched: L == 0, M == 0, gcd(L, M) != 1,
 * L > XLATING_RESAMPLE_MAX_L, taps == NULL, taps_len == 0, ceil(taps_len / L) > XLATING_RESAMPLE_MAX_Q, M >= 2^31.  The taps are
 * copied.  Streams whose (L, M, taps) are equal byte for byte share one device table (phase-major, [p][q]), which lives as long
 * as one of them does.  Streams may be added and removed between any two feeds (growing the per-stream state, and removing a stream
 * that has consumed samples, wait for the feeds' work). */
int xlating_resample_bank_add(xlating_resample_bank *b, uint32_t L, uint32_t M, const float *taps, size_t taps_len);
int xlating_resample_bank_remove(xlating_resample_bank *b, int stream_id);

/* Advance n streams at once: stream ids[i] consumes counts[i] complex float32 samples, read in place from device address
 * dev_samples[i].  ids, dev_samples and counts are HOST arrays, read before the call returns.  An id may appear at most once per
 * call and must be a live stream, and a count may not exceed 2^30: -EINVAL otherwise, and nothing is consumed.  counts[i] == 0 is
 * allowed.  Stream-ordered on hip_stream (NULL: the default stream): the buffers stay valid until that stream has passed this
 * call's work, the call does not wait, consecutive feeds may use different streams (each is ordered behind the previous feed's
 * work).  0, or a negative errno: -ENOMEM when the feed's outputs cannot be held (one stream's new outputs reach 2^31, or the
 * output arena cannot be allocated; nothing is consumed), -EIO after a HIP failure (the bank is then unusable). */
int xlating_resample_bank_feed_device(xlating_resample_bank *b, size_t n, const int *ids, const void *const *dev_samples,
                                      const size_t *counts, void *hip_stream);

/* The outputs the LATEST feed produced for this stream (n_complex == 0 and a NULL pointer when it produced none or did not name
 * the stream): a device row of complex float32, written in the order of the feed's stream, valid until the next feed. */
int xlating_resample_bank_output_device(xlating_resample_bank *b, int stream_id, const void **d_out, size_t *n_complex);

/* One device-to-host copy of every stream's latest outputs into pinned memory; waits for it.  output_host then gives a stream's
 * part (interleaved re, im), valid until the next fetch or destroy. */
int xlating_resample_bank_fetch(xlating_resample_bank *b);
int xlating_resample_bank_output_host(xlating_resample_bank *b, int stream_id, const float **out, size_t *n_complex);

/* Outputs since the stream was added (host state, no waiting); 0 for an id that is not live. */
uint64_t xlating_resample_bank_produced(const xlating_resample_bank *b, int stream_id);

/* What the latest feed issued: kernel launches and memory copies.  A feed that consumes anything is the ragged resampling launch,
 * the carry launch (left out when no stream of the feed has more than one tap per phase) and one table copy. */
int xlating_resample_bank_last_feed_ops(const xlating_resample_bank *b, unsigned *launches, unsigned *copies);

/* Live streams, device tap tables and their bytes. */
int xlating_resample_bank_stats(const xlating_resample_bank *b, unsigned *streams, unsigned *tables, size_t *table_bytes);

void xlating_resample_bank_destroy(xlating_resample_bank *b);

#ifdef __cplusplus
}
#endif

#endif /* XLATING_RESAMPLE_H_ */
