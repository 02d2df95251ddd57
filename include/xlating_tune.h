/*
 * The tuner bank: a stage behind the batch engine (and behind the resampler bank) that rotates MANY independent complex float32
 * streams, each by its own phase-continuous frequency shift that may be changed between any two feeds and may ramp linearly (a Doppler
 * correction that follows a pass).  One feed advances every stream with ONE kernel launch and ONE table copy, however many streams it
 * carries.  Plain C ABI, no HIP header: streams are void *.  Library: lib/libxlating_tune.so.
 *
 * The rule (csrc/xl_tune_rule.h holds the text the kernel and the tests' sweep both compile).  All phase arithmetic is 64-bit and
 * modular; 2^64 is one turn.  A stream's state is P (uint64, the phase of its next sample), F (int64, turns * 2^64 per sample) and
 * R (int64, turns * 2^64 per sample^2).  Sample j = 0, 1, .. of a feed has phase
 *     phi_j = P + j F + (j (j - 1) / 2) R   mod 2^64
 * and leaves as
 *     re = fl(fl(xr c) - fl(xi s)),  im = fl(fl(xr s) + fl(xi c)),  (c, s) = xlating_tune_cs(phi_j >> 32)
 * in float32, nothing fused; after a feed of n samples P <- P + n F + (n (n - 1) / 2) R and F <- F + n R, both wrapping.  A positive F
 * moves the spectrum up.  xlating_tune_cs approximates cos and sin of 2 pi p / 2^32 by integer quadrant reduction and float32
 * polynomials: exactly 0 and +-1 at the quarter turns, cs(p + 2^30) = (-s, c) and cs(-p) = (c, -s) bit for bit as values, and within
 * the error DESIGN section 3.11 records (below 2^-22) of libm's double functions.  Integer phases and a fixed order of float32
 * operations: the outputs are BIT-IDENTICAL under any split of a stream into feeds and in any company of other streams.
 */
#ifndef XLATING_TUNE_H_
#define XLATING_TUNE_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct xlating_tune_bank xlating_tune_bank;

/* 0 on success.  -EINVAL: out == NULL.  -ENODEV (with a "<3>" line on stderr): no usable HIP device -- there is no CPU path.
 * -ENOMEM, -EIO. */
int xlating_tune_bank_create(xlating_tune_bank **out);

/* A new stream whose sample 0 is the first sample it is fed, with the state (P, F, R).  Returns its stream id >= 0 (ids of removed
 * streams are reused), -EINVAL (b == NULL) or -ENOMEM.  Host state only: the device is not touched. */
int xlating_tune_bank_add(xlating_tune_bank *b, uint64_t P, int64_t F, int64_t R);
int xlating_tune_bank_remove(xlating_tune_bank *b, int stream_id);

/* New steps from the next sample fed on.  P is untouched: the phase is continuous.  0, -EINVAL (not a live stream). */
int xlating_tune_bank_set(xlating_tune_bank *b, int stream_id, int64_t F, int64_t R);

/* Advance n streams at once: stream ids[i] rotates counts[i] complex float32 samples, read in place from the 8-byte aligned device
 * address dev_samples[i] and never written.  ids, dev_samples and counts are HOST arrays, read before the call returns.  An id may
 * appear at most once per call and must be a live stream, and a count may not exceed 2^30: -EINVAL otherwise, and nothing is
 * consumed.  counts[i] == 0 is allowed.  Stream-ordered on hip_stream (NULL: the default stream): the buffers stay valid until that
 * stream has passed this call's work, the call waits for nothing, consecutive feeds may use different streams (each is ordered
 * behind the previous feed's work).  0, or a negative errno: -ENOMEM when the output arena cannot be held (nothing is consumed), -EIO
 * after a HIP failure (the bank is then unusable). */
int xlating_tune_bank_feed_device(xlating_tune_bank *b, size_t n, const int *ids, const void *const *dev_samples, const size_t *counts,
                                  void *hip_stream);

/* The row the LATEST feed produced for this stream (n_complex == 0 and a NULL pointer when it consumed nothing or did not name the
 * stream): complex float32 in the bank's own arena, 8-byte aligned, written in the order of the feed's stream, valid until the next
 * feed. */
int xlating_tune_bank_output_device(xlating_tune_bank *b, int stream_id, const void **d_out, size_t *n_complex);

/* The stream's state as the next sample fed will see it, and the samples it has consumed since it was added.  Host state: does not
 * wait.  Any output may be NULL.  0, -EINVAL. */
int xlating_tune_bank_state(const xlating_tune_bank *b, int stream_id, uint64_t *P, int64_t *F, int64_t *R, uint64_t *consumed);

/* What the latest feed issued: kernel launches and memory copies -- one ragged launch and one table copy when it consumed anything,
 * none when it consumed nothing or was refused. */
int xlating_tune_bank_last_feed_ops(const xlating_tune_bank *b, unsigned *launches, unsigned *copies);

void xlating_tune_bank_destroy(xlating_tune_bank *b);

/* The rule, for tests and for consumers that undo or repeat a rotation on the host: cos and sin of 2 pi p / 2^32 as the kernel
 * computes them. */
void xlating_tune_cs(uint32_t p, float *c, float *s);
/* F = llrint(ldexp(shift_hz / rate, 64)) and R = llrint(ldexp(ramp_hz_per_s / rate / rate, 64)), in double.  0, or -EINVAL unless both
 * quotients are finite and below 0.5 in magnitude (nothing is written then). */
int xlating_tune_from_hz(double shift_hz, double ramp_hz_per_s, double rate, int64_t *F, int64_t *R);
/* The samples of a row one workgroup of the launch rotates. */
unsigned xlating_tune_chunk_samples(void);

#ifdef __cplusplus
}
#endif

#endif /* XLATING_TUNE_H_ */
