/*
 * Streaming spectrogram on the GPU: the waterfall of the reference's sdr_spectrogram (src/spectrogram/spectrogram.c:84-168) as an
 * object that consumes I/Q samples in pieces of any length, from host memory or in place from device memory -- for example the
 * blocks the batch engine already holds (xlating_batch_process_device).  Plain C ABI, no HIP header: streams are void *.
 * Library: lib/libxlating_spectrum.so.
 *
 * Rows: row r covers stream samples r * sampling_rate ..; it is the bin-wise maximum of the power spectra of its
 * F = sampling_rate / width transforms of `width` consecutive samples (the S = sampling_rate % width samples after them are skipped,
 * never transformed).  Power = re^2 + im^2 + 1e-20f with re, im the forward DFT's components times 1.0f / width; a row's value is
 * 10 log10f(max), the two halves of half = width / 2 bins swapped so that DC is in the middle (an odd width's last bin stays last),
 * and its pixel is (int)(dB + 255) clamped to [0, 255] (png_util.c:53-63).
 * A row is complete once its F-th transform is in (its skipped tail need not have been fed).  Any split of the same input into feeds
 * gives bit-identical rows.
 */
#ifndef XLATING_SPECTRUM_H_
#define XLATING_SPECTRUM_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* sample formats: the values of XL_FMT_CU8 / XL_FMT_CS16 / XL_FMT_CF32 of xlating_batch.h (cs8 is not a spectrogram format) */
enum { XLATING_SPECTRUM_CU8 = 0, XLATING_SPECTRUM_CS16 = 2, XLATING_SPECTRUM_CF32 = 3 };

#define XLATING_SPECTRUM_MAX_WIDTH 8192
#define XLATING_SPECTRUM_MAX_WIDE_WIDTH 1048576

typedef struct xlating_spectrum xlating_spectrum;

/* 0 on success.  -EINVAL: width <= 0, width > XLATING_SPECTRUM_MAX_WIDTH, sampling_rate == 0, width > sampling_rate, an unknown
 * format or out == NULL.  -ENODEV (with a "<3>" line on stderr): no usable HIP device -- there is no CPU path.  -ENOMEM. */
int xlating_spectrum_create(uint32_t sampling_rate, int width, int format, xlating_spectrum **out);

/* The same with the cap at XLATING_SPECTRUM_MAX_WIDE_WIDTH: the same checks in the same order with the same return values, every
 * -EINVAL decided before the device is touched.  The object is fed, read and destroyed with the functions below.  Up to
 * XLATING_SPECTRUM_MAX_WIDTH it is the very object xlating_spectrum_create builds (same kernels, bit-identical rows).  A wider one
 * runs each transform in two levels across workgroups, through a scratch buffer in device memory (64 MiB), and keeps `width`-sized
 * row buffers: at width 1048576 about 160 MiB of device and 60 MiB of pinned host memory.  Everything above about rows, their
 * completion and splits holds. */
int xlating_spectrum_create_wide(uint32_t sampling_rate, int width, int format, xlating_spectrum **out);

/* Consume n samples (complex samples: n * 2 bytes of cu8, n * 4 of cs16, n * 8 of cf32) from host memory.  The caller's buffer is
 * copied before the call returns.  0, or a negative errno (-EIO after a HIP failure; the object is then unusable). */
int xlating_spectrum_feed_host(xlating_spectrum *s, const void *samples, size_t n);

/* The same from device memory, read in place and stream-ordered on `hip_stream` (NULL: the default stream), like
 * xlating_batch_process_device: the buffer must stay valid until that stream has passed this call's work; the call does not wait
 * for it.  Consecutive feeds may use different streams: each is ordered behind the previous feed's work. */
int xlating_spectrum_feed_device(xlating_spectrum *s, const void *dev_samples, size_t n, void *hip_stream);

/* Copy up to max_rows completed rows, oldest first, and drop them from the object: `width` floats (dB) per row to db and `width`
 * bytes (pixels) per row to pixels; either pointer may be NULL.  Waits for the feeds' work.  Returns the number of rows copied
 * (0 when none is complete), or a negative errno.  Rows are never lost or reordered: un-taken rows accumulate and the object's
 * row store GROWS to hold them (a feed fails with -ENOMEM only if that growth cannot be allocated, and then consumes nothing);
 * a long-lived caller takes rows regularly. */
int xlating_spectrum_take_rows(xlating_spectrum *s, float *db, uint8_t *pixels, size_t max_rows);

void xlating_spectrum_destroy(xlating_spectrum *s);

/*
 * The spectrum bank: MANY independent streams of one common width and sample format, each with its own sampling_rate (for example
 * every client of a batch engine at its output rate), all advanced by ONE feed call whose number of kernel launches and copies does
 * not depend on how many streams it carries.  Per stream the rows are, bit for bit, the rows an xlating_spectrum of the same
 * (sampling_rate, width, format) produces from the same samples: everything above about rows, their completion and splits holds per
 * stream.
 */
typedef struct xlating_spectrum_bank xlating_spectrum_bank;

/* width (1 .. XLATING_SPECTRUM_MAX_WIDTH; wider: xlating_spectrum_bank_create_wide) and format as xlating_spectrum_create.  0, -EINVAL, -ENODEV (with a "<3>" line on stderr), -ENOMEM. */
int xlating_spectrum_bank_create(int width, int format, xlating_spectrum_bank **out);

/* The same with the cap at XLATING_SPECTRUM_MAX_WIDE_WIDTH: the same checks in the same order with the same return values, every
 * -EINVAL decided before the device is touched (*out is then left alone).  The bank is added to, fed, read and destroyed with the
 * functions below.  Up to XLATING_SPECTRUM_MAX_WIDTH it is the very bank xlating_spectrum_bank_create builds (same kernels,
 * bit-identical rows).  A wider one runs each transform in two levels across workgroups, the transforms of ALL streams of a feed in
 * one ragged list that goes through a scratch buffer in device memory a chunk at a time; per stream its rows are, bit for bit, those
 * of an xlating_spectrum_create_wide object of the same (sampling_rate, width, format) from the same samples -- under any split into
 * feeds, in any company of other streams, with streams added and removed between feeds.
 * Memory of a bank of `width` W (s: bytes per complex sample, 2 / 4 / 8):
 *   per stream, device: W * s of carry and two row slots of W * 4 -- W * (s + 8) bytes: 768 KB for cf32 at W = 48000, 16 MiB at
 *     W = 1048576.  The arrays grow by doubling as streams are added, from as many streams as 64 MiB hold (at most 64);
 *   per stream, host: its completed rows that have not been taken, W * 5 bytes each;
 *   per bank, device: the scratch (64 MiB), the tables (8 .. 40 bytes per bin), and a staging for completed rows of at most 32 MiB (or
 *     one row), allocated when the first row completes;
 *   per bank, pinned host: one batch of at most the staging's size EACH per round whose rows are on their way, kept for reuse: a
 *     feed that the staging cuts into k rounds holds k of them (not bounded in total).
 * An empty bank of width 1048576 holds about 72 MiB of device memory and no pinned row memory. */
int xlating_spectrum_bank_create_wide(int width, int format, xlating_spectrum_bank **out);

/* A new stream whose sample 0 is the first sample it is fed.  Returns its stream id >= 0 (ids of removed streams are reused), -EINVAL
 * (sampling_rate == 0 or < width) or -ENOMEM.  Streams may be added and removed between any two feeds; the per-stream device state
 * grows as streams are added (growing, and removing a stream that has consumed samples, wait for the feeds' work).
 * remove drops the stream's un-taken rows. */
int xlating_spectrum_bank_add(xlating_spectrum_bank *b, uint32_t sampling_rate);
int xlating_spectrum_bank_remove(xlating_spectrum_bank *b, int stream_id);

/* Advance n streams at once: stream ids[i] consumes counts[i] complex samples, read in place from device address dev_samples[i].
 * ids, dev_samples and counts are HOST arrays, read before the call returns.  An id may appear at most once per call and must be a
 * live stream, and a count may not exceed 2^30: -EINVAL otherwise, and nothing is consumed.  counts[i] == 0 is allowed.
 * Stream-ordered on hip_stream (NULL: the default stream) exactly like xlating_spectrum_feed_device: the buffers stay valid until
 * that stream has passed this call's work, the call does not wait, consecutive feeds may use different streams.
 * 0, or a negative errno (-EIO after a HIP failure, -ENOMEM; the bank is then unusable). */
int xlating_spectrum_bank_feed_device(xlating_spectrum_bank *b, size_t n, const int *ids, const void *const *dev_samples,
                                      const size_t *counts, void *hip_stream);

/* Per stream, like xlating_spectrum_take_rows: up to max_rows completed rows, oldest first; rows are never lost or reordered.  Waits
 * for the feeds' work only when rows of this stream are still on their way. */
int xlating_spectrum_bank_take_rows(xlating_spectrum_bank *b, int stream_id, float *db, uint8_t *pixels, size_t max_rows);
/* Without waiting for the device: the rows of that stream whose work has been queued and that have not been taken. */
int xlating_spectrum_bank_rows_pending(const xlating_spectrum_bank *b, int stream_id);

/* What the latest feed issued: kernel launches and memory copies (for tests, logs and benchmarks).  A feed is a few launches (carry
 * appends, one ragged transform launch, carry saves, one finishing launch when rows complete) and one to three copies, times the
 * number of rounds: a feed that takes a stream through more rows than the bank keeps row slots per stream (2 .. 16 by width) is cut
 * into rounds.
 * A width above XLATING_SPECTRUM_MAX_WIDTH: the transform launch becomes two launches (a power-of-two width) or three (any other) per
 * CHUNK of the round's transforms, a chunk being as many transforms as the scratch holds (64 MiB / (8 N) with N the transform length:
 * the width if a power of two, else the power of two >= 2 width - 1); and a round also ends when the rows it completes would exceed
 * the staging.  So the launch count of a feed depends on how many transforms it runs, how many rows it completes and how many
 * transforms the scratch holds -- not on how the transforms are spread over streams. */
int xlating_spectrum_bank_last_feed_ops(const xlating_spectrum_bank *b, unsigned *launches, unsigned *copies);

void xlating_spectrum_bank_destroy(xlating_spectrum_bank *b);

#ifdef __cplusplus
}
#endif

#endif /* XLATING_SPECTRUM_H_ */
