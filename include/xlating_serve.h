/*
 * include/xlating_serve.h -- the whole loop in one object: one band on one GPU, from a client's wire request to the bytes in its file
 * or socket.
 *
 * What a server's sdr_callback does with the pieces of this project -- admission (xlating_wire.h), the batch engine (xlating_batch.h),
 * the second stage of clients whose rate does not divide the band rate (xlating_resample.h, xlating_resample_q15.h), delivery
 * (xlating_delivery.h) and the writer threads (xlating_sinks.h) -- is done here, in C, behind about ten calls:
 *
 *     xlating_serve_create(&cfg, &s);
 *     xlating_serve_request(s, msg, len, fd, response, &rlen, &id);     // per client message; send `response` back
 *     xlating_serve_blocks_host(s, iq, input_len, nblocks);             // per device callback (or _blocks_device)
 *     n = xlating_serve_dropped(s, ids, cap);                           // clients whose peer failed or fell behind: close them
 *     xlating_serve_remove(s, id);                                      // a client that left
 *     xlating_serve_flush(s); xlating_serve_destroy(s);
 *
 * Per blocks call: the engine call in the configured mode; one resampler-bank feed for the fractional clients (pointers from
 * xlating_batch_outputs_device); one tuner-bank feed for the clients of xlating_serve_set_tune, if there are any; one meter launch for the clients of xlating_serve_set_squelch, if there are any; ONE delivery batch
 * holding the final row of every client (key: the client id; 8 bytes a sample in the cf32 family, 4 in the cs16 family and in
 * XL_SERVE_CF32_AS_CS16), which is one launch and one device-to-host copy of exactly those
 * bytes.  xlating_batch_fetch and the banks' _fetch are never called: a fractional client's engine row never crosses to the host, and after an XL_MODE_Q15 call only
 * the int16 pairs do.  With overlap = 0 the call waits for that copy and queues the rows to the sinks before it returns; with
 * overlap = 1 it queues the PREVIOUS call's rows, whose copy ran beside this call's launches, and the latest call's rows are queued by
 * the next call, by xlating_serve_flush or by xlating_serve_remove of a client that has some.  Per client the bytes written are
 * exactly the stream of the engine (an integer-rate client) or of the bank fed from the engine (a fractional client): the object adds
 * no arithmetic -- in XL_SERVE_CF32_AS_CS16 that stream narrowed by the delivery's one rule, sample by sample.
 *
 * Ordering: the feed and the pack launch run on a stream of the object's own, behind an event recorded behind the engine call
 * (xlating_batch_record_event); the next engine call is ordered behind an event recorded behind the pack launch (a device call waits
 * for it on its stream, xlating_batch_process_device_group_ev; a host call waits for it on the host, as it does for the previous
 * call), so the rows are read before they are rewritten; the bank's next feed is on the same stream as the pack launch before it.
 *
 * Memory: the delivery object's, delivery_slots x the largest call's rows on the device and pinned (xlating_delivery.h).
 * Not thread-safe: one thread at a time per object.
 */
#ifndef SDR_SERVER_AMD_XLATING_SERVE_H_
#define SDR_SERVER_AMD_XLATING_SERVE_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct xlating_serve_t xlating_serve;
struct xlating_batch_t;

/* XL_SERVE_CF32_AS_CS16: the cf32 family in everything (the engine's mode, `native`, every input format, cf32 included, the float
 * resampler bank) except the delivery, which narrows each row to cs16 on its way to the host (xlating_delivery_pack_device_cs16: round
 * to nearest even of y * 32768, saturated; the Q15 family's scale without its truncating arithmetic or its slower call).  Files are
 * <id>.cs16[.gz], 4 bytes a sample cross to the host and pass through the sinks; xlating_serve_outputs_device still gives the cf32 rows
 * on the device (a spectrum bank fed from them is a "cf32" bank). */
enum { XL_SERVE_CF32 = 0, XL_SERVE_CS16 = 1, XL_SERVE_CF32_AS_CS16 = 2 };

typedef struct {
  uint32_t band_sampling_rate;
  int input_format;        /* XL_FMT_* (xlating_batch.h) */
  uint32_t buffer_size;    /* bytes of a cu8 block: the engine's max_input_buffer_length */
  unsigned group_blocks;   /* most blocks per call, 1 .. 64 (0: 1) */
  int device;              /* HIP device ordinal, or -1 for the calling thread's current device */
  int family;              /* XL_SERVE_CF32 | XL_SERVE_CS16 (XL_MODE_Q15 + the Q15 resampler bank) | XL_SERVE_CF32_AS_CS16 */
  int native;              /* cf32 family and XL_SERVE_CF32_AS_CS16: XL_MODE_NATIVE instead of XL_MODE_OPTIMIZED */
  int any_rate;            /* admit through xlating_wire_admit_any_rate */
  uint32_t lpf_cutoff_rate; /* (0: 5, the reference's default) */
  const char *base_path;   /* FILE destinations: <base_path>/<id>.<cf32|cs16>[.gz]; copied */
  int use_gzip;
  unsigned writer_threads; /* (0: 2) */
  size_t queue_bytes;      /* per client, allocated when its sink is attached; a row that does not fit drops the client
                            * (0: 8 calls of a client at a quarter of the band rate = 8 x group_blocks x (buffer_size / 8 + 64) x 8 bytes,
                            * x 4 bytes for XL_SERVE_CF32_AS_CS16;
                            * set it from the rates you serve: 1024 clients cost 1024 x queue_bytes of host memory) */
  unsigned delivery_slots; /* 2 .. 16 (0: 2) */
  int overlap;             /* 0: a block's rows reach the sinks before its call returns; 1: during the next call / flush */
} xlating_serve_config;

/* 0, -EINVAL, -ENODEV, -ENOMEM, -EIO. */
int xlating_serve_create(const xlating_serve_config *cfg, xlating_serve **out);

/* One client message as it came off the socket: header + request.  The call parses it, admits it against the band of the clients
 * running (0 if none), designs the taps, adds the engine client and, for a rate that does not divide, the second stage, and attaches
 * the sink: FILE -> <base_path>/<id>.<cf32|cs16>[.gz]; SOCKET -> socket_fd, owned by the caller.  It writes the response bytes the
 * reference's server would send: SUCCESS + id, FAILURE + INVALID_REQUEST / OUT_OF_BAND_FREQ, or FAILURE + INTERNAL_ERROR after
 * undoing what it had added.  Returns 0 admitted (*client_id set), 1 refused (a response was written); -EAGAIN / -EPROTO from the wire
 * parsers (also -EPROTO: a message that is no request), -EINVAL: no response was written. */
int xlating_serve_request(xlating_serve *s, const uint8_t *msg, size_t len, int socket_fd, uint8_t response[7], size_t *response_len,
                          int *client_id);
/* A client that left: what it is still owed (overlap = 1) is queued first, then its queue is flushed and its file closed.  0, -EINVAL. */
int xlating_serve_remove(xlating_serve *s, int client_id);

/* nblocks consecutive blocks of input_len scalar elements each, back to back (xlating_batch_process_*_group).  0, or the engine's,
 * the bank's or the delivery's error. */
int xlating_serve_blocks_host(xlating_serve *s, const void *input, size_t input_len, unsigned nblocks);
int xlating_serve_blocks_device(xlating_serve *s, const void *d_input, size_t input_len, unsigned nblocks, void *hip_stream);
/* Everything processed so far has reached the OS, or its sink has failed. */
int xlating_serve_flush(xlating_serve *s);

/* The rows the latest call delivered, at each client's FINAL rate: an integer-rate client's engine row, a fractional client's bank
 * row -- the arguments of xlating_spectrum_bank_feed_device.  Valid until the next blocks call; the feed that reads them must be
 * ordered by the caller before it (e.g. synchronised).  0, -EINVAL (an id that is not a client: nothing is filled). */
int xlating_serve_outputs_device(xlating_serve *s, size_t n, const int *client_ids, const void **d_rows, size_t *n_complex);
/* Clients removed because their sink failed or overflowed (engine, bank and sinks), each reported once; returns how many were stored. */
size_t xlating_serve_dropped(xlating_serve *s, int *client_ids, size_t cap);
/* The sinks' totals since creation (xlating_sinks_stats): bytes handed to the OS / zlib, and rows refused because a sink had failed. */
int xlating_serve_sink_stats(xlating_serve *s, uint64_t *bytes_written, uint64_t *blocks_dropped);
/* The engine: options, describe, timing.  Clients are added and removed through this object only. */
struct xlating_batch_t *xlating_serve_engine(xlating_serve *s);
/* What the latest blocks call issued behind the engine call: kernel launches (the bank's feed, the pack), memory copies, and the
 * bytes of the device-to-host copy. */
int xlating_serve_last_ops(const xlating_serve *s, unsigned *launches_after_engine, unsigned *copies_after_engine, uint64_t *d2h_bytes);

/* ---- XL_SERVE_CF32_AS_CS16 only (every other family: -EINVAL): a power-of-two gain per client and a level meter.
 * A cf32 stream has no scale of its own, and a deep decimation leaves a weak signal few of the 16 bits: each client's row may be
 * delivered as clamp(rne(y * 2^(15 + g))) with its own g in -48 .. 48 (xlating_delivery_pack_device_cs16_gain), and every delivered
 * row's level comes back with it: peak_bits (the bit pattern of the largest magnitude before the gain), clipped (floats where the
 * clamp acted) and nans.  The object packs through that call exactly when levels are enabled or some client's gain is not 0 or is
 * automatic: still one pack launch and one device-to-host copy, one more memory operation in xlating_serve_last_ops (the zeroing of
 * the level table) and 12 bytes a non-empty row more in d2h_bytes.  Otherwise a call is, launch for launch and byte for byte, what it
 * is without these functions. */
/* The client's gain from the next blocks call on; default 0.  Ends automatic gain for the client.  0, -EINVAL (another family, no such
 * client, a gain outside -48 .. 48). */
int xlating_serve_set_gain(xlating_serve *s, int client_id, int gain_log2);
/* Automatic gain on or off (csrc/xl_serve_gain.h holds the policy; turning it off keeps the gain it had reached).  After each call
 * whose rows are queued to the sinks, from the row's level and the gain g it was packed with, with top the exponent such that
 * |peak| * 2^g lies in [2^(top - 1), 2^top): clipped > 0 or top > 0 lowers the gain by max(1, top); a nonzero peak with top <= -3 in
 * each of the last 8 such calls raises it by 1 and the count restarts; silence changes nothing; the gain stays in -48 .. 48.  A
 * constant level ends with |peak| * 2^g in [1/8, 1).  LAG: a new gain holds from the next call that has not been packed yet -- with
 * overlap = 0 a step in level at call N is answered from call N + 1 on, with overlap = 1 (call N's rows are queued during call N + 1,
 * behind its pack) from call N + 2 on; the calls between clip, and are counted.  0, -EINVAL. */
int xlating_serve_set_auto_gain(xlating_serve *s, int client_id, int on);
/* Levels without any gain: every call packs through the gain call (all gains 0 deliver the bytes of the plain rule).  0, -EINVAL. */
int xlating_serve_enable_levels(xlating_serve *s, int on);
/* The level of each client's row in the latest call whose rows have been QUEUED TO THE SINKS (with overlap = 1 the call before the
 * latest, until a flush), the gain that row was packed with, and the client's clipped floats since it joined.  Any output array may be
 * NULL.  Zeros until such a call was delivered through the gain call.  0, -EINVAL (another family; an id that is not a client:
 * nothing is filled). */
int xlating_serve_levels(xlating_serve *s, size_t n, const int *client_ids, uint32_t *peak_bits, uint32_t *clipped, uint32_t *nans,
                         int8_t *gain_log2, uint64_t *clipped_total);
/* The client's latest gain changes, at most 64 and at most cap, oldest first, whether made by xlating_serve_set_gain or by the
 * policy: from sample first_sample[i] of the client's delivered stream (4 bytes each in its file) the gain is gain_log2[i]; before the
 * first change it is 0.  A consumer undoes the gain exactly: y = int16 * 2^-(15 + g).  Returns the number of entries written, or
 * -EINVAL. */
int xlating_serve_gain_log(xlating_serve *s, int client_id, size_t cap, uint64_t *first_sample, int8_t *gain_log2);

/* ---- XL_SERVE_CF32 and XL_SERVE_CF32_AS_CS16 (XL_SERVE_CS16: -EINVAL; a Q15 rotator does not exist): tune a running client.
 * A client's centre frequency is fixed by its request; this moves its signal afterwards, phase-continuously, by a rotation of its
 * FINAL row (xlating_tune.h): from the next blocks call on, sample by sample, y[j] * exp(2 pi i phi_j / 2^64) with phi stepping by
 * shift_hz and ramping by ramp_hz_per_s (Hz per second: a Doppler correction follows a pass without a call per block).  The steps
 * are xlating_tune_from_hz(shift_hz, ramp_hz_per_s, rate) with the client's final rate as the double
 * (double)band_rate * L / ((double)D * M), L = M = 1 for an integer-rate client; a positive shift moves the spectrum up.
 * THE ROTATION FOLLOWS THE CLIENT'S FILTERS: a shift moves the signal inside the band the request bought; it does not widen that band,
 * and what the filters removed stays removed.
 * The first call puts the client into the object's tuner bank (created then) with phase 0, where it stays, at (0, 0) too: its phase
 * is continuous over every later change.  Per blocks call the tuned clients' final rows go through ONE tuner feed (one launch, one
 * table copy, counted in xlating_serve_last_ops) behind the resampler bank's, and everything behind it -- the pack, the gain and the
 * levels, xlating_serve_outputs_device and with it a spectrum bank -- sees the tuned row.  With no client ever tuned a call is, launch
 * for launch and byte for byte, what it is without these functions.
 * 0; -EINVAL: the cs16 family, no such client, or a quotient that is not finite or not below 0.5 in magnitude; the banks' errors. */
int xlating_serve_set_tune(xlating_serve *s, int client_id, double shift_hz, double ramp_hz_per_s);
/* The client's latest changes of rotation, at most 64 and at most cap, oldest first: from sample first_sample[i] of the client's
 * delivered stream the steps are F[i] and R[i] (turns * 2^64 per sample and per sample^2, xlating_tune.h); the phase at the first
 * entry's sample is 0 and continues through every later entry, and before the first entry the stream is not rotated.  With it a
 * consumer knows the exact rotation of every delivered sample.  Returns the number of entries written, or -EINVAL. */
int xlating_serve_tune_log(xlating_serve *s, int client_id, size_t cap, uint64_t *first_sample, int64_t *F, int64_t *R);

/* ---- every family: a squelch per client on a power meter that runs on the device (xlating_meter.h).
 * A monitor of many narrow channels is mostly quiet channels, and without this each of them pays its bytes over PCIe, through its queue
 * and out of its descriptor on every call.  A client with a squelch has the mean power of its FINAL row measured on every blocks call
 * (the resampler's and the tuner's row where those apply; cf32 rows in XL_SERVE_CF32 and XL_SERVE_CF32_AS_CS16, 1.0 = |y| of 1; int16
 * pairs in XL_SERVE_CS16, 1.0 = full scale): ONE meter launch on the object's stream for all squelched clients, behind the tuner feed
 * and in front of the pack, with one table copy and one small copy back (counted in xlating_serve_last_ops).  THE HOST WAITS for that
 * copy, with overlap = 0 and with overlap = 1: the decision is made on the same call's power, before the pack, so a transmission's
 * first call is delivered whole.  The wait covers the engine call's device time -- a fraction of a millisecond per block against a
 * call period of tens of milliseconds at 1024 clients.
 * The policy (csrc/xl_serve_squelch.h), per client and per call with power P, gate closed at first:  P not below open_power (a NaN
 * included) opens the gate;  while it is open, each call with P < close_power counts, the gate closes once more than hang_calls such
 * calls came in a row, and a call with close_power <= P < open_power restarts the count;  a closed gate stays closed under open_power.
 * A call's row is delivered exactly when the gate is open after the step (hang_calls = h still delivers h calls below the close mark).
 * A power that is not finite opens: a broken stream is never hidden.
 * A closed row is packed with length 0: it costs no byte of the image, of the device-to-host copy or of the client's queue, nothing
 * is written to its sink, and to the gain policy, the levels, the gain log and the tune log's sample count it is a call that did not
 * happen (those count DELIVERED samples; the tuner's phase runs on through the withheld ones).  When every row of a call is closed,
 * no pack launch and no device-to-host copy are issued.  xlating_serve_outputs_device still gives every row: a spectrum bank sees the
 * quiet calls too.  With no squelch ever set a call is, launch for launch and byte for byte, what it is without these functions. */
/* The client's squelch from the next blocks call on (mean power, not dB); a client that has one keeps its gate and takes the new
 * marks.  The meter object is created with the first call.  Marks of (0, 0) never close: a level meter without a squelch.
 * 0; -EINVAL: no such client, a mark that is not finite or is negative, open_power < close_power; the meter's errors. */
int xlating_serve_set_squelch(xlating_serve *s, int client_id, double open_power, double close_power, unsigned hang_calls);
/* No squelch from the next blocks call on: every row is delivered again.  0 (also for a client that had none), -EINVAL. */
int xlating_serve_clear_squelch(xlating_serve *s, int client_id);
/* The latest blocks call's figures: each client's mean power, its gate after the step (1: the row was delivered) and the samples
 * withheld from it since it joined.  A client without a squelch reports power 0 and an open gate.  Any output array may be NULL.
 * 0, -EINVAL (an id that is not a client: nothing is filled). */
int xlating_serve_squelch_state(xlating_serve *s, size_t n, const int *client_ids, double *power, uint8_t *open, uint64_t *withheld_samples);
/* The client's latest gate changes, at most 64 and at most cap, oldest first: from sample stream_sample[i] of the stream the client
 * PRODUCED (delivered or not, counted from its first block) the gate is open[i], and at that point the client had been DELIVERED
 * delivered_sample[i] samples -- the index the gain log and the tune log count in.  Before the first entry the gate is open (a client
 * is delivered until its squelch first closes); the entries alternate.  Returns the number of entries written, or -EINVAL. */
int xlating_serve_squelch_log(xlating_serve *s, int client_id, size_t cap, uint64_t *stream_sample, uint64_t *delivered_sample,
                              uint8_t *open);

void xlating_serve_destroy(xlating_serve *s);

#ifdef __cplusplus
}
#endif
#endif /* SDR_SERVER_AMD_XLATING_SERVE_H_ */
