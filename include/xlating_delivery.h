/*
 * include/xlating_delivery.h -- delivery of device rows to the host: one ragged pack launch and one staged copy per batch.
 *
 * After a call of the batch engine (xlating_batch.h) and a feed of a resampler bank (xlating_resample.h, xlating_resample_q15.h) the
 * samples a server owes its clients lie in rows scattered over device memory: rows of the engine's output arena for the clients whose
 * rate divides the band rate, rows of the bank's arena for the others, 8 bytes a sample (cf32) or 4 (cs16).  This object moves exactly
 * those bytes to pinned host memory without waiting for anything:
 *
 *     t = xlating_delivery_pack_device(d, n, keys, dev_rows, bytes, stream);   // one launch on `stream`, one copy behind it
 *     ... the next engine call may be enqueued on `stream` at once: it may overwrite the rows ...
 *     xlating_delivery_wait(d, t);                                             // or _query
 *     xlating_delivery_row(d, t, key, &host, &bytes);                          // for each key
 *     xlating_delivery_release(d, t);
 *
 * pack_device enqueues ONE kernel launch on `hip_stream`, which copies all rows into a dense device staging image of one of the
 * object's `slots`; behind an event, ONE device-to-host copy on the object's own copy stream moves exactly that image into the slot's
 * pinned buffer.  Work enqueued on `hip_stream` after the call may overwrite the sources.  The delivered bytes are the source bytes,
 * bit for bit.  In the image a row begins at the lowest offset behind its predecessor that is congruent to its device address mod 16
 * (csrc/xl_delivery_plan.h): at most 12 bytes of padding a row, which cross to the host with it.
 *
 * No call waits for the device except xlating_delivery_wait -- with the exceptions the banks have: a slot's buffers and the table of
 * rows grow at need (a batch larger than every batch before), which allocates and, for the table, waits for the previous launch.
 * Memory: slots x the largest batch so far, on the device AND pinned on the host; at 1024 clients x 48 kHz of cf32 and 8 blocks of
 * 262144 bytes a call a batch is about 204 MB, so 2 slots hold 0.41 GB of each.
 *
 * A plain C ABI; streams are void * (a hipStream_t; NULL = HIP's default stream).  Not thread-safe: one thread at a time per object.
 */
#ifndef SDR_SERVER_AMD_XLATING_DELIVERY_H_
#define SDR_SERVER_AMD_XLATING_DELIVERY_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct xlating_delivery_t xlating_delivery;

/* slots: batches that may be in flight or unreleased at a time, 2 .. 16.  The object belongs to the calling thread's current device.
 * 0, -EINVAL, -ENODEV (no usable HIP device: a "<3>" line on stderr), -ENOMEM, -EIO. */
int xlating_delivery_create(unsigned slots, xlating_delivery **out);

/* One batch of n rows.  Row i is bytes[i] bytes at device address dev_rows[i]; dev_rows[i] is 4-byte aligned and bytes[i] a multiple
 * of 4 (below 4 GiB); bytes[i] == 0 is allowed, with any pointer.  Row i is tagged keys[i]; keys are unique within the batch.  keys,
 * dev_rows and bytes are host arrays, read before the call returns.  n == 0, or no bytes at all, is an empty batch: a ticket that is
 * done at once, no launch and no copy.
 * Returns a ticket >= 0, or -EINVAL (nothing was done), -EAGAIN (every slot is in flight or unreleased; nothing was done), -ENOMEM
 * (nothing was done), -EIO (a HIP error: the object is broken and refuses further batches). */
int xlating_delivery_pack_device(xlating_delivery *d, size_t n, const int *keys, const void *const *dev_rows, const size_t *bytes,
                                 void *hip_stream);

/* The same batch, NARROWED on its way into the image: row i is n_complex[i] cf32 samples (8 bytes each) at the 8-byte aligned device
 * address dev_rows[i] and is delivered as n_complex[i] cs16 samples (4 bytes each: re, im as int16), at most 0xFFFFFFFC delivered
 * bytes a row; n_complex[i] == 0 is allowed, with any pointer.  Each float y becomes clamp(rne(y * 32768), -32768, 32767), rne = to
 * nearest, ties to even; a NaN becomes 0 (csrc/xl_dlv_narrow.h): the Q15 family's scale, so +1.0 -> 32767 and -1.0 -> -32768.  Still
 * ONE launch (a kernel of its own that reads 8 bytes and writes 4 a sample) and ONE copy, of half the bytes; the sources are not
 * written.  In the image a row begins at the lowest offset behind its predecessor that is congruent to (its device address mod 32) / 2
 * mod 16: at most 12 bytes of padding a row.  xlating_delivery_row gives the narrowed row of 4 * n_complex[i] bytes; tickets, slots,
 * errors and everything else are pack_device's, and plain and narrowing batches may alternate on one object. */
int xlating_delivery_pack_device_cs16(xlating_delivery *d, size_t n, const int *keys, const void *const *dev_rows,
                                      const size_t *n_complex, void *hip_stream);

/* pack_device_cs16 with a GAIN per row and the row's LEVEL recorded.  gain_log2[i] (a host array of n, read before the call returns)
 * is a power of two, -48 .. 48: each float y of row i becomes clamp(rne(y * 2^(15 + gain_log2[i])), -32768, 32767), a NaN 0
 * (csrc/xl_dlv_gain.h: the product is exact, there is one rounding; integer arithmetic on the float's fields).  With every gain 0 the
 * image is byte for byte pack_device_cs16's.  A gain outside -48 .. 48, of an empty row too, is -EINVAL and nothing is done.
 * Per row the launch also reports three uint32 (xlating_delivery_row_level): peak_bits, the bit pattern of the largest magnitude among
 * the row's floats BEFORE the gain, NaNs aside (0 for an empty or all-NaN row, 0x7F800000 for an Inf; as a float it is that magnitude);
 * clipped, the floats where the clamp acted (a rounded magnitude above 32767 for a positive value, above 32768 for a negative; an Inf
 * counts, a NaN does not); nans, the NaN floats.  Integer maxima and sums: bit-identical for a row whatever rows share its batch and in
 * whatever order.  The table of levels lies behind the image at the next 16-byte boundary, 12 bytes a non-empty row, and crosses in the
 * SAME copy: still ONE launch and ONE device-to-host copy.  The table is zeroed on `hip_stream` before the launch by a memset node,
 * which xlating_delivery_last_ops counts among the copies: 1 launch, 3 memory operations (the table of rows up, the zeroing, image
 * and levels down), and d2h_bytes = the image rounded up to 16 + 12 x the non-empty rows.  Tickets, slots, errors and everything else
 * are pack_device's; the three pack calls may alternate on one object. */
int xlating_delivery_pack_device_cs16_gain(xlating_delivery *d, size_t n, const int *keys, const void *const *dev_rows,
                                           const size_t *n_complex, const int8_t *gain_log2, void *hip_stream);
/* After the ticket is done: the level of the row tagged `key` of a pack_device_cs16_gain batch (0, 0, 0 for an empty row).
 * 0, -EINVAL (no such ticket or key, a null pointer), -EBUSY (not done yet), -EIO; -ENODATA: the ticket is one of pack_device or
 * pack_device_cs16, which record no levels. */
int xlating_delivery_row_level(xlating_delivery *d, int ticket, int key, uint32_t *peak_bits, uint32_t *clipped, uint32_t *nans);

/* 1: the ticket's rows are in host memory; 0: not yet.  -EINVAL (no such ticket), -EIO.  Tickets complete in the order given out. */
int xlating_delivery_query(xlating_delivery *d, int ticket);
/* Blocks until they are.  0, -EINVAL, -EIO. */
int xlating_delivery_wait(xlating_delivery *d, int ticket);
/* After the ticket is done: the row tagged `key`, in pinned host memory that stays valid until the ticket is released (*host == NULL
 * and *bytes == 0 for an empty row).  0, -EINVAL (no such ticket or key), -EBUSY (not done yet), -EIO. */
int xlating_delivery_row(xlating_delivery *d, int ticket, int key, const void **host, size_t *bytes);
/* Gives the ticket's slot back, in any order.  0, -EINVAL, -EBUSY (not done yet: nothing waits here), -EIO. */
int xlating_delivery_release(xlating_delivery *d, int ticket);

/* What the latest pack_device or pack_device_cs16 issued: kernel launches (1), memory copies (2: the table of rows up, the image
 * down) and the bytes of the device-to-host copy (the rows as delivered plus their alignment padding); 0, 0, 0 for an empty batch.
 * After pack_device_cs16_gain: 1 launch, 3 memory operations (the zeroing of the level table is one), the bytes stated there. */
int xlating_delivery_last_ops(const xlating_delivery *d, unsigned *launches, unsigned *copies, uint64_t *d2h_bytes);
/* Bytes of the image one workgroup of the pack kernel moves (for tests). */
unsigned xlating_delivery_chunk_bytes(void);

/* Waits for what is in flight and frees everything. */
void xlating_delivery_destroy(xlating_delivery *d);

#ifdef __cplusplus
}
#endif
#endif /* SDR_SERVER_AMD_XLATING_DELIVERY_H_ */
