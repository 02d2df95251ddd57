/*
 * The power meter: the mean power of MANY rows of device memory, measured by ONE kernel launch, one table copy and one small copy
 * back, however many rows a measurement carries.  It tells whether a channel holds a signal before any of its bytes cross to the host:
 * the serve object's squelch (xlating_serve_set_squelch) decides on it.  Plain C ABI, no HIP header: streams are void *.
 * Library: lib/libxlating_meter.so.
 *
 * The rule (csrc/xl_meter_rule.h holds the text the kernel compiles, and the bound).  A row is cut into pieces of
 * xlating_meter_piece_samples() = 2048 samples from its first; the last piece may be short.  One workgroup measures one piece in a
 * FIXED order of float32 operations, nothing fused, subnormals kept, and leaves one partial of 8 bytes:
 *   XL_METER_CF32 (float32 pairs, 8-byte aligned): the float32 sum of fl(fl(re re) + fl(im im)), its bits in the partial's low half;
 *                 the row's mean power is the double sum of its partials, in ascending order, divided by its samples: 1.0 = |y| of 1;
 *   XL_METER_CS16 (int16 pairs, 4-byte aligned): the exact integer sum of re re + im im; the row's mean power is
 *                 (double)(the uint64 sum of its partials) / samples / 2^30: 1.0 = full scale.
 * A row of 0 samples has power 0.  A NaN, an infinity or a square that overflows makes the row's power non-finite.  A row's partials
 * and power are BIT-IDENTICAL in any company of other rows.  The rows are read in place and never written.
 */
#ifndef XLATING_METER_H_
#define XLATING_METER_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct xlating_meter xlating_meter;

enum { XL_METER_CF32 = 0, XL_METER_CS16 = 1 };

/* 0 on success.  -EINVAL: out == NULL.  -ENODEV (with a "<3>" line on stderr): no usable HIP device -- there is no CPU path.
 * -ENOMEM, -EIO. */
int xlating_meter_create(xlating_meter **out);

/* Measure n rows of one format: row i is counts[i] samples at the device address dev_rows[i].  dev_rows and counts are HOST arrays,
 * read before the call returns.  A count may not exceed 2^30; counts[i] == 0 is allowed (its address is not looked at).  Stream-ordered
 * on hip_stream (NULL: the default stream): the rows stay valid until that stream has passed this call's work; the call waits for
 * nothing.  ONE measurement is outstanding at a time: the figures are the latest measurement's, and the next may begin once
 * xlating_meter_query has returned 1 or xlating_meter_wait 0.
 * 0, or a negative errno: -EINVAL (m == NULL, a format that is none, a NULL array, a count above 2^30, a misaligned or NULL row)
 * and -EBUSY (the previous measurement has not been seen done) before the device is touched; -ENOMEM (nothing was issued); -EIO
 * after a HIP failure (the object is then unusable). */
int xlating_meter_measure_device(xlating_meter *m, int fmt, size_t n, const void *const *dev_rows, const size_t *counts, void *hip_stream);

/* Whether the latest measurement's figures are on the host: 1 done (also when nothing was ever measured), 0 not yet, -EINVAL, -EIO. */
int xlating_meter_query(xlating_meter *m);
/* Waits for them.  0, -EINVAL, -EIO. */
int xlating_meter_wait(xlating_meter *m);

/* Row i of the latest measurement, which is done: its mean power and its samples.  Either output may be NULL.
 * 0, -EINVAL (no such row), -EBUSY (not done). */
int xlating_meter_power(xlating_meter *m, size_t i, double *mean_power, uint64_t *samples);
/* For tests: row i's partials as the kernel left them, at most cap of them, in ascending order.  Returns how many the row has
 * (ceil(samples / 2048)), -EINVAL or -EBUSY. */
int xlating_meter_partials(xlating_meter *m, size_t i, size_t cap, uint64_t *partials);

/* What the latest measurement issued: kernel launches and memory copies -- one ragged launch, one table copy and one copy back when
 * any row had a sample, none when every row was empty or the call was refused. */
int xlating_meter_last_ops(const xlating_meter *m, unsigned *launches, unsigned *copies);
/* The samples of a row one workgroup of the launch measures. */
unsigned xlating_meter_piece_samples(void);

void xlating_meter_destroy(xlating_meter *m);

#ifdef __cplusplus
}
#endif

#endif /* XLATING_METER_H_ */
