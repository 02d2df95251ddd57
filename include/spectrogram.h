/*
 * Drop-in for the reference's sdr_spectrogram library (src/spectrogram/spectrogram.h): the same request fields, in the same order,
 * and the same two functions, computed on the GPU (lib/libxlating_spectrum.so).  No FFTW or libpng: a caller that sets the six
 * request fields and calls spectrogram_main compiles unchanged against this header.
 *
 * spectrogram_main: reads a cu8 / cs16 / cf32 recording (plain, or gzip when the name contains ".gz") and writes its waterfall as an
 * 8-bit grayscale PNG, one row per sampling_rate samples (see xlating_spectrum.h for a row).  Returns 0, or:
 *   -EINVAL  input_file or output_file NULL, width <= 0, sampling_rate == 0, width > sampling_rate,
 *            width > 8192 (deviation: the reference has no limit; spectrogram_main_wide serves widths up to 1048576), or a file shorter
 *            than one row (deviation: no image is written);
 *   -1       an unknown data_format, an input that cannot be opened, or an output that cannot be written;
 *   -ENODEV  no usable HIP device; -ENOMEM / -EIO from the device.
 * Arguments are checked and the input is opened before the device is touched.  An fftw_flags value other than "FFTW_MEASURE" /
 * "FFTW_ESTIMATE" is reported on stderr and otherwise ignored (there is no plan to tune).  Plain files are counted in 64 bits;
 * gzip files by their ISIZE trailer (uncompressed size mod 2^32), as the reference does.
 * spectrogram_main_wide: spectrogram_main with the width's cap at 1048576 (XLATING_SPECTRUM_MAX_WIDE_WIDTH of xlating_spectrum.h)
 * instead of 8192: the same checks in the same order, the same return values, the same image for every width both accept.  It is an
 * entry of its own so that a caller of spectrogram_main sees no change; xl_private cannot carry the choice (callers do not zero it).
 * spectrogram_sighandler: a signal handler that stops spectrogram_main after the row it is on (the image then has fewer rows).
 */
#ifndef SPECTROGRAM_H_
#define SPECTROGRAM_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
  uint32_t sampling_rate;
  int width;
  char *data_format;
  char *input_file;
  char *output_file;
  char *fftw_flags;

  void *xl_private[6]; /* reserved: spectrogram_main neither reads nor needs it */
} spectrogram;

int spectrogram_main(spectrogram *req);

int spectrogram_main_wide(spectrogram *req);

void spectrogram_sighandler(int signum);

#ifdef __cplusplus
}
#endif

#endif /* SPECTROGRAM_H_ */
