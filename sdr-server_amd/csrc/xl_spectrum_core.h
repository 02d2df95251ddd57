// xl_spectrum_core.h -- what spectrogram_main (xl_spectrogram.cpp) uses of the streaming core beyond include/xlating_spectrum.h.
#ifndef XL_SPECTRUM_CORE_H_
#define XL_SPECTRUM_CORE_H_

#include <stddef.h>
#include <stdint.h>

#include "../../include/xlating_spectrum.h"

// feed_host, but straight from the caller's pinned memory when pinned_src (no staging copy): the caller keeps the buffer unchanged
// until xlating_spectrum_take_rows has returned
int xl_spectrum_feed_staged(xlating_spectrum *s, const void *samples, size_t n, bool pinned_src);
size_t xl_spectrum_chunk(const xlating_spectrum *s);  // samples per staging buffer
uint32_t xl_spectrum_bytes_per_sample(const xlating_spectrum *s);
void *xl_spectrum_pinned_alloc(size_t bytes);
void xl_spectrum_pinned_free(void *p);

#endif
