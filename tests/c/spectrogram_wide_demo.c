/* A plain C caller of the spectrogram's wide entry points, built with gcc against include/spectrogram.h and
 * include/xlating_spectrum.h alone: the streaming object of xlating_spectrum_create_wide (created and destroyed; it is fed and read with
 * the functions of the default one), then the file path through spectrogram_main_wide.  Prints both return codes. */
#include <signal.h>
#include <stdio.h>
#include <stdlib.h>

#include "spectrogram.h"
#include "xlating_spectrum.h"

int main(int argc, char **argv) {
  if (argc < 6) {
    fprintf(stderr, "usage: %s <input> <output> <width> <sampling_rate> <format>\n", argv[0]);
    return 2;
  }
  spectrogram spec;
  spec.input_file = argv[1];
  spec.output_file = argv[2];
  spec.width = atoi(argv[3]);
  spec.sampling_rate = (uint32_t)atof(argv[4]);
  spec.data_format = argv[5];
  spec.fftw_flags = "FFTW_MEASURE";
  xlating_spectrum *s = NULL;
  int created = xlating_spectrum_create_wide(spec.sampling_rate, spec.width, XLATING_SPECTRUM_CU8, &s);
  if (created == 0) xlating_spectrum_destroy(s);
  signal(SIGINT, spectrogram_sighandler);
  signal(SIGTERM, spectrogram_sighandler);
  int code = spectrogram_main_wide(&spec);
  printf("%d\n%d\n", created, code);
  return code == 0 ? 0 : 1;
}
