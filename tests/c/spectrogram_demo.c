/* A plain C caller of the spectrogram drop-in, written the way the reference's own command line uses its library: set the six
 * request fields, install the signal handler, call spectrogram_main.  Built with gcc against include/spectrogram.h alone. */
#include <signal.h>
#include <stdio.h>
#include <stdlib.h>

#include "spectrogram.h"

int main(int argc, char **argv) {
  if (argc < 6) {
    fprintf(stderr, "usage: %s <input> <output> <width> <sampling_rate> <format> [fftw_flags]\n", argv[0]);
    return 2;
  }
  spectrogram spec;
  spec.input_file = argv[1];
  spec.output_file = argv[2];
  spec.width = atoi(argv[3]);
  spec.sampling_rate = (uint32_t)atof(argv[4]);
  spec.data_format = argv[5];
  spec.fftw_flags = argc > 6 ? argv[6] : "FFTW_MEASURE";
  signal(SIGINT, spectrogram_sighandler);
  signal(SIGTERM, spectrogram_sighandler);
  int code = spectrogram_main(&spec);
  printf("%d\n", code);
  return code == 0 ? 0 : 1;
}
