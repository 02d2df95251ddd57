// sdr_spectrogram.c -- the command line of the reference's sdr_spectrogram (same options and defaults) on include/spectrogram.h, and
// one option of its own: -W, which calls spectrogram_main_wide (widths up to 1048576).
// Exit status: spectrogram_main's (or spectrogram_main_wide's) return value.
#define _POSIX_C_SOURCE 200809L  // getopt
#include <signal.h>
#include <stdio.h>
#include <stdlib.h>
#include <unistd.h>

#include "../../include/spectrogram.h"

static void usage(const char *argv0) {
  printf("Usage: %s [options]\n", argv0);
  printf("  -h                   this help\n");
  printf("  -w <width>           image width = FFT size, 1 .. 8192, with -W 1 .. 1048576 (default: 1024)\n");
  printf("  -W                   accept widths above 8192 (a two-level transform; not an option of the reference)\n");
  printf("  -s <sampling_rate>   samples per image row (default: 48000)\n");
  printf("  -d <data_format>     cu8, cs16 or cf32 (default: cu8)\n");
  printf("  -i <input_file>      I/Q recording; gzip when the name contains \".gz\"\n");
  printf("  -o <output_file>     PNG to write\n");
  printf("  -f <fftw_flags>      FFTW_MEASURE or FFTW_ESTIMATE; accepted for compatibility, no effect (default: FFTW_MEASURE)\n");
}

int main(int argc, char **argv) {
  spectrogram req = {0};
  req.sampling_rate = 48000;
  req.width = 1024;
  req.data_format = "cu8";
  req.fftw_flags = "FFTW_MEASURE";
  int c, wide = 0;
  while ((c = getopt(argc, argv, "hWw:s:d:i:o:f:")) != -1) {
    if (c == 'h') {
      usage(argv[0]);
      return EXIT_SUCCESS;
    } else if (c == 'W') {
      wide = 1;
    } else if (c == 'w') {
      req.width = atoi(optarg);
    } else if (c == 's') {
      req.sampling_rate = (uint32_t)atof(optarg);
    } else if (c == 'd') {
      req.data_format = optarg;
    } else if (c == 'i') {
      req.input_file = optarg;
    } else if (c == 'o') {
      req.output_file = optarg;
    } else if (c == 'f') {
      req.fftw_flags = optarg;
    } else {
      usage(argv[0]);
      return EXIT_FAILURE;
    }
  }
  signal(SIGINT, spectrogram_sighandler);
  signal(SIGHUP, spectrogram_sighandler);
  signal(SIGTERM, spectrogram_sighandler);
  return wide ? spectrogram_main_wide(&req) : spectrogram_main(&req);
}
