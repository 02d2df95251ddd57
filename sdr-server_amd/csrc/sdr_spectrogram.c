// sdr_spectrogram.c -- the command line of the reference's sdr_spectrogram (same options and defaults) on include/spectrogram.h.
// Exit status: spectrogram_main's return value.
#define _POSIX_C_SOURCE 200809L  // getopt
#include <signal.h>
#include <stdio.h>
#include <stdlib.h>
#include <unistd.h>

#include "../../include/spectrogram.h"

static void usage(const char *argv0) {
  printf("Usage: %s [options]\n", argv0);
  printf("  -h                   this help\n");
  printf("  -w <width>           image width = FFT size, 1 .. 8192 (default: 1024)\n");
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
  int c;
  while ((c = getopt(argc, argv, "hw:s:d:i:o:f:")) != -1) {
    if (c == 'h') {
      usage(argv[0]);
      return EXIT_SUCCESS;
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
  return spectrogram_main(&req);
}
