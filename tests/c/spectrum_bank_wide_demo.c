/* A plain C caller of the spectrum bank's wide entry, built with gcc against include/xlating_spectrum.h alone: create a bank of a width
 * up to XLATING_SPECTRUM_MAX_WIDE_WIDTH with xlating_spectrum_bank_create_wide (and show what xlating_spectrum_bank_create answers
 * to the same width), add a stream per rate given, feed nothing, take nothing, destroy -- a wide bank is driven by the very calls of
 * tests/c/spectrum_bank_demo.c.  Prints the default entry's code and the code of the wide path's first call that fails (or 0). */
#include <stdio.h>
#include <stdlib.h>

#include "xlating_spectrum.h"

int main(int argc, char **argv) {
  if (argc < 3) {
    fprintf(stderr, "usage: %s <width> <format> [sampling_rate ...]\n", argv[0]);
    return 2;
  }
  const int width = atoi(argv[1]), format = atoi(argv[2]);
  xlating_spectrum_bank *narrow = NULL, *bank = NULL;
  const int narrow_code = xlating_spectrum_bank_create(width, format, &narrow); /* -EINVAL above XLATING_SPECTRUM_MAX_WIDTH */
  xlating_spectrum_bank_destroy(narrow);
  int code = xlating_spectrum_bank_create_wide(width, format, &bank);
  for (int i = 3; i < argc && code == 0; ++i) {
    int id = xlating_spectrum_bank_add(bank, (uint32_t)atol(argv[i]));
    if (id < 0) code = id;
  }
  if (code == 0) {
    unsigned launches = 0, copies = 0;
    code = xlating_spectrum_bank_feed_device(bank, 0, NULL, NULL, NULL, NULL);
    if (code == 0) code = xlating_spectrum_bank_last_feed_ops(bank, &launches, &copies);
    if (code == 0 && argc > 3) code = xlating_spectrum_bank_rows_pending(bank, 0);
    if (code == 0 && argc > 3) code = xlating_spectrum_bank_take_rows(bank, 0, NULL, NULL, 1);
    if (code == 0 && argc > 3) code = xlating_spectrum_bank_remove(bank, 0);
  }
  xlating_spectrum_bank_destroy(bank);
  printf("%d %d\n", narrow_code, code);
  return code == 0 ? 0 : 1;
}
