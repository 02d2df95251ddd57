/* A plain C caller of the Q15 resampler bank, built with gcc against include/xlating_resample_q15.h alone: quantise a tap, create a
 * bank (or, with "null", ask for one without a place to put it), add a stream per L M pair given with the one-tap prototype {0.5f},
 * feed nothing, read nothing, destroy.  Prints the code of the first call that fails (or 0). */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "xlating_resample_q15.h"

int main(int argc, char **argv) {
  const float half = 0.5f;
  int16_t c = 0;
  xlating_resample_q15_bank *bank = NULL;
  int code, nadded = 0;
  if (xlating_resample_q15_quantize(&half, 1, &c) != 0 || c != 16384) {
    printf("quantize\n");
    return 2;
  }
  if (argc > 1 && strcmp(argv[1], "null") == 0) {
    code = xlating_resample_q15_bank_create(NULL);
    if (code == 0) code = xlating_resample_q15_bank_add(NULL, 1, 1, &half, 1);
    printf("%d\n", code);
    return code == 0 ? 0 : 1;
  }
  code = xlating_resample_q15_bank_create(&bank);
  for (int i = 1; i + 1 < argc && code == 0; i += 2) {
    int id = xlating_resample_q15_bank_add(bank, (uint32_t)atol(argv[i]), (uint32_t)atol(argv[i + 1]), &half, 1);
    if (id < 0) code = id; else nadded++;
  }
  if (code == 0) {
    unsigned launches = 0, copies = 0, streams = 0, tables = 0;
    size_t bytes = 0, n = 0;
    const void *d = NULL;
    const int16_t *h = NULL;
    code = xlating_resample_q15_bank_feed_device(bank, 0, NULL, NULL, NULL, NULL);
    if (code == 0) code = xlating_resample_q15_bank_last_feed_ops(bank, &launches, &copies);
    if (code == 0) code = xlating_resample_q15_bank_stats(bank, &streams, &tables, &bytes);
    if (code == 0) code = xlating_resample_q15_bank_fetch(bank);
    if (code == 0 && nadded > 0) code = xlating_resample_q15_bank_output_device(bank, 0, &d, &n);
    if (code == 0 && nadded > 0) code = xlating_resample_q15_bank_output_host(bank, 0, &h, &n);
    if (code == 0 && nadded > 0) code = xlating_resample_q15_bank_produced(bank, 0) == 0 ? 0 : -1;
    if (code == 0 && nadded > 0) code = xlating_resample_q15_bank_remove(bank, 0);
  }
  xlating_resample_q15_bank_destroy(bank);
  printf("%d\n", code);
  return code == 0 ? 0 : 1;
}
