/* A plain C caller of the serve object, built with gcc against include/xlating_serve.h, xlating_wire.h and xlating_batch.h alone:
 *   serve_demo <out_dir> <cf32|cs16> [overlap]
 * One band of 192000 Hz in cu8, blocks of 65536 bytes.  Two wire requests with FILE destinations -- 48000 Hz (the rate divides: the
 * engine's row) and 44100 Hz (it does not: D = 4, then 147 / 160 in the resampler bank) -- six blocks of a ramp, a flush, and the
 * sizes of the two files, which must be the samples the rates promise: prints "<id> <bytes>" per client and 0, or the code of the
 * first call that fails. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>

#include "xlating_batch.h"
#include "xlating_serve.h"
#include "xlating_wire.h"

#define BAND_RATE 192000u
#define BAND_FREQ 460100000u
#define BLOCK 65536u
#define NBLOCKS 6

int main(int argc, char **argv) {
  if (argc < 3) return 2;
  const int cs16 = strcmp(argv[2], "cs16") == 0;
  xlating_serve_config cfg;
  memset(&cfg, 0, sizeof(cfg));
  cfg.band_sampling_rate = BAND_RATE, cfg.input_format = XL_FMT_CU8, cfg.buffer_size = BLOCK, cfg.group_blocks = 2, cfg.device = -1;
  cfg.family = cs16 ? XL_SERVE_CS16 : XL_SERVE_CF32, cfg.native = 1, cfg.any_rate = 1, cfg.base_path = argv[1];
  cfg.overlap = argc > 3 && strcmp(argv[3], "overlap") == 0;
  xlating_serve *s = NULL;
  int code = xlating_serve_create(&cfg, &s);
  const uint32_t rates[2] = {48000u, 44100u};
  int ids[2] = {-1, -1};
  for (int i = 0; i < 2 && code == 0; ++i) {
    const xlating_wire_request req = {BAND_FREQ + 12000u * (uint32_t)i, rates[i], BAND_FREQ, XL_WIRE_DESTINATION_FILE};
    uint8_t msg[15], resp[7];
    size_t rlen = 0;
    uint8_t status = 1;
    uint32_t details = 0;
    if (xlating_wire_build_request(&req, msg) != sizeof(msg)) code = -1;
    if (code == 0) code = xlating_serve_request(s, msg, sizeof(msg), -1, resp, &rlen, &ids[i]);
    if (code == 0 && (xlating_wire_parse_response(resp, rlen, &status, &details) != 0 || status != XL_WIRE_STATUS_SUCCESS ||
                      details != (uint32_t)ids[i]))
      code = -2;
  }
  uint8_t *iq = malloc((size_t)2 * BLOCK);
  if (iq == NULL) code = code ? code : -3;
  for (int k = 0; k < NBLOCKS / 2 && code == 0; ++k) {  /* two blocks per call */
    for (size_t j = 0; j < (size_t)2 * BLOCK; ++j) iq[j] = (uint8_t)((j * 7u + (size_t)k * 13u) >> 3);
    code = xlating_serve_blocks_host(s, iq, BLOCK, 2);
  }
  if (code == 0) code = xlating_serve_flush(s);
  int dropped[2];
  if (code == 0 && xlating_serve_dropped(s, dropped, 2) != 0) code = -4;
  if (code == 0 && xlating_batch_num_clients(xlating_serve_engine(s)) != 2) code = -5;
  xlating_serve_destroy(s);
  /* NBLOCKS * BLOCK / 2 input samples: / 4 at 48000; / 4 * 147 / 160, rounded up, at 44100 */
  const long in = (long)NBLOCKS * BLOCK / 2, esz = cs16 ? 4 : 8;
  const long want[2] = {in / 4 * esz, (in / 4 * 147 + 159) / 160 * esz};
  for (int i = 0; i < 2 && code == 0; ++i) {
    char path[4096];
    struct stat sb;
    snprintf(path, sizeof(path), "%s/%d.%s", argv[1], ids[i], cs16 ? "cs16" : "cf32");
    if (stat(path, &sb) != 0) code = -6;
    else printf("%d %ld\n", ids[i], (long)sb.st_size);
    if (code == 0 && (long)sb.st_size != want[i]) code = -7;
  }
  free(iq);
  printf("%d\n", code);
  return code == 0 ? 0 : 1;
}
