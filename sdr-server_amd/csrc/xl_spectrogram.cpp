// xl_spectrogram.cpp -- spectrogram_main and spectrogram_main_wide (include/spectrogram.h): file -> streaming core -> PNG.  Reference behaviour:
// src/spectrogram/spectrogram.c:55-168 (checks, rows), iq_file.c (formats, sample count), png_util.c (8-bit gray, one row per row).
//
// Order: the request is checked and the input opened and counted before the device is touched, so that every refusal is the
// same without a GPU.  A reader thread fills two pinned buffers in turn (fread / gzread) while the main thread feeds the other to
// the core (one H2D copy, no staging copy), takes the completed rows and streams them into the PNG.  The PNG writer is ours, on
// zlib: signature, IHDR, IDAT chunks of one deflate stream (filter byte 0 per row), IEND; CRCs from zlib's crc32.
#include "../../include/spectrogram.h"

#include <errno.h>
#include <signal.h>
#include <stdio.h>
#include <string.h>
#include <unistd.h>
#include <zlib.h>

#include <condition_variable>
#include <mutex>
#include <thread>
#include <vector>

#include "xl_spectrum_core.h"

extern "C" const char *xl_exp_getenv(const char *name);  // libxlating_hip.so (xl_common.h)

static volatile sig_atomic_t g_spec_exit = 0;

extern "C" void spectrogram_sighandler(int signum) {
  (void)signum;
  static const char msg[] = "spectrogram: signal caught, stopping after the current row\n";
  ssize_t r = write(2, msg, sizeof(msg) - 1);  // (async-signal-safe)
  (void)r;
  g_spec_exit = 1;
}

namespace {

// ------------------------------------------------------------------------------------------------------------------ input
struct Input {
  FILE *fp = nullptr;
  gzFile gz = nullptr;
  uint64_t samples = 0;
  ~Input() {
    if (fp) fclose(fp);
    if (gz) gzclose(gz);
  }
  size_t read(void *dst, size_t bytes) {
    if (fp) return fread(dst, 1, bytes, fp);
    size_t got = 0;
    while (got < bytes) {
      const int r = gzread(gz, static_cast<uint8_t *>(dst) + got, (unsigned)(bytes - got));
      if (r <= 0) break;
      got += (size_t)r;
    }
    return got;
  }
};

// iq_file.c:36-84, 177-197: ".gz" anywhere in the name selects gzip, counted by its ISIZE trailer; plain files by their size
int open_input(const char *name, uint32_t ssz, Input &in) {
  if (strstr(name, ".gz") != nullptr) {
    FILE *fp = fopen(name, "rb");
    if (fp == nullptr) {
      fprintf(stderr, "cannot open input %s: %s\n", name, strerror(errno));
      return -1;
    }
    uint8_t t[4];
    const bool ok = fseek(fp, -4, SEEK_END) == 0 && fread(t, 1, 4, fp) == 4;
    fclose(fp);
    if (!ok) {
      fprintf(stderr, "input %s is too short for a gzip file\n", name);
      return -1;
    }
    const uint32_t isize = (uint32_t)t[0] | ((uint32_t)t[1] << 8) | ((uint32_t)t[2] << 16) | ((uint32_t)t[3] << 24);
    in.gz = gzopen(name, "rb");
    if (in.gz == nullptr) {
      fprintf(stderr, "cannot open input %s: %s\n", name, strerror(errno));
      return -1;
    }
    (void)gzbuffer(in.gz, 128 * 1024);
    in.samples = isize / ssz;
    return 0;
  }
  in.fp = fopen(name, "rb");
  if (in.fp == nullptr) {
    fprintf(stderr, "cannot open input %s: %s\n", name, strerror(errno));
    return -1;
  }
  (void)setvbuf(in.fp, nullptr, _IOFBF, 128 * 1024);
  if (fseeko(in.fp, 0, SEEK_END) != 0) return -1;
  const off_t size = ftello(in.fp);
  rewind(in.fp);
  in.samples = size > 0 ? (uint64_t)size / ssz : 0;  // 64 bits (deviation: the reference's count is uint32_t)
  return 0;
}

// ------------------------------------------------------------------------------------------------------------------ PNG
struct Png {
  FILE *fp = nullptr;
  z_stream z;
  bool zinit = false, failed = false;
  std::vector<uint8_t> out = std::vector<uint8_t>(1 << 16), row;
  ~Png() {
    if (zinit) deflateEnd(&z);
    if (fp) fclose(fp);
  }
  static void be32(uint8_t *p, uint32_t v) {
    p[0] = (uint8_t)(v >> 24), p[1] = (uint8_t)(v >> 16), p[2] = (uint8_t)(v >> 8), p[3] = (uint8_t)v;
  }
  void chunk(const char *type, const uint8_t *data, uint32_t len) {
    uint8_t h[8];
    be32(h, len);
    memcpy(h + 4, type, 4);
    uLong crc = crc32(0L, reinterpret_cast<const Bytef *>(type), 4);
    if (len) crc = crc32(crc, data, len);
    uint8_t c[4];
    be32(c, (uint32_t)crc);
    if (fwrite(h, 1, 8, fp) != 8 || (len && fwrite(data, 1, len, fp) != len) || fwrite(c, 1, 4, fp) != 4) failed = true;
  }
  int begin(uint32_t width, uint32_t height) {
    static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1A, '\n'};
    if (fwrite(sig, 1, 8, fp) != 8) failed = true;
    uint8_t ihdr[13];
    be32(ihdr, width);
    be32(ihdr + 4, height);
    ihdr[8] = 8, ihdr[9] = 0, ihdr[10] = 0, ihdr[11] = 0, ihdr[12] = 0;  // 8-bit gray, deflate, adaptive filters, no interlace
    chunk("IHDR", ihdr, 13);
    memset(&z, 0, sizeof(z));
    if (deflateInit(&z, Z_DEFAULT_COMPRESSION) != Z_OK) return -ENOMEM;
    zinit = true;
    row.resize((size_t)width + 1);
    return 0;
  }
  void pump(int flush) {
    do {
      z.next_out = out.data();
      z.avail_out = (uInt)out.size();
      const int r = deflate(&z, flush);
      if (r == Z_STREAM_ERROR) {
        failed = true;
        return;
      }
      const uint32_t n = (uint32_t)(out.size() - z.avail_out);
      if (n) chunk("IDAT", out.data(), n);
    } while (z.avail_out == 0 || (flush == Z_FINISH && z.avail_in > 0));
  }
  void put_row(const uint8_t *px) {
    row[0] = 0;  // filter type None
    memcpy(row.data() + 1, px, row.size() - 1);
    z.next_in = row.data();
    z.avail_in = (uInt)row.size();
    pump(Z_NO_FLUSH);
  }
  int end() {
    z.next_in = nullptr;
    z.avail_in = 0;
    int r;
    do {
      z.next_out = out.data();
      z.avail_out = (uInt)out.size();
      r = deflate(&z, Z_FINISH);
      const uint32_t n = (uint32_t)(out.size() - z.avail_out);
      if (n) chunk("IDAT", out.data(), n);
    } while (r == Z_OK);
    if (r != Z_STREAM_END) failed = true;
    chunk("IEND", nullptr, 0);
    const int c = fclose(fp);
    fp = nullptr;
    return failed || c != 0 ? -1 : 0;
  }
};

// ------------------------------------------------------------------------------------------------------------------ reader
struct Reader {
  std::mutex mu;
  std::condition_variable cv;
  void *buf[2] = {nullptr, nullptr};
  bool full[2] = {false, false}, last[2] = {false, false}, stop = false;
  size_t n[2] = {0, 0};
};

void reader_loop(Reader &R, Input &in, uint64_t total, size_t chunk, uint32_t ssz) {
  for (int k = 0;; k ^= 1) {
    {
      std::unique_lock<std::mutex> l(R.mu);
      R.cv.wait(l, [&] { return R.stop || !R.full[k]; });
      if (R.stop) return;
    }
    const size_t want = (size_t)std::min<uint64_t>(chunk, total);
    const size_t got = want ? in.read(R.buf[k], want * ssz) / ssz : 0;
    total -= got;
    std::lock_guard<std::mutex> l(R.mu);
    R.n[k] = got;
    R.last[k] = got < want || total == 0;
    R.full[k] = true;
    R.cv.notify_all();
    if (R.last[k]) return;
  }
}

}  // namespace

// spectrogram_main (max_width 8192, xlating_spectrum_create) and spectrogram_main_wide (1048576, xlating_spectrum_create_wide)
static int spectrogram_run(spectrogram *req, const int max_width) {
  // spectrogram.c:56-82, in its order
  if (req->input_file == nullptr) {
    fprintf(stderr, "missing input file (-i)\n");
    return -EINVAL;
  }
  if (req->output_file == nullptr) {
    fprintf(stderr, "missing output file (-o)\n");
    return -EINVAL;
  }
  if (req->width <= 0) {
    fprintf(stderr, "width (-w) must be positive, got %d\n", req->width);
    return -EINVAL;
  }
  if (req->sampling_rate == 0) {
    fprintf(stderr, "sampling rate (-s) must be positive, got %u\n", req->sampling_rate);
    return -EINVAL;
  }
  if ((uint32_t)req->width > req->sampling_rate) {
    fprintf(stderr, "width (-w) %d exceeds the sampling rate %u\n", req->width, req->sampling_rate);
    return -EINVAL;
  }
  if (req->width > max_width) {
    fprintf(stderr, "width (-w) %d exceeds the largest supported width %d\n", req->width, max_width);
    return -EINVAL;
  }
  // iq_file.c:13-33: the format, then the input
  int fmt;
  const char *df = req->data_format != nullptr ? req->data_format : "";
  if (strcmp(df, "cu8") == 0)
    fmt = XLATING_SPECTRUM_CU8;
  else if (strcmp(df, "cs16") == 0)
    fmt = XLATING_SPECTRUM_CS16;
  else if (strcmp(df, "cf32") == 0)
    fmt = XLATING_SPECTRUM_CF32;
  else {
    fprintf(stderr, "unsupported data format: %s\n", df);
    return -1;
  }
  const uint32_t ssz = fmt == XLATING_SPECTRUM_CU8 ? 2u : (fmt == XLATING_SPECTRUM_CS16 ? 4u : 8u);
  Input in;
  if (open_input(req->input_file, ssz, in) != 0) return -1;
  const uint64_t height = in.samples / req->sampling_rate;
  if (height == 0) {
    fprintf(stderr, "input %s holds less than one row (%u samples): no image\n", req->input_file, req->sampling_rate);
    return -EINVAL;
  }
  if (height > 0x7FFFFFFFull) {
    fprintf(stderr, "input %s: %llu rows exceed the PNG limit\n", req->input_file, (unsigned long long)height);
    return -EINVAL;
  }
  // spectrogram.c:44-53
  if (req->fftw_flags != nullptr && strcmp(req->fftw_flags, "FFTW_MEASURE") != 0 && strcmp(req->fftw_flags, "FFTW_ESTIMATE") != 0)
    fprintf(stderr, "unsupported fftw flag: %s. Fallback to FFTW_ESTIMATE\n", req->fftw_flags);

  // the device
  xlating_spectrum *s = nullptr;
  int rc = max_width > XLATING_SPECTRUM_MAX_WIDTH ? xlating_spectrum_create_wide(req->sampling_rate, req->width, fmt, &s)
                                                  : xlating_spectrum_create(req->sampling_rate, req->width, fmt, &s);
  if (rc != 0) return rc;
  Png png;
  png.fp = fopen(req->output_file, "wb");
  if (png.fp == nullptr) {
    fprintf(stderr, "cannot write output %s: %s\n", req->output_file, strerror(errno));
    xlating_spectrum_destroy(s);
    return -1;
  }
  rc = png.begin((uint32_t)req->width, (uint32_t)height);
  const size_t chunk = xl_spectrum_chunk(s);
  const uint64_t total = height * req->sampling_rate;  // the rows' samples; nothing past the last row is read
  Reader R;
  for (int k = 0; k < 2 && rc == 0; ++k)
    if ((R.buf[k] = xl_spectrum_pinned_alloc(chunk * ssz)) == nullptr) rc = -ENOMEM;
  uint64_t written = 0;
  // tools/spectrogram_bench.py's read floor: the same reader loop into the same pinned buffers, no GPU work, no rows
  const char *rf = xl_exp_getenv("XL_EXP_SPEC_READ_FLOOR");
  const bool read_floor = rf != nullptr && strcmp(rf, "1") == 0;
  if (rc == 0) {
    std::thread reader(reader_loop, std::ref(R), std::ref(in), total, chunk, ssz);
    const size_t rows_cap = chunk / req->sampling_rate + 2;
    std::vector<uint8_t> px(rows_cap * (size_t)req->width);
    for (int k = 0;; k ^= 1) {
      size_t n;
      bool last;
      {
        std::unique_lock<std::mutex> l(R.mu);
        R.cv.wait(l, [&] { return R.full[k]; });
        n = R.n[k];
        last = R.last[k];
      }
      if (n > 0 && !read_floor) rc = xl_spectrum_feed_staged(s, R.buf[k], n, true);
      for (int got = read_floor ? 0 : 1; rc == 0 && got > 0;) {  // (take_rows waits for the feed: the buffer is free afterwards)
        got = xlating_spectrum_take_rows(s, nullptr, px.data(), rows_cap);
        if (got < 0) rc = got;
        for (int i = 0; i < got && written < height && !g_spec_exit; ++i, ++written) png.put_row(px.data() + (size_t)i * req->width);
      }
      {
        std::lock_guard<std::mutex> l(R.mu);
        R.full[k] = false;
        if (last || rc != 0 || g_spec_exit || written >= height) R.stop = true;
        R.cv.notify_all();
      }
      if (last || rc != 0 || g_spec_exit || written >= height) break;
    }
    reader.join();
  }
  for (int k = 0; k < 2; ++k) xl_spectrum_pinned_free(R.buf[k]);
  xlating_spectrum_destroy(s);
  if (rc != 0) return rc;
  // (a short or interrupted input leaves fewer rows than IHDR announces, as the reference's png_write_end does)
  return png.end();
}

extern "C" int spectrogram_main(spectrogram *req) { return spectrogram_run(req, XLATING_SPECTRUM_MAX_WIDTH); }

extern "C" int spectrogram_main_wide(spectrogram *req) { return spectrogram_run(req, XLATING_SPECTRUM_MAX_WIDE_WIDTH); }
