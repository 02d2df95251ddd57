// xl_spectrum.cpp -- the streaming spectrogram (include/xlating_spectrum.h): the state carried across feeds and the launches of
// xl_spectrum.hip.  Reference: src/spectrogram/spectrogram.c:84-168 (one row), iq_file.c (sample formats).
//
// State across feeds: P, the number of samples consumed (row r starts at r * sr; its transform k covers r * sr + k W .. + W); the raw
// samples of the transform that straddles two feeds (at most W - 1, in d_carry, stream-ordered device copies); the per-row maxima in
// a ring of `cap` row slots (d_max, float bits, zero between rows).  A span of a feed is cut by xl_spectrum_cut.h's xl_spec_cut, as the
// bank cuts every stream of its feeds, into: the straddling transform (completed from the carry), the transforms that lie wholly
// inside the span (one launch over the span in place), and the start of the next straddling one (into the carry).  Skipped samples
// are never transformed.  Every row whose F-th transform is in gets one finishing launch (dB, shift, pixel into d_db / d_px of its
// slot) and a copy into the pinned host ring; take_rows waits for the latest feed.
// Any split gives bit-identical rows: every transform sees the same samples and the same code, and max is exact.
// An object of xlating_spectrum_create_wide with a width above 8192 differs in two places only: "launch the transforms of this span"
// goes to the two-level transform (xl_spectrum_wide.hip) in chunks of what its scratch buffer holds, and the finishing launch is
// that file's (a plain width's reads the row pass's bin order).  The cut, the carry, the row ring and the copies are the same.
#include "../../include/xlating_spectrum.h"

#include <errno.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <complex>
#include <new>
#include <vector>

#include "xl_common.h"
#include "xl_device.h"
#include "xl_spectrum.h"
#include "xl_spectrum_core.h"
#include "xl_spectrum_cut.h"
#include "xl_spectrum_wide_plan.h"

struct xlating_spectrum : XlSpecSetup {
  uint32_t sr = 0, F = 0;
  hipStream_t stream = nullptr;  // host feeds
  hipEvent_t last = nullptr;     // behind the latest feed's work
  bool fed = false, broken = false;
  uint8_t *d_carry = nullptr;
  uint32_t cap = 0;
  uint32_t *d_max = nullptr;
  float *d_db = nullptr, *h_db = nullptr;
  uint8_t *d_px = nullptr, *h_px = nullptr;
  int64_t P = 0, rows_finished = 0, rows_taken = 0;
  size_t chunk = 0;  // samples per host staging buffer
  void *h_stage[2] = {nullptr, nullptr}, *d_stage[2] = {nullptr, nullptr};
  hipEvent_t stage_ev[2] = {nullptr, nullptr};
  bool stage_used[2] = {false, false};
  int stage_i = 0;
  // a width above XL_SPEC_MAX_W: the two-level transform's scratch ([transform][k1][j2]) and how many transforms it holds
  bool wide = false;
  float2 *d_scratch = nullptr;
  uint32_t scratch_T = 0;
};

// ---------------------------------------------------------------------------------------------------------- host tables (double)
static void xl_fft_double(std::vector<std::complex<double>> &a) {  // in-place radix-2 forward DFT, size a power of two
  const size_t n = a.size();
  for (size_t i = 1, j = 0; i < n; ++i) {
    size_t bit = n >> 1;
    for (; j & bit; bit >>= 1) j ^= bit;
    j ^= bit;
    if (i < j) std::swap(a[i], a[j]);
  }
  for (size_t len = 2; len <= n; len <<= 1)
    for (size_t i = 0; i < n; i += len)
      for (size_t k = 0; k < len / 2; ++k) {
        const double ang = -2.0 * M_PI * (double)k / (double)len;
        const std::complex<double> w(cos(ang), sin(ang));
        const std::complex<double> u = a[i + k], v = a[i + k + len / 2] * w;
        a[i + k] = u + v;
        a[i + k + len / 2] = u - v;
      }
}

// the same with the twiddles from a table w[m] = exp(-2 pi i m / n): the wide widths' lengths (2^15 .. 2^21), where a cos and a sin per
// butterfly would take seconds
static void xl_fft_double_tab(std::vector<std::complex<double>> &a, const std::vector<std::complex<double>> &w) {
  const size_t n = a.size();
  for (size_t i = 1, j = 0; i < n; ++i) {
    size_t bit = n >> 1;
    for (; j & bit; bit >>= 1) j ^= bit;
    j ^= bit;
    if (i < j) std::swap(a[i], a[j]);
  }
  for (size_t len = 2; len <= n; len <<= 1)
    for (size_t i = 0; i < n; i += len)
      for (size_t k = 0; k < len / 2; ++k) {
        const std::complex<double> u = a[i + k], v = a[i + k + len / 2] * w[k * (n / len)];
        a[i + k] = u + v;
        a[i + k + len / 2] = u - v;
      }
}

static int xl_spec_upload(const std::vector<float2> &h, float2 **d) {
  XL_TRY_RET(hipMalloc(d, sizeof(float2) * h.size()));
  XL_TRY_RET(hipMemcpy(*d, h.data(), sizeof(float2) * h.size(), hipMemcpyHostToDevice));
  return 0;
}

static std::vector<float2> xl_spec_twiddles(uint32_t n) {
  std::vector<float2> tw(n);
  for (uint32_t m = 0; m < n; ++m) {
    const double ang = -2.0 * M_PI * (double)m / (double)n;
    tw[m] = make_float2((float)cos(ang), (float)sin(ang));
  }
  return tw;
}

// A wide width's tables: the N-point twiddles (one rounding each: what the column passes multiply by between the levels), the two
// levels' own twiddles, and for Bluestein the chirp and the chirp filter's spectrum over L = N, times 1 / L, in the order the row pass
// reads it: Bs[k1 + N1 k2] at [k1 * N2 + k2].
static int xl_spec_tables_wide(XlSpecSetup *u) {
  const uint32_t W = u->W, N = u->N, N1 = u->N1, N2 = u->N2;
  std::vector<std::complex<double>> w(N);
  std::vector<float2> tw(N);
  for (uint32_t m = 0; m < N; ++m) {
    const double ang = -2.0 * M_PI * (double)m / (double)N;
    w[m] = std::complex<double>(cos(ang), sin(ang));
    tw[m] = make_float2((float)w[m].real(), (float)w[m].imag());
  }
  int rc = xl_spec_upload(tw, &u->d_tw);
  if (rc == 0) rc = xl_spec_upload(xl_spec_twiddles(N1), &u->d_tw1);
  if (rc == 0) rc = xl_spec_upload(xl_spec_twiddles(N2), &u->d_tw2);
  if (rc != 0 || !u->blue) return rc;
  std::vector<std::complex<double>> b(N, 0.0);
  std::vector<float2> ch(W), bs(N);
  for (uint32_t n = 0; n < W; ++n) {
    const uint64_t q = (uint64_t)n * n % (2ull * W);
    const double ang = -M_PI * (double)q / (double)W;
    const std::complex<double> c(cos(ang), sin(ang));
    ch[n] = make_float2((float)c.real(), (float)c.imag());
    b[n] = std::conj(c);
    if (n > 0) b[N - n] = std::conj(c);
  }
  xl_fft_double_tab(b, w);
  for (uint32_t k = 0; k < N; ++k)
    bs[(size_t)xl_specw_bin_pos(N1, N2, k)] = make_float2((float)(b[k].real() / N), (float)(b[k].imag() / N));
  rc = xl_spec_upload(ch, &u->d_chirp);
  if (rc == 0) rc = xl_spec_upload(bs, &u->d_bspec);
  return rc;
}

static int xl_spec_tables(uint32_t W, uint32_t N, bool blue, float2 **d_tw, float2 **d_chirp, float2 **d_bspec) {
  std::vector<float2> tw(N);
  for (uint32_t m = 0; m < N; ++m) {
    const double ang = -2.0 * M_PI * (double)m / (double)N;
    tw[m] = make_float2((float)cos(ang), (float)sin(ang));
  }
  XL_TRY_RET(hipMalloc(d_tw, sizeof(float2) * N));
  XL_TRY_RET(hipMemcpy(*d_tw, tw.data(), sizeof(float2) * N, hipMemcpyHostToDevice));
  if (!blue) return 0;
  // chirp c[n] = exp(-i pi (n^2 mod 2W) / W); the filter b[m] = conj(c[|m|]) on -(W-1) .. W-1, wrapped into L
  std::vector<std::complex<double>> c(W), b(N, 0.0);
  for (uint32_t n = 0; n < W; ++n) {
    const uint64_t q = (uint64_t)n * n % (2ull * W);
    const double ang = -M_PI * (double)q / (double)W;
    c[n] = std::complex<double>(cos(ang), sin(ang));
  }
  b[0] = std::conj(c[0]);
  for (uint32_t m = 1; m < W; ++m) b[m] = b[N - m] = std::conj(c[m]);
  xl_fft_double(b);
  std::vector<float2> ch(W), bs(N);
  for (uint32_t n = 0; n < W; ++n) ch[n] = make_float2((float)c[n].real(), (float)c[n].imag());
  for (uint32_t m = 0; m < N; ++m) bs[m] = make_float2((float)(b[m].real() / N), (float)(b[m].imag() / N));
  XL_TRY_RET(hipMalloc(d_chirp, sizeof(float2) * W));
  XL_TRY_RET(hipMemcpy(*d_chirp, ch.data(), sizeof(float2) * W, hipMemcpyHostToDevice));
  XL_TRY_RET(hipMalloc(d_bspec, sizeof(float2) * N));
  XL_TRY_RET(hipMemcpy(*d_bspec, bs.data(), sizeof(float2) * N, hipMemcpyHostToDevice));
  return 0;
}

int xl_spec_setup_init(XlSpecSetup *u, int width, int max_width, int format, const char *who) {
  if (width <= 0 || width > max_width ||
      (format != XLATING_SPECTRUM_CU8 && format != XLATING_SPECTRUM_CS16 && format != XLATING_SPECTRUM_CF32))
    return -EINVAL;
  u->device = xl_hip_select_device(-1);
  if (u->device < 0) {
    XL_LOG_ERR("%s: no usable HIP device (%s); there is no CPU path", who, xlating_hip_device_info());
    return -ENODEV;
  }
  u->W = (uint32_t)width, u->fmt = format, u->ssz = xl_bytes_per_sample(format);
  u->blue = (u->W & (u->W - 1u)) != 0;
  u->N = u->W;
  if (u->blue) {
    u->N = 1;
    while (u->N < 2u * u->W - 1u) u->N <<= 1;
  }
  const hipError_t e = hipSetDevice(u->device);
  if (e != hipSuccess) {
    xl_last_hip_error = e;
    XL_LOG_ERR("%s: %s", who, hipGetErrorString(e));
    return xl_errno_of_last_hip_error();
  }
  int rc;
  if (u->W > XL_SPEC_MAX_W) {
    XlSpecWidePlan p;
    if (xl_specw_plan(u->W, &p) != 0 || p.N != u->N) return -EINVAL;
    u->N1 = p.N1, u->N2 = p.N2;
    rc = xl_spec_tables_wide(u);
  } else {
    rc = xl_spec_tables(u->W, u->N, u->blue, &u->d_tw, &u->d_chirp, &u->d_bspec);
  }
  if (rc != 0) xl_spec_setup_free(u);
  return rc;
}

void xl_spec_setup_free(XlSpecSetup *u) {
  if (u->d_tw) (void)hipFree(u->d_tw);
  if (u->d_chirp) (void)hipFree(u->d_chirp);
  if (u->d_bspec) (void)hipFree(u->d_bspec);
  if (u->d_tw1) (void)hipFree(u->d_tw1);
  if (u->d_tw2) (void)hipFree(u->d_tw2);
  u->d_tw = u->d_chirp = u->d_bspec = u->d_tw1 = u->d_tw2 = nullptr;
}

uint64_t xl_specw_scratch_bytes(void) {
  uint64_t scratch = XL_SPECW_SCRATCH_DEFAULT;
  if (const char *v = xl_exp_getenv("XL_EXP_SPEC_SCRATCH")) {  // test knob: the scratch buffer's size in bytes
    const long long b = strtoll(v, nullptr, 10);
    if (b > 0) scratch = (uint64_t)std::min<long long>(b, 1ll << 30);
  }
  return scratch;
}

// ---------------------------------------------------------------------------------------------------------- row ring
static void xl_spec_free_rows(uint32_t *d_max, float *d_db, uint8_t *d_px, float *h_db, uint8_t *h_px) {
  if (d_max) (void)hipFree(d_max);
  if (d_db) (void)hipFree(d_db);
  if (d_px) (void)hipFree(d_px);
  if (h_db) (void)hipHostFree(h_db);
  if (h_px) (void)hipHostFree(h_px);
}

// a ring of `cap` slots, replacing the current one: the un-taken finished rows (host) and the rows in progress (device maxima) move
// to their slots in the new ring.  Everything queued so far has completed (the caller waited for `last`).
static int xl_spec_rows_alloc(xlating_spectrum *s, uint32_t cap) {
  const size_t W = s->W;
  uint32_t *d_max = nullptr;
  float *d_db = nullptr, *h_db = nullptr;
  uint8_t *d_px = nullptr, *h_px = nullptr;
  hipError_t e = hipMalloc(&d_max, sizeof(uint32_t) * W * cap);
  if (e == hipSuccess) e = hipMemset(d_max, 0, sizeof(uint32_t) * W * cap);
  if (e == hipSuccess) e = hipMalloc(&d_db, sizeof(float) * W * cap);
  if (e == hipSuccess) e = hipMalloc(&d_px, W * cap);
  if (e == hipSuccess) e = hipHostMalloc(&h_db, sizeof(float) * W * cap, hipHostMallocDefault);
  if (e == hipSuccess) e = hipHostMalloc(&h_px, W * cap, hipHostMallocDefault);
  if (e == hipSuccess && s->cap > 0) {
    for (int64_t r = s->rows_taken; r < s->rows_finished; ++r) {
      const size_t o = (size_t)(r % s->cap) * W, n = (size_t)(r % cap) * W;
      memcpy(h_db + n, s->h_db + o, sizeof(float) * W);
      memcpy(h_px + n, s->h_px + o, W);
    }
    const int64_t rows_started = s->P > 0 ? (s->P - 1) / s->sr + 1 : 0;
    for (int64_t r = s->rows_finished; r < rows_started && e == hipSuccess; ++r)
      e = hipMemcpy(d_max + (size_t)(r % cap) * W, s->d_max + (size_t)(r % s->cap) * W, sizeof(uint32_t) * W,
                    hipMemcpyDeviceToDevice);
  }
  if (e == hipSuccess) e = hipStreamSynchronize(nullptr);  // (the memset and copies ran on the null stream; the feeds do not)
  if (e != hipSuccess) {
    xl_last_hip_error = e;
    XL_LOG_ERR("spectrum row store of %u rows x %zu bins: %s", cap, W, hipGetErrorString(e));
    xl_spec_free_rows(d_max, d_db, d_px, h_db, h_px);
    return e == hipErrorOutOfMemory ? -ENOMEM : -EIO;
  }
  xl_spec_free_rows(s->d_max, s->d_db, s->d_px, s->h_db, s->h_px);
  s->d_max = d_max, s->d_db = d_db, s->d_px = d_px, s->h_db = h_db, s->h_px = h_px, s->cap = cap;
  return 0;
}

// room for every row from the oldest un-taken one through the row of sample P1 - 1
static int xl_spec_reserve(xlating_spectrum *s, int64_t P1, hipStream_t st) {
  const int64_t need = (P1 - 1) / s->sr - s->rows_taken + 1;
  if (need <= (int64_t)s->cap) return 0;
  if (need > (int64_t)1 << 30) return -ENOMEM;
  uint32_t cap = s->cap * 2;
  while ((int64_t)cap < need) cap *= 2;
  if (s->fed) XL_TRY_RET(hipEventSynchronize(s->last));
  XL_TRY_RET(hipStreamSynchronize(st));  // (this feed's earlier spans: `last` is recorded at the end of a feed)
  return xl_spec_rows_alloc(s, cap);
}

// ---------------------------------------------------------------------------------------------------------- one span
static int xl_spec_launch_t(xlating_spectrum *s, const void *in, int64_t base, int64_t g0, int64_t T, hipStream_t st) {
  XlSpecArgs a;
  a.in = in, a.base = base, a.g0 = g0, a.T = (uint32_t)T, a.F = s->F, a.sr = s->sr, a.W = s->W, a.cap = s->cap;
  a.rowmax = s->d_max, a.tw = s->d_tw, a.chirp = s->d_chirp, a.bspec = s->d_bspec, a.norm = 1.0f / (float)s->W;
  if (!s->wide) {
    XL_TRY_RET(xl_spec_launch(a, s->N, s->blue, s->fmt, st));
    return 0;
  }
  // the two-level transform, as many transforms at a time as the scratch holds (stream order keeps one chunk's passes and the next
  // chunk's apart)
  XlSpecWideArgs w;
  w.scratch = s->d_scratch, w.tw1 = s->d_tw1, w.tw2 = s->d_tw2, w.N = s->N, w.N1 = s->N1, w.N2 = s->N2;
  for (int64_t t = 0; t < T; t += s->scratch_T) {
    w.a = a;
    w.a.g0 = g0 + t, w.a.T = (uint32_t)std::min<int64_t>(s->scratch_T, T - t);
    XL_TRY_RET(xl_specw_launch(w, s->blue, s->fmt, st));
  }
  return 0;
}

// n (0 < n <= XL_SPEC_SPAN_MAX) samples at device address `in`: stream samples P .. P + n - 1
static int xl_spec_span(xlating_spectrum *s, const uint8_t *in, int64_t n, hipStream_t st) {
  const int64_t W = s->W, ssz = s->ssz;
  int rc = xl_spec_reserve(s, s->P + n, st);
  if (rc != 0) return rc;
  const XlSpecCut c = xl_spec_cut(s->sr, W, s->P, n);
  // the transform that straddles P: its first samples are in the carry
  if (c.carry_app > 0)
    XL_TRY_RET(hipMemcpyAsync(s->d_carry + c.carry_have * ssz, in, (size_t)(c.carry_app * ssz), hipMemcpyDeviceToDevice, st));
  if (c.carry_done && (rc = xl_spec_launch_t(s, s->d_carry, c.carry_t0, c.carry_g, 1, st)) != 0) return rc;
  // the transforms wholly inside the span, in place
  if (c.T > 0 && (rc = xl_spec_launch_t(s, in, s->P, c.g_first, c.T, st)) != 0) return rc;
  // the transform that straddles P + n and starts inside the span: its start into the carry
  if (c.save_n > 0)
    XL_TRY_RET(hipMemcpyAsync(s->d_carry, in + c.save_off * ssz, (size_t)(c.save_n * ssz), hipMemcpyDeviceToDevice, st));
  s->P += n;
  // rows whose F-th transform is in: finish, and copy to the host ring
  const int64_t done = c.rows_done;
  for (int64_t r = s->rows_finished; r < done;) {
    const int64_t slot = r % s->cap;
    const int64_t nr = std::min<int64_t>({done - r, (int64_t)s->cap - slot, 65535});
    if (s->wide)
      XL_TRY_RET(xl_specw_finish(s->d_max, s->d_db, s->d_px, s->W, s->N1, s->N2, !s->blue, s->cap, r, (uint32_t)nr, st));
    else
      XL_TRY_RET(xl_spec_finish(s->d_max, s->d_db, s->d_px, s->W, s->cap, r, (uint32_t)nr, st));
    const size_t o = (size_t)slot * W;
    XL_TRY_RET(hipMemcpyAsync(s->h_db + o, s->d_db + o, sizeof(float) * W * nr, hipMemcpyDeviceToHost, st));
    XL_TRY_RET(hipMemcpyAsync(s->h_px + o, s->d_px + o, (size_t)(W * nr), hipMemcpyDeviceToHost, st));
    r += nr;
  }
  s->rows_finished = std::max(s->rows_finished, done);
  return 0;
}

static int xl_spec_begin(xlating_spectrum *s, hipStream_t st) {
  if (s->broken) return -EIO;
  XL_TRY_RET(hipSetDevice(s->device));
  if (s->fed) XL_TRY_RET(hipStreamWaitEvent(st, s->last, 0));
  return 0;
}

static int xl_spec_end(xlating_spectrum *s, hipStream_t st, int rc) {
  if (rc != 0) {
    s->broken = true;
    return rc;
  }
  XL_TRY_RET(hipEventRecord(s->last, st));
  s->fed = true;
  return 0;
}

// ---------------------------------------------------------------------------------------------------------- C API
static int xl_spectrum_create_cap(uint32_t sampling_rate, int width, int max_width, int format, xlating_spectrum **out, const char *who) {
  if (out == nullptr || sampling_rate == 0 || (int64_t)width > (int64_t)sampling_rate) return -EINVAL;
  XlSpecSetup u;
  int rc = xl_spec_setup_init(&u, width, max_width, format, who);
  if (rc == -EINVAL) return rc;  // (as the refusals above: *out is left alone)
  *out = nullptr;
  if (rc != 0) return rc;
  xlating_spectrum *s = new (std::nothrow) xlating_spectrum();
  if (s == nullptr) {
    xl_spec_setup_free(&u);
    return -ENOMEM;
  }
  static_cast<XlSpecSetup &>(*s) = u;
  s->sr = sampling_rate, s->F = sampling_rate / s->W;
  s->chunk = ((size_t)16 << 20) / s->ssz;
  if (const char *e = xl_exp_getenv("XL_EXP_SPEC_CHUNK")) {  // test knob: host staging size in samples
    const long v = strtol(e, nullptr, 10);
    if (v > 0) s->chunk = (size_t)v;
  }
  hipError_t e = hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&s->last, hipEventDisableTiming);
  for (int i = 0; i < 2 && e == hipSuccess; ++i) {
    e = hipEventCreateWithFlags(&s->stage_ev[i], hipEventDisableTiming);
    if (e == hipSuccess) e = hipHostMalloc(&s->h_stage[i], s->chunk * s->ssz, hipHostMallocDefault);
    if (e == hipSuccess) e = hipMalloc(&s->d_stage[i], s->chunk * s->ssz);
  }
  if (e == hipSuccess) e = hipMalloc(&s->d_carry, (size_t)s->W * s->ssz);
  if (s->W > XL_SPEC_MAX_W) {
    s->wide = true;
    s->scratch_T = (uint32_t)xl_specw_chunk(xl_specw_scratch_bytes(), s->N);
    if (e == hipSuccess) e = hipMalloc(&s->d_scratch, sizeof(float2) * (size_t)s->N * s->scratch_T);
  }
  if (e != hipSuccess) {
    xl_last_hip_error = e;
    XL_LOG_ERR("%s: %s", who, hipGetErrorString(e));
    rc = xl_errno_of_last_hip_error();
  }
  // room for the rows one staging buffer can complete, and two more
  if (rc == 0) rc = xl_spec_rows_alloc(s, (uint32_t)std::min<size_t>(s->chunk / s->sr + 3, 1u << 16));
  if (rc != 0) {
    xlating_spectrum_destroy(s);
    return rc;
  }
  *out = s;
  return 0;
}

extern "C" int xlating_spectrum_create(uint32_t sampling_rate, int width, int format, xlating_spectrum **out) {
  return xl_spectrum_create_cap(sampling_rate, width, XLATING_SPECTRUM_MAX_WIDTH, format, out, "xlating_spectrum_create");
}

extern "C" int xlating_spectrum_create_wide(uint32_t sampling_rate, int width, int format, xlating_spectrum **out) {
  return xl_spectrum_create_cap(sampling_rate, width, XLATING_SPECTRUM_MAX_WIDE_WIDTH, format, out, "xlating_spectrum_create_wide");
}

// host samples: through the two pinned staging buffers (or, pinned_src, straight from the caller's pinned memory, which it keeps
// until take_rows has returned) into device staging, one span per chunk
int xl_spectrum_feed_staged(xlating_spectrum *s, const void *samples, size_t n, bool pinned_src) {
  if (s == nullptr || (samples == nullptr && n > 0)) return -EINVAL;
  if (n == 0) return 0;
  hipStream_t st = s->stream;
  int rc = xl_spec_begin(s, st);
  if (rc != 0) return rc;
  const uint8_t *src = static_cast<const uint8_t *>(samples);
  for (size_t i = 0; i < n && rc == 0;) {
    const size_t m = std::min(s->chunk, n - i), bytes = m * s->ssz;
    const int k = s->stage_i;
    hipError_t e = hipSuccess;
    if (s->stage_used[k]) e = hipEventSynchronize(s->stage_ev[k]);
    const void *h = src + i * s->ssz;
    if (e == hipSuccess && !pinned_src) {
      memcpy(s->h_stage[k], h, bytes);
      h = s->h_stage[k];
    }
    if (e == hipSuccess) e = hipMemcpyAsync(s->d_stage[k], h, bytes, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipEventRecord(s->stage_ev[k], st);
    if (e != hipSuccess) {
      xl_last_hip_error = e;
      XL_LOG_ERR("xlating_spectrum_feed_host: %s", hipGetErrorString(e));
      rc = -EIO;
      break;
    }
    s->stage_used[k] = true;
    s->stage_i ^= 1;
    rc = xl_spec_span(s, static_cast<const uint8_t *>(s->d_stage[k]), (int64_t)m, st);
    i += m;
  }
  return xl_spec_end(s, st, rc);
}

extern "C" int xlating_spectrum_feed_host(xlating_spectrum *s, const void *samples, size_t n) {
  return xl_spectrum_feed_staged(s, samples, n, false);
}

extern "C" int xlating_spectrum_feed_device(xlating_spectrum *s, const void *dev_samples, size_t n, void *hip_stream) {
  if (s == nullptr || (dev_samples == nullptr && n > 0)) return -EINVAL;
  if (n == 0) return 0;
  hipStream_t st = static_cast<hipStream_t>(hip_stream);
  int rc = xl_spec_begin(s, st);
  if (rc != 0) return rc;
  const uint8_t *src = static_cast<const uint8_t *>(dev_samples);
  for (size_t i = 0; i < n && rc == 0;) {
    const size_t m = std::min(XL_SPEC_SPAN_MAX, n - i);
    rc = xl_spec_span(s, src + i * s->ssz, (int64_t)m, st);
    i += m;
  }
  return xl_spec_end(s, st, rc);
}

extern "C" int xlating_spectrum_take_rows(xlating_spectrum *s, float *db, uint8_t *pixels, size_t max_rows) {
  if (s == nullptr) return -EINVAL;
  if (s->broken) return -EIO;
  if (s->fed) {
    XL_TRY_RET(hipSetDevice(s->device));
    XL_TRY_RET(hipEventSynchronize(s->last));
  }
  const int64_t n = std::min<int64_t>((int64_t)std::min<size_t>(max_rows, 1u << 30), s->rows_finished - s->rows_taken);
  const size_t W = s->W;
  for (int64_t i = 0; i < n; ++i) {
    const size_t o = (size_t)((s->rows_taken + i) % s->cap) * W;
    if (db != nullptr) memcpy(db + (size_t)i * W, s->h_db + o, sizeof(float) * W);
    if (pixels != nullptr) memcpy(pixels + (size_t)i * W, s->h_px + o, W);
  }
  s->rows_taken += n;
  return (int)n;
}

extern "C" void xlating_spectrum_destroy(xlating_spectrum *s) {
  if (s == nullptr) return;
  (void)hipSetDevice(s->device);
  if (s->fed) (void)hipEventSynchronize(s->last);
  if (s->stream) (void)hipStreamSynchronize(s->stream);
  xl_spec_free_rows(s->d_max, s->d_db, s->d_px, s->h_db, s->h_px);
  for (int i = 0; i < 2; ++i) {
    if (s->h_stage[i]) (void)hipHostFree(s->h_stage[i]);
    if (s->d_stage[i]) (void)hipFree(s->d_stage[i]);
    if (s->stage_ev[i]) (void)hipEventDestroy(s->stage_ev[i]);
  }
  if (s->d_carry) (void)hipFree(s->d_carry);
  if (s->d_scratch) (void)hipFree(s->d_scratch);
  xl_spec_setup_free(s);
  if (s->last) (void)hipEventDestroy(s->last);
  if (s->stream) (void)hipStreamDestroy(s->stream);
  delete s;
}

// spectrogram_main's view (xl_spectrum_core.h)
size_t xl_spectrum_chunk(const xlating_spectrum *s) { return s->chunk; }
uint32_t xl_spectrum_bytes_per_sample(const xlating_spectrum *s) { return s->ssz; }
void *xl_spectrum_pinned_alloc(size_t bytes) {
  void *p = nullptr;
  return hipHostMalloc(&p, bytes, hipHostMallocDefault) == hipSuccess ? p : nullptr;
}
void xl_spectrum_pinned_free(void *p) {
  if (p) (void)hipHostFree(p);
}
