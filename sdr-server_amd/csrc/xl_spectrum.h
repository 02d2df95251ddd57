// xl_spectrum.h -- the spectrogram's launches (xl_spectrum.hip) as the streaming core (xl_spectrum.cpp) calls them, and what the single
// object and the bank (xl_spectrum_bank.cpp) both set up for a width and a format.
// Internal to libxlating_spectrum.so; the public interface is include/xlating_spectrum.h.
#ifndef XL_SPECTRUM_INTERNAL_H_
#define XL_SPECTRUM_INTERNAL_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

#define XL_SPEC_MAX_W 8192   // the one-workgroup kernels (xl_spectrum.hip); wider: the two-level transform (xl_spectrum_wide.hip)
#define XL_SPEC_MAX_L 16384  // Bluestein length for W = 8191: the power of two >= 2 W - 1
// samples of one stream that one cut (xl_spectrum_cut.h) may take -- a span of the single object's feed, a stream's count in a feed of the
// bank: keeps every in-launch offset within 32 bits
#define XL_SPEC_SPAN_MAX ((size_t)1 << 30)

// One launch: transforms g0 .. g0 + T - 1 of the stream (transform g = row g / F, k = g % F; its samples start at stream index
// (g / F) * sr + (g % F) * W).  `in` holds stream samples base .. : every transform of the launch lies inside it, so that the relative
// offsets fit 32 bits (the core cuts spans to XL_SPEC_SPAN_MAX samples).  Per bin, the power's maximum over a row's transforms goes
// to rowmax[(row % cap) * W + bin] by an unsigned atomicMax on the float's bits (every power is positive, so the bit order is the
// value order, and max is exact: the result does not depend on the work split or on arrival order; a NaN power enters as 0u and so
// loses, as against the reference's fmaxf: xl_spec_max_bits).
struct XlSpecArgs {
  const void *in;
  int64_t base;
  int64_t g0;
  uint32_t T;
  uint32_t F;
  uint32_t sr;
  uint32_t W;
  uint32_t cap;
  uint32_t *rowmax;
  const float2 *tw;     // N-point twiddles exp(-2 pi i m / N), m < N (N = W, or L for Bluestein)
  const float2 *chirp;  // Bluestein: exp(-i pi (n^2 mod 2W) / W), n < W
  const float2 *bspec;  // Bluestein: FFT_L of the chirp filter, times 1 / L
  float norm;           // 1.0f / W (spectrogram.c:104)
};

// N: the transform length (W for a power of two, else the Bluestein L); fmt: XLF_CU8 / XLF_CS16 / XLF_CF32.  0 or a hipError_t.
int xl_spec_launch(const XlSpecArgs &a, uint32_t N, bool bluestein, int fmt, hipStream_t st);

// Rows r0 .. r0 + nrows - 1 (ring slots row % cap): 10 log10f, the half swap (odd W: the last bin stays), the pixel; writes W floats to
// db[slot * W ..] and W bytes to px[slot * W ..], and zeroes the slot's maxima for the row that reuses it.
int xl_spec_finish(uint32_t *rowmax, float *db, uint8_t *px, uint32_t W, uint32_t cap, int64_t r0, uint32_t nrows, hipStream_t st);

// The two-level transform of widths above XL_SPEC_MAX_W (xl_spectrum_wide.hip; the rules are xl_spectrum_wide_plan.h's): the same
// transforms g0 .. g0 + T - 1 of the same stream, T at most what `scratch` holds ([transform][k1][j2], N float2 each).  Two launches
// (plain) or three (Bluestein), stream-ordered, through the scratch.  A plain width leaves bin k1 + N1 k2 of a row at
// rowmax[slot * W + k1 * N2 + k2]; Bluestein leaves bin k at rowmax[slot * W + k].
struct XlSpecWideArgs {
  XlSpecArgs a;          // tw: the N-point table (the twiddles between the two levels); bspec: Bluestein, in [k1][k2] order
  float2 *scratch;
  const float2 *tw1;     // N1-point twiddles
  const float2 *tw2;     // N2-point twiddles
  uint32_t N, N1, N2;
};
int xl_specw_launch(const XlSpecWideArgs &w, bool bluestein, int fmt, hipStream_t st);
// xl_spec_finish for a wide object's rows: permuted (a plain width): column j reads its bin (the half swap first) from the row pass's
// position; the dB is xl_spec_db, as in xl_spec_finish
int xl_specw_finish(uint32_t *rowmax, float *db, uint8_t *px, uint32_t W, uint32_t N1, uint32_t N2, bool permuted, uint32_t cap, int64_t r0,
                    uint32_t nrows, hipStream_t st);

// What a width and a format determine, the same for the single object and the bank: the transform length N (W for a power of two, else
// the Bluestein L) and the tables on `device` (host, double, rounded to float): N-point twiddles, and for Bluestein the chirp and the chirp
// filter's spectrum.
struct XlSpecSetup {
  uint32_t W = 0, N = 0, ssz = 0;  // ssz: bytes per complex sample
  int fmt = 0;
  bool blue = false;
  int device = 0;
  float2 *d_tw = nullptr, *d_chirp = nullptr, *d_bspec = nullptr;
  // a width above XL_SPEC_MAX_W (the wide entries of the single object and of the bank): the split, the two levels' twiddles; d_bspec is
  // in [k1][k2] order
  uint32_t N1 = 0, N2 = 0;
  float2 *d_tw1 = nullptr, *d_tw2 = nullptr;
};

// In this order: -EINVAL for a width outside 1 .. max_width (XLATING_SPECTRUM_MAX_WIDTH, or XLATING_SPECTRUM_MAX_WIDE_WIDTH from
// xlating_spectrum_create_wide and xlating_spectrum_bank_create_wide) or an unknown format, before the device is touched; the
// device, -ENODEV with a "<3>" line that names `who` (the calling function) when there is none; N; the tables (-ENOMEM, -EIO).  The
// device is left current.  A failed init leaves nothing to free.
int xl_spec_setup_init(XlSpecSetup *u, int width, int max_width, int format, const char *who);
void xl_spec_setup_free(XlSpecSetup *u);

// Bytes of the two-level transform's scratch buffer, for the single wide object and the wide bank alike: XL_SPECW_SCRATCH_DEFAULT, or
// what the test knob beside XL_TESTING=1 says (xl_spectrum.cpp; at most 1 GiB).  xl_specw_chunk turns it into transforms.
uint64_t xl_specw_scratch_bytes(void);

#endif
