// xl_spectrum_bank.h -- the spectrum bank's launches (xl_spectrum_bank.hip) as its host side (xl_spectrum_bank.cpp) calls them.
// Internal to libxlating_spectrum.so; the public interface is include/xlating_spectrum.h.
#ifndef XL_SPECTRUM_BANK_INTERNAL_H_
#define XL_SPECTRUM_BANK_INTERNAL_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

// One run of transforms of one stream inside the ragged launch: transforms g0 .. of the stream (g = row g / F, k = g % F, samples
// from stream index (g / F) * sr + (g % F) * W), read from `src`, which holds stream samples base .. (the feed's buffer, or the
// stream's carry for a completed straddling transform).  The launch's transform t belongs to the entry with tsum <= t < next tsum.
// The row maximum of row r goes to row slot slot0 + r % slots.
struct XlBankRun {
  const void *src;
  int64_t base;
  int64_t g0;
  uint32_t tsum;
  uint32_t F;
  uint32_t sr;
  uint32_t slot0;
};

// One stream's carry work: before the transforms, `app` samples from src[0 ..] go to carry[stream][have ..]; after them, save_n
// samples from src[save_off ..] go to carry[stream][0 ..].
struct XlBankCarry {
  const void *src;
  uint32_t stream;
  uint32_t have;
  uint32_t app;
  uint32_t save_off;
  uint32_t save_n;
  uint32_t pad;
};

struct XlBankArgs {
  const XlBankRun *runs;  // device
  uint32_t nruns;
  uint32_t T;             // transforms of the launch: the last run's tsum + its count
  uint32_t W;
  uint32_t slots;         // row slots per stream
  uint32_t *rowmax;       // [stream * slots + slot][W], float bits, zero between rows
  const float2 *tw, *chirp, *bspec;  // as XlSpecArgs
  float norm;
};

// N: the transform length (W for a power of two, else the Bluestein L); fmt: XLF_CU8 / XLF_CS16 / XLF_CF32.  0 or a hipError_t.
int xl_bank_launch(const XlBankArgs &a, uint32_t N, bool bluestein, int fmt, hipStream_t st);

// The carries of n streams (ops: device): save == false the appends, save == true the new partial transforms.  ssz: bytes per complex
// sample; carry: [stream][W] samples.
int xl_bank_carry(const XlBankCarry *ops, uint32_t n, void *carry, uint32_t W, uint32_t ssz, bool save, hipStream_t st);

// Rows list[0 .. nrows) (global row slots, device): 10 log10f, half swap, pixel of row i to db[i * W ..] / px[i * W ..]; clears the maxima.
int xl_bank_finish(const uint32_t *list, uint32_t nrows, uint32_t *rowmax, float *db, uint8_t *px, uint32_t W, hipStream_t st);

// ---- widths above XL_SPEC_MAX_W (xl_spectrum_bank_wide.hip; the rules are xl_spectrum_wide_plan.h's and xl_spectrum_bank_plan.h's)
// One chunk of a round's ragged transform list through the two-level transform: transforms t0 .. t0 + Tc - 1 of the round's a.T, transform
// t0 + t in slot t of `scratch` ([transform][k1][j2], N float2 each; Tc at most what it holds).  Two launches (plain) or three
// (Bluestein), stream-ordered.  Bins are left as XlSpecWideArgs says: a plain width's bin k1 + N1 k2 at position k1 * N2 + k2 of its row slot.
struct XlBankWideArgs {
  XlBankArgs a;        // tw: the N-point table (the twiddles between the two levels); bspec: Bluestein, in [k1][k2] order
  float2 *scratch;
  const float2 *tw1;   // N1-point twiddles
  const float2 *tw2;   // N2-point twiddles
  uint32_t N, N1, N2;
  uint32_t t0, Tc;
};
int xl_bankw_launch(const XlBankWideArgs &w, bool bluestein, int fmt, hipStream_t st);
static inline unsigned xl_bankw_passes(bool bluestein) { return bluestein ? 3u : 2u; }  // launches of one xl_bankw_launch

// xl_bank_carry on a grid over (stream, piece of XL_BANKW_CARRY_PIECE samples of the carry)
int xl_bankw_carry(const XlBankCarry *ops, uint32_t n, void *carry, uint32_t W, uint32_t ssz, bool save, hipStream_t st);

// xl_bank_finish with the wide object's arithmetic (xl_specw_finish's: permuted for a plain width)
int xl_bankw_finish(const uint32_t *list, uint32_t nrows, uint32_t *rowmax, float *db, uint8_t *px, uint32_t W, uint32_t N1, uint32_t N2,
                    bool permuted, hipStream_t st);

#endif
