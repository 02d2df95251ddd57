/* xl_spectrum_wide_plan.h -- what the two-level spectrogram transform (widths above 8192: xl_spectrum_wide.hip) is told by the host:
 * pure integer rules, plain C, no HIP (compiled by gcc in tests/test_spectrogram_wide_cpu.py, and with the sanitizers by
 * tests/c/spectrum_wide_plan_sweep.c).  The only place that decides them; the kernels and xl_spectrum.cpp call these functions.
 *
 * Transform length: a power-of-two W runs at N = W, any other W runs Bluestein at the power of two N = L >= 2 W - 1.  Widths
 * 8193 .. 1048576 give N = 2^14 .. 2^21.
 * Split: N = N1 * N2, input index n = n1 * N2 + j2, output bin k = k1 + N1 * k2 (n1, k1 < N1; j2, k2 < N2).  N2 = min(8192, N / 64): a
 * contiguous row of N2 points fits a workgroup's LDS, and N1 is 64, 128 or 256, so that a workgroup's pack of 4096 / N1 adjacent columns
 * reads runs of 64, 32 or 16 samples.
 * Scratch: one float2 buffer [transform][k1][j2]; a span's transforms go through it max(1, scratch bytes / (8 N)) at a time.
 * Bin order of the plain path: the row pass leaves bin k1 + N1 * k2 at position k1 * N2 + k2 of the transform's N slots, and the row
 * maxima stay in that order; the finishing pass reads column j's bin -- the half swap first -- from that position.  (The Bluestein path's
 * last pass is a column pass: its bins come out in natural order, position = bin.) */
#ifndef XL_SPECTRUM_WIDE_PLAN_H_
#define XL_SPECTRUM_WIDE_PLAN_H_

#include <stdint.h>

#if defined(__HIPCC__)
#define XL_SPECW_FN static inline __host__ __device__
#else
#define XL_SPECW_FN static inline
#endif

#define XL_SPECW_MIN_W 8193u      /* narrower widths are the one-workgroup kernels' (xl_spectrum.hip) */
#define XL_SPECW_MAX_W 1048576u   /* XLATING_SPECTRUM_MAX_WIDE_WIDTH */
#define XL_SPECW_PACK_POINTS 4096u /* points a column pass's workgroup holds: 32 KiB of float2 */
#define XL_SPECW_MAX_N2 8192u
#define XL_SPECW_SCRATCH_DEFAULT ((uint64_t)64 << 20)
/* the split rule, as a constant expression for the kernels' template arguments and as xl_specw_plan's */
#define XL_SPECW_N2(N) ((N) / 64u < XL_SPECW_MAX_N2 ? (N) / 64u : XL_SPECW_MAX_N2)

typedef struct {
  uint32_t W, N, N1, N2;
  uint32_t pack; /* adjacent columns per workgroup of a column pass: XL_SPECW_PACK_POINTS / N1 */
  uint32_t blue; /* 1: Bluestein at L = N */
} XlSpecWidePlan;

/* N for a width: W itself when a power of two, else the power of two >= 2 W - 1.  W >= 1. */
XL_SPECW_FN uint32_t xl_specw_length(uint32_t W) {
  if ((W & (W - 1u)) == 0u) return W;
  uint32_t L = 1u;
  while ((uint64_t)L < 2ull * W - 1ull) L <<= 1;
  return L;
}

/* 0 and *p filled, or -1 for a width outside XL_SPECW_MIN_W .. XL_SPECW_MAX_W (then *p is left alone) */
XL_SPECW_FN int xl_specw_plan(uint32_t W, XlSpecWidePlan *p) {
  if (W < XL_SPECW_MIN_W || W > XL_SPECW_MAX_W) return -1;
  p->W = W;
  p->N = xl_specw_length(W);
  p->blue = p->N != W;
  p->N2 = XL_SPECW_N2(p->N);
  p->N1 = p->N / p->N2;
  p->pack = XL_SPECW_PACK_POINTS / p->N1;
  return 0;
}

/* transforms per pass through a scratch buffer of `scratch_bytes` (8 N bytes each), at least one */
XL_SPECW_FN uint64_t xl_specw_chunk(uint64_t scratch_bytes, uint32_t N) {
  const uint64_t c = scratch_bytes / (8ull * N);
  return c > 0 ? c : 1;
}

/* plain path: where bin k (< N = W) sits among the transform's N positions */
XL_SPECW_FN uint32_t xl_specw_bin_pos(uint32_t N1, uint32_t N2, uint32_t k) { return (k % N1) * N2 + k / N1; }

/* spectrogram.c:150-158: the bin that lands in column j after the halves of half = W / 2 are swapped (an odd W's last bin in place) */
XL_SPECW_FN uint32_t xl_specw_shift_src(uint32_t j, uint32_t W) {
  const uint32_t half = W / 2u;
  return j < half ? j + half : (j < 2u * half ? j - half : j);
}

/* plain path: the position the finishing pass reads for column j (< W): the half swap first, then (k1, k2) */
XL_SPECW_FN uint32_t xl_specw_col_pos(uint32_t N1, uint32_t N2, uint32_t W, uint32_t j) {
  return xl_specw_bin_pos(N1, N2, xl_specw_shift_src(j, W));
}

#endif /* XL_SPECTRUM_WIDE_PLAN_H_ */
