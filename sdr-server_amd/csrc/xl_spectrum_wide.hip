// xl_spectrum_wide.hip -- the spectrogram's transforms of widths above 8192 (up to 1048576): a two-level transform across workgroups,
// through one float2 scratch buffer in device memory.  The rules (length, split, chunking, bin order) are xl_spectrum_wide_plan.h's.
//
// Method.  N = N1 N2, input n = n1 N2 + j2, output k = k1 + N1 k2:
//   X[k1 + N1 k2] = sum_j2 w_N2^(j2 k2) . w_N^(j2 k1) . sum_n1 x[n1 N2 + j2] w_N1^(n1 k1).
// Column pass: a workgroup holds pack = 4096 / N1 adjacent columns j2 of one transform in 32 KiB of LDS (column c at buf[c N1 ..]), loads
// x[n1 N2 + j2] through the sample converter (runs of `pack` samples), transforms the N1 points of each column, multiplies by w_N^(j2 k1)
// from the N-entry table and stores to scratch[t][k1][j2] in runs of `pack`.
// Row pass, plain widths: xl_spec_b(N2) adjacent rows k1 per workgroup; N2 contiguous points each, transform, power, row maximum.  Bin
// k1 + N1 k2 stays at position k1 N2 + k2 of the row slot: nothing is scattered, and the finishing launch reads through that order
// (xl_specw_col_pos).  Two launches.
// Bluestein (every other width, L = N): the column pass loads x[n] c[n], zero from n = W on (whole rows n1 N2 >= W load nothing).  The
// second transform runs over k = k1 + N1 k2 as its INPUT index, with output m = N2 m1 + m2:
//   conv'[N2 m1 + m2] = sum_k1 w_N1^(k1 m1) . w_N^(k1 m2) . sum_k2 A'[k1 + N1 k2] w_N2^(k2 m2),
// whose first stage is over k2: contiguous in the row the first transform's row pass has just produced.  So the row pass does
// FFT_N2, conj(. Bs) (Bs stored in [k1][k2] order), FFT_N2, times w_N^(k1 m2) without leaving LDS and writes its row back in place; a last
// column pass does the N1-point transforms, X[m] = c[m] conj(conv'[m]), the power of bins m < W and the row maximum, in natural bin
// order and in runs of `pack`.  Three launches.
// What a workgroup does in each pass is xl_spectrum_wide_dev.h's (shared with the bank's ragged kernels, xl_spectrum_bank_wide.hip); every
// piece of its arithmetic is xl_spectrum_dev.h's (xl_fft_lds, xl_sample via xl_spec_point, xl_spec_blue_mid,
// xl_spec_power, the atomicMax on the float's bits); tables are made on the host in double.  The transforms are SCALAR FP32 ONLY, no
// matrix instruction, no sin / cos: the file is compiled with SPEC_FLAGS and -ffp-contract=off like xl_spectrum.hip.  The finishing pass
// takes one double log10 per bin and row (xl_spec_db), as every finishing pass of the family.
#include "xl_spectrum.h"
#include "xl_spectrum_wide_dev.h"

namespace {

// the launch's transform t: its first sample relative to a.in, and its row's ring slot
XL_DEV void xl_specw_where(const XlSpecArgs &a, const uint32_t t, uint32_t &off, uint32_t &slot) {
  const int64_t g = a.g0 + (int64_t)t;
  const int64_t row = g / a.F, k = g - row * a.F;
  off = (uint32_t)(row * a.sr + k * a.W - a.base);
  slot = (uint32_t)(row % a.cap);
}

// The three passes: the single object's prologue (transform t of the launch is transform g0 + t of the one stream, in slot t of the
// scratch) and xl_spectrum_wide_dev.h's body.
template <uint32_t N1, uint32_t N2, int FMT, bool BLUE>
__global__ void __launch_bounds__(XL_SPECW_COL_NT) xl_specw_col_in_kernel(const XlSpecWideArgs w) {
  constexpr uint32_t B = xl_specw_pack(N1), N = N1 * N2, PB = N2 / B;  // PB: packs per transform
  __shared__ v2f buf[XL_SPECW_PACK_POINTS];
  const uint32_t t = blockIdx.x / PB, j0 = (blockIdx.x % PB) * B;
  uint32_t off, slot;
  xl_specw_where(w.a, t, off, slot);
  xl_specw_col_in<N1, N2, FMT, BLUE>(buf, w.a.in, off, j0, w.scratch + (size_t)t * N, w.a.W, w.a.chirp, w.tw1, w.a.tw);
}

template <uint32_t N1, uint32_t N2, bool BLUE>
__global__ void __launch_bounds__(xl_spec_nt(N2)) xl_specw_row_kernel(const XlSpecWideArgs w) {
  constexpr uint32_t B = xl_spec_b(N2), N = N1 * N2;
  __shared__ v2f buf[B * N2];
  const uint32_t r0 = blockIdx.x * B;  // first row of the pack among the launch's T * N1 rows
  const uint32_t t = r0 / N1, k10 = r0 % N1;
  xl_specw_row<N1, N2, BLUE>(buf, w.scratch + (size_t)t * N + (size_t)k10 * N2, k10, w.a.bspec, w.tw2, w.a.tw, w.a.norm, [&]() {
    uint32_t off, slot;
    xl_specw_where(w.a, t, off, slot);
    return w.a.rowmax + (size_t)slot * w.a.W + (size_t)k10 * N2;  // (plain: W = N)
  });
}

template <uint32_t N1, uint32_t N2>
__global__ void __launch_bounds__(XL_SPECW_COL_NT) xl_specw_col_out_kernel(const XlSpecWideArgs w) {
  constexpr uint32_t B = xl_specw_pack(N1), N = N1 * N2, PB = N2 / B;
  __shared__ v2f buf[XL_SPECW_PACK_POINTS];
  const uint32_t t = blockIdx.x / PB, m0 = (blockIdx.x % PB) * B;
  uint32_t off, slot;
  xl_specw_where(w.a, t, off, slot);
  xl_specw_col_out<N1, N2>(buf, w.scratch + (size_t)t * N, m0, w.a.rowmax + (size_t)slot * w.a.W, w.a.W, w.a.chirp, w.tw1, w.a.norm);
}

// the finishing pass of a wide object's rows: xl_spec_finish_kernel's, with the row pass's bin order for a plain width (permuted) and
// nothing else (xl_spec_db and xl_spec_pixel as there)
__global__ void __launch_bounds__(256) xl_specw_finish_kernel(uint32_t *rowmax, float *db, uint8_t *px, const uint32_t W, const uint32_t N1,
                                                              const uint32_t N2, const bool permuted, const uint32_t cap, const int64_t r0) {
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  if (j >= W) return;
  const size_t s = (size_t)((r0 + (int64_t)blockIdx.y) % cap) * W;
  xl_specw_finish_col(rowmax, db, px, s, permuted ? xl_specw_col_pos(N1, N2, W, j) : xl_spec_shift_src(j, W), s, j);
}

// ------------------------------------------------------------------------------------------------------------ launches
template <uint32_t N, bool BLUE>
int xl_specw_launch_n(const XlSpecWideArgs &w, const int fmt, hipStream_t st) {
  constexpr uint32_t N2 = XL_SPECW_N2(N), N1 = N / N2, B = xl_specw_pack(N1);
  static_assert(B >= 16 && N2 % B == 0 && N1 * N2 == N, "the split");
  if (w.N1 != N1 || w.N2 != N2) return (int)hipErrorInvalidValue;  // (the plan and the kernels disagree)
  const dim3 col_grid(w.a.T * (N2 / B)), row_grid(w.a.T * (N1 / xl_spec_b(N2))), col_nt(XL_SPECW_COL_NT);
  if (fmt == XLF_CU8)
    hipLaunchKernelGGL((xl_specw_col_in_kernel<N1, N2, XLF_CU8, BLUE>), col_grid, col_nt, 0, st, w);
  else if (fmt == XLF_CS16)
    hipLaunchKernelGGL((xl_specw_col_in_kernel<N1, N2, XLF_CS16, BLUE>), col_grid, col_nt, 0, st, w);
  else
    hipLaunchKernelGGL((xl_specw_col_in_kernel<N1, N2, XLF_CF32, BLUE>), col_grid, col_nt, 0, st, w);
  hipLaunchKernelGGL((xl_specw_row_kernel<N1, N2, BLUE>), row_grid, dim3(xl_spec_nt(N2)), 0, st, w);
  if constexpr (BLUE) hipLaunchKernelGGL((xl_specw_col_out_kernel<N1, N2>), col_grid, col_nt, 0, st, w);
  return (int)hipGetLastError();
}

}  // namespace

int xl_specw_launch(const XlSpecWideArgs &w, bool bluestein, int fmt, hipStream_t st) {
  if (w.a.T == 0) return 0;
  return xl_specw_dispatch(w.N, bluestein, [&](auto n, auto blue) { return xl_specw_launch_n<n, blue>(w, fmt, st); });
}

int xl_specw_finish(uint32_t *rowmax, float *db, uint8_t *px, uint32_t W, uint32_t N1, uint32_t N2, bool permuted, uint32_t cap, int64_t r0,
                    uint32_t nrows, hipStream_t st) {
  if (nrows == 0) return 0;
  hipLaunchKernelGGL(xl_specw_finish_kernel, dim3((W + 255u) / 256u, nrows), dim3(256), 0, st, rowmax, db, px, W, N1, N2, permuted, cap, r0);
  return (int)hipGetLastError();
}
