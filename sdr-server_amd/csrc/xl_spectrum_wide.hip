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
// Every piece of the transforms' arithmetic is xl_spectrum_dev.h's (xl_fft_lds, xl_sample via xl_spec_point, xl_spec_blue_mid,
// xl_spec_power, the atomicMax on the float's bits); tables are made on the host in double.  The transforms are SCALAR FP32 ONLY, no
// matrix instruction, no sin / cos: the file is compiled with SPEC_FLAGS and -ffp-contract=off like xl_spectrum.hip.  The finishing pass
// alone takes one double log10 per bin and row (xl_specw_db).
#include "xl_spectrum.h"
#include "xl_spectrum_dev.h"
#include "xl_spectrum_wide_plan.h"

namespace {

constexpr uint32_t PACK_POINTS = XL_SPECW_PACK_POINTS;
constexpr uint32_t COL_NT = 256;  // xl_spec_nt of a 4096-point pack
constexpr uint32_t xl_specw_row_points(uint32_t N2) { return xl_spec_b(N2) * N2; }

// the launch's transform t: its first sample relative to a.in, and its row's ring slot
XL_DEV void xl_specw_where(const XlSpecArgs &a, const uint32_t t, uint32_t &off, uint32_t &slot) {
  const int64_t g = a.g0 + (int64_t)t;
  const int64_t row = g / a.F, k = g - row * a.F;
  off = (uint32_t)(row * a.sr + k * a.W - a.base);
  slot = (uint32_t)(row % a.cap);
}

// ------------------------------------------------------------------------------------------------------------ column pass, input side
template <uint32_t N1, uint32_t N2, int FMT, bool BLUE>
__global__ void __launch_bounds__(COL_NT) xl_specw_col_in_kernel(const XlSpecWideArgs w) {
  constexpr uint32_t B = PACK_POINTS / N1, N = N1 * N2, PB = N2 / B;  // PB: packs per transform
  static_assert(xl_spec_b(N1) == B && xl_spec_nt(N1) == COL_NT, "a column pack is an xl_fft_lds pack");
  __shared__ v2f buf[PACK_POINTS];
  const uint32_t tid = threadIdx.x;
  const uint32_t t = blockIdx.x / PB, j0 = (blockIdx.x % PB) * B;
  uint32_t off, slot;
  xl_specw_where(w.a, t, off, slot);
  for (uint32_t q = tid; q < PACK_POINTS; q += COL_NT) {
    const uint32_t c = q % B, n1 = q / B, n = n1 * N2 + j0 + c;
    v2f v = (v2f){0.0f, 0.0f};
    if (n < w.a.W) v = xl_spec_point<FMT, BLUE>(w.a.in, off, n, w.a.chirp);
    buf[c * N1 + n1] = v;
  }
  __syncthreads();
  xl_fft_lds<N1, B, COL_NT>(buf, w.tw1, tid);
  float2 *out = w.scratch + (size_t)t * N;
  for (uint32_t q = tid; q < PACK_POINTS; q += COL_NT) {
    const uint32_t c = q % B, k1 = q / B, j2 = j0 + c;
    const float2 tw = w.a.tw[j2 * k1];
    const v2f v = cmul(buf[c * N1 + k1], (v2f){tw.x, tw.y});
    out[k1 * N2 + j2] = make_float2(v.x, v.y);
  }
}

// ------------------------------------------------------------------------------------------------------------ row pass
template <uint32_t N1, uint32_t N2, bool BLUE>
__global__ void __launch_bounds__(xl_spec_nt(N2)) xl_specw_row_kernel(const XlSpecWideArgs w) {
  constexpr uint32_t B = xl_spec_b(N2), NT = xl_spec_nt(N2), P = B * N2, N = N1 * N2;
  static_assert(N1 % B == 0, "a pack of rows stays inside one transform");
  __shared__ v2f buf[P];
  const uint32_t tid = threadIdx.x;
  const uint32_t r0 = blockIdx.x * B;  // first row of the pack among the launch's T * N1 rows
  const uint32_t t = r0 / N1, k10 = r0 % N1;
  float2 *row = w.scratch + (size_t)t * N + (size_t)k10 * N2;  // B rows, contiguous
  for (uint32_t q = tid; q < P; q += NT) {
    const float2 v = row[q];
    buf[q] = (v2f){v.x, v.y};
  }
  __syncthreads();
  xl_fft_lds<N2, B, NT>(buf, w.tw2, tid);
  if constexpr (BLUE) {
    const float2 *bs = w.a.bspec + (size_t)k10 * N2;
    for (uint32_t q = tid; q < P; q += NT) buf[q] = xl_spec_blue_mid(buf[q], bs[q]);
    __syncthreads();
    xl_fft_lds<N2, B, NT>(buf, w.tw2, tid);
    for (uint32_t q = tid; q < P; q += NT) {
      const uint32_t k1 = k10 + q / N2, m2 = q % N2;
      const float2 tw = w.a.tw[k1 * m2];
      const v2f v = cmul(buf[q], (v2f){tw.x, tw.y});
      row[q] = make_float2(v.x, v.y);
    }
  } else {
    uint32_t off, slot;
    xl_specw_where(w.a, t, off, slot);
    uint32_t *mx = w.a.rowmax + (size_t)slot * w.a.W + (size_t)k10 * N2;  // (plain: W = N)
    for (uint32_t q = tid; q < P; q += NT) {
      const float pw = xl_spec_power<false>(buf[q], (v2f){1.0f, 0.0f}, w.a.norm);
      atomicMax(mx + q, __float_as_uint(pw));
    }
  }
}

// ------------------------------------------------------------------------------------------------------------ column pass, output side
template <uint32_t N1, uint32_t N2>
__global__ void __launch_bounds__(COL_NT) xl_specw_col_out_kernel(const XlSpecWideArgs w) {
  constexpr uint32_t B = PACK_POINTS / N1, N = N1 * N2, PB = N2 / B;
  __shared__ v2f buf[PACK_POINTS];
  const uint32_t tid = threadIdx.x;
  const uint32_t t = blockIdx.x / PB, m0 = (blockIdx.x % PB) * B;
  uint32_t off, slot;
  xl_specw_where(w.a, t, off, slot);
  const float2 *in = w.scratch + (size_t)t * N;
  for (uint32_t q = tid; q < PACK_POINTS; q += COL_NT) {
    const uint32_t c = q % B, k1 = q / B;
    const float2 v = in[k1 * N2 + m0 + c];
    buf[c * N1 + k1] = (v2f){v.x, v.y};
  }
  __syncthreads();
  xl_fft_lds<N1, B, COL_NT>(buf, w.tw1, tid);
  uint32_t *mx = w.a.rowmax + (size_t)slot * w.a.W;
  for (uint32_t q = tid; q < PACK_POINTS; q += COL_NT) {
    const uint32_t c = q % B, m1 = q / B, m = m1 * N2 + m0 + c;
    if (m < w.a.W) {
      const float2 cj = w.a.chirp[m];
      const float pw = xl_spec_power<true>(buf[c * N1 + m1], (v2f){cj.x, cj.y}, w.a.norm);
      atomicMax(mx + m, __float_as_uint(pw));
    }
  }
}

// spectrogram.c:150: 10 * log10f(v) with the log10f the reference gets from its libm, the correctly rounded one.  The device's log10f is
// an ulp off here and there -- at v = 1e-20f, the floor every bin of a silent input sits on, it gives -20.000002 and so pixel 54 where
// the reference writes 55 -- so this one value per bin and row is taken in double and rounded once; the product is the float one.
XL_DEV float xl_specw_db(const float v) { return 10.0f * (float)log10((double)v); }

// the finishing pass of a wide object's rows: xl_spec_finish_kernel's, with the row pass's bin order for a plain width (permuted) and
// xl_specw_db
__global__ void __launch_bounds__(256) xl_specw_finish_kernel(uint32_t *rowmax, float *db, uint8_t *px, const uint32_t W, const uint32_t N1,
                                                              const uint32_t N2, const bool permuted, const uint32_t cap, const int64_t r0) {
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  if (j >= W) return;
  const size_t s = (size_t)((r0 + (int64_t)blockIdx.y) % cap) * W;
  const uint32_t from = permuted ? xl_specw_col_pos(N1, N2, W, j) : xl_spec_shift_src(j, W);
  const float v = __uint_as_float(rowmax[s + from]);
  rowmax[s + from] = 0u;  // (either order is a permutation of the slot: every bin is read and cleared by exactly one thread)
  const float d = xl_specw_db(v);
  db[s + j] = d;
  px[s + j] = xl_spec_pixel(d);
}

// ------------------------------------------------------------------------------------------------------------ launches
template <uint32_t N, bool BLUE>
int xl_specw_launch_n(const XlSpecWideArgs &w, const int fmt, hipStream_t st) {
  constexpr uint32_t N2 = XL_SPECW_N2(N), N1 = N / N2, B = PACK_POINTS / N1;
  static_assert(B >= 16 && N2 % B == 0 && N1 * N2 == N, "the split");
  if (w.N1 != N1 || w.N2 != N2) return (int)hipErrorInvalidValue;  // (the plan and the kernels disagree)
  const dim3 col_grid(w.a.T * (N2 / B)), row_grid(w.a.T * (N1 / xl_spec_b(N2)));
  if (fmt == XLF_CU8)
    hipLaunchKernelGGL((xl_specw_col_in_kernel<N1, N2, XLF_CU8, BLUE>), col_grid, dim3(COL_NT), 0, st, w);
  else if (fmt == XLF_CS16)
    hipLaunchKernelGGL((xl_specw_col_in_kernel<N1, N2, XLF_CS16, BLUE>), col_grid, dim3(COL_NT), 0, st, w);
  else
    hipLaunchKernelGGL((xl_specw_col_in_kernel<N1, N2, XLF_CF32, BLUE>), col_grid, dim3(COL_NT), 0, st, w);
  hipLaunchKernelGGL((xl_specw_row_kernel<N1, N2, BLUE>), row_grid, dim3(xl_spec_nt(N2)), 0, st, w);
  if constexpr (BLUE) hipLaunchKernelGGL((xl_specw_col_out_kernel<N1, N2>), col_grid, dim3(COL_NT), 0, st, w);
  return (int)hipGetLastError();
}

}  // namespace

int xl_specw_launch(const XlSpecWideArgs &w, bool bluestein, int fmt, hipStream_t st) {
  if (w.a.T == 0) return 0;
  if (bluestein) {
    switch (w.N) {
      case 1u << 15: return xl_specw_launch_n<1u << 15, true>(w, fmt, st);
      case 1u << 16: return xl_specw_launch_n<1u << 16, true>(w, fmt, st);
      case 1u << 17: return xl_specw_launch_n<1u << 17, true>(w, fmt, st);
      case 1u << 18: return xl_specw_launch_n<1u << 18, true>(w, fmt, st);
      case 1u << 19: return xl_specw_launch_n<1u << 19, true>(w, fmt, st);
      case 1u << 20: return xl_specw_launch_n<1u << 20, true>(w, fmt, st);
      case 1u << 21: return xl_specw_launch_n<1u << 21, true>(w, fmt, st);
    }
    return (int)hipErrorInvalidValue;
  }
  switch (w.N) {
    case 1u << 14: return xl_specw_launch_n<1u << 14, false>(w, fmt, st);
    case 1u << 15: return xl_specw_launch_n<1u << 15, false>(w, fmt, st);
    case 1u << 16: return xl_specw_launch_n<1u << 16, false>(w, fmt, st);
    case 1u << 17: return xl_specw_launch_n<1u << 17, false>(w, fmt, st);
    case 1u << 18: return xl_specw_launch_n<1u << 18, false>(w, fmt, st);
    case 1u << 19: return xl_specw_launch_n<1u << 19, false>(w, fmt, st);
    case 1u << 20: return xl_specw_launch_n<1u << 20, false>(w, fmt, st);
  }
  return (int)hipErrorInvalidValue;
}

int xl_specw_finish(uint32_t *rowmax, float *db, uint8_t *px, uint32_t W, uint32_t N1, uint32_t N2, bool permuted, uint32_t cap, int64_t r0,
                    uint32_t nrows, hipStream_t st) {
  if (nrows == 0) return 0;
  hipLaunchKernelGGL(xl_specw_finish_kernel, dim3((W + 255u) / 256u, nrows), dim3(256), 0, st, rowmax, db, px, W, N1, N2, permuted, cap, r0);
  return (int)hipGetLastError();
}
