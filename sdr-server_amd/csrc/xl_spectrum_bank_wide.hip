// xl_spectrum_bank_wide.hip -- the spectrum bank's kernels for widths above 8192 (xlating_spectrum_bank_create_wide): the two-level
// transform of xl_spectrum_wide.hip over the RAGGED transform list of a bank's round, a chunk of it at a time through the bank's scratch
// buffer; the carries of all streams on a grid over (stream, piece of the carry); the finishing pass over the round's list of rows.
//
// What a workgroup does in each of the three passes is xl_spectrum_wide_dev.h's body, the one xl_spectrum_wide.hip calls too: a row of
// the wide bank is bit for bit the single wide object's row.  What differs is the prologue: transform t of a launch is transform
// t0 + t of the round (t0: the chunk's base); it belongs to the run (XlBankRun) whose running sum tsum covers it, found with
// xl_ragged_find as in xl_bank_kernel, and the run gives the source pointer, the sample offset and the row slot.  It uses slot t of the
// scratch.  A chunk may end inside a run or between two streams' runs: a transform's place in the scratch depends on t alone.
// SCALAR FP32 ONLY, no matrix instructions (Makefile: SPEC_FLAGS), as xl_spectrum_bank.hip: these launches run behind and beside the
// engine's matrix-core launches.  The finishing pass takes one double log10 per bin and row (xl_spec_db), as every finishing pass of
// the family.
#include "xl_ragged.h"
#include "xl_spectrum_bank.h"
#include "xl_spectrum_bank_plan.h"
#include "xl_spectrum_wide_dev.h"

namespace {

// transform t of the launch: its source buffer, its first sample in it, the row slot of its maxima
XL_DEV void xl_bankw_where(const XlBankWideArgs &w, const uint32_t t, const void *&src, uint32_t &off, uint32_t &slot) {
  const uint32_t tr = w.t0 + t;
  const XlBankRun r = w.a.runs[xl_ragged_find(w.a.runs, w.a.nruns, tr, [](const XlBankRun &x) { return x.tsum; })];
  const int64_t g = r.g0 + (int64_t)(tr - r.tsum);
  const int64_t row = g / r.F, k = g - row * r.F;
  src = r.src;
  off = (uint32_t)(row * r.sr + k * w.a.W - r.base);
  slot = r.slot0 + (uint32_t)(row % w.a.slots);
}

template <uint32_t N1, uint32_t N2, int FMT, bool BLUE>
__global__ void __launch_bounds__(XL_SPECW_COL_NT) xl_bankw_col_in_kernel(const XlBankWideArgs w) {
  constexpr uint32_t B = xl_specw_pack(N1), N = N1 * N2, PB = N2 / B;  // PB: packs per transform
  __shared__ v2f buf[XL_SPECW_PACK_POINTS];
  const uint32_t t = blockIdx.x / PB, j0 = (blockIdx.x % PB) * B;
  const void *src;
  uint32_t off, slot;
  xl_bankw_where(w, t, src, off, slot);
  xl_specw_col_in<N1, N2, FMT, BLUE>(buf, src, off, j0, w.scratch + (size_t)t * N, w.a.W, w.a.chirp, w.tw1, w.a.tw);
}

template <uint32_t N1, uint32_t N2, bool BLUE>
__global__ void __launch_bounds__(xl_spec_nt(N2)) xl_bankw_row_kernel(const XlBankWideArgs w) {
  constexpr uint32_t B = xl_spec_b(N2), N = N1 * N2;
  __shared__ v2f buf[B * N2];
  const uint32_t r0 = blockIdx.x * B;  // first row of the pack among the launch's Tc * N1 rows
  const uint32_t t = r0 / N1, k10 = r0 % N1;
  xl_specw_row<N1, N2, BLUE>(buf, w.scratch + (size_t)t * N + (size_t)k10 * N2, k10, w.a.bspec, w.tw2, w.a.tw, w.a.norm, [&]() {
    const void *src;
    uint32_t off, slot;
    xl_bankw_where(w, t, src, off, slot);
    return w.a.rowmax + (size_t)slot * w.a.W + (size_t)k10 * N2;  // (plain: W = N)
  });
}

template <uint32_t N1, uint32_t N2>
__global__ void __launch_bounds__(XL_SPECW_COL_NT) xl_bankw_col_out_kernel(const XlBankWideArgs w) {
  constexpr uint32_t B = xl_specw_pack(N1), N = N1 * N2, PB = N2 / B;
  __shared__ v2f buf[XL_SPECW_PACK_POINTS];
  const uint32_t t = blockIdx.x / PB, m0 = (blockIdx.x % PB) * B;
  const void *src;
  uint32_t off, slot;
  xl_bankw_where(w, t, src, off, slot);
  xl_specw_col_out<N1, N2>(buf, w.scratch + (size_t)t * N, m0, w.a.rowmax + (size_t)slot * w.a.W, w.a.W, w.a.chirp, w.tw1, w.a.norm);
}

// xl_bank_carry_kernel's copies on a grid over (stream of the feed, piece of XL_BANKW_CARRY_PIECE samples): a carry of a million samples
// is not one workgroup's work.  T: an unsigned type of one complex sample's size.
template <typename T>
__global__ void __launch_bounds__(256) xl_bankw_carry_kernel(const XlBankCarry *__restrict__ ops, T *__restrict__ carry, const uint32_t W,
                                                             const bool save) {
  const XlBankCarry op = ops[blockIdx.x];
  const uint32_t n = save ? op.save_n : op.app;
  const uint32_t i0 = blockIdx.y * XL_BANKW_CARRY_PIECE;
  if (i0 >= n) return;
  const uint32_t i1 = n - i0 < XL_BANKW_CARRY_PIECE ? n : i0 + XL_BANKW_CARRY_PIECE;
  const T *__restrict__ in = static_cast<const T *>(op.src) + (save ? op.save_off : 0u);
  T *out = carry + (size_t)op.stream * W + (save ? 0u : op.have);
  for (uint32_t i = i0 + threadIdx.x; i < i1; i += 256u) out[i] = in[i];
}

// xl_bank_finish_kernel's walk over a list of row slots with the wide object's arithmetic: a plain width's bins through the row pass's
// order (xl_specw_col_pos); row i of the list goes to row i of the staging buffers
__global__ void __launch_bounds__(256) xl_bankw_finish_kernel(const uint32_t *__restrict__ list, uint32_t *rowmax, float *db, uint8_t *px,
                                                              const uint32_t W, const uint32_t N1, const uint32_t N2, const bool permuted) {
  const uint32_t j = blockIdx.y * 256u + threadIdx.x;
  if (j >= W) return;
  xl_specw_finish_col(rowmax, db, px, (size_t)list[blockIdx.x] * W, permuted ? xl_specw_col_pos(N1, N2, W, j) : xl_spec_shift_src(j, W),
                      (size_t)blockIdx.x * W, j);
}

template <uint32_t N, bool BLUE>
int xl_bankw_launch_n(const XlBankWideArgs &w, const int fmt, hipStream_t st) {
  constexpr uint32_t N2 = XL_SPECW_N2(N), N1 = N / N2, B = xl_specw_pack(N1);
  static_assert(B >= 16 && N2 % B == 0 && N1 * N2 == N, "the split");
  if (w.N1 != N1 || w.N2 != N2) return (int)hipErrorInvalidValue;  // (the plan and the kernels disagree)
  const dim3 col_grid(w.Tc * (N2 / B)), row_grid(w.Tc * (N1 / xl_spec_b(N2))), col_nt(XL_SPECW_COL_NT);
  if (fmt == XLF_CU8)
    hipLaunchKernelGGL((xl_bankw_col_in_kernel<N1, N2, XLF_CU8, BLUE>), col_grid, col_nt, 0, st, w);
  else if (fmt == XLF_CS16)
    hipLaunchKernelGGL((xl_bankw_col_in_kernel<N1, N2, XLF_CS16, BLUE>), col_grid, col_nt, 0, st, w);
  else
    hipLaunchKernelGGL((xl_bankw_col_in_kernel<N1, N2, XLF_CF32, BLUE>), col_grid, col_nt, 0, st, w);
  hipLaunchKernelGGL((xl_bankw_row_kernel<N1, N2, BLUE>), row_grid, dim3(xl_spec_nt(N2)), 0, st, w);
  if constexpr (BLUE) hipLaunchKernelGGL((xl_bankw_col_out_kernel<N1, N2>), col_grid, col_nt, 0, st, w);
  return (int)hipGetLastError();
}

}  // namespace

int xl_bankw_launch(const XlBankWideArgs &w, bool bluestein, int fmt, hipStream_t st) {
  if (w.Tc == 0 || w.a.nruns == 0 || (uint64_t)w.t0 + w.Tc > w.a.T) return (int)hipErrorInvalidValue;
  return xl_specw_dispatch(w.N, bluestein, [&](auto n, auto blue) { return xl_bankw_launch_n<n, blue>(w, fmt, st); });
}

int xl_bankw_carry(const XlBankCarry *ops, uint32_t n, void *carry, uint32_t W, uint32_t ssz, bool save, hipStream_t st) {
  if (n == 0) return 0;
  const dim3 grid(n, (W + XL_BANKW_CARRY_PIECE - 1u) / XL_BANKW_CARRY_PIECE);
  if (ssz == 2)
    hipLaunchKernelGGL(xl_bankw_carry_kernel<uint16_t>, grid, dim3(256), 0, st, ops, static_cast<uint16_t *>(carry), W, save);
  else if (ssz == 4)
    hipLaunchKernelGGL(xl_bankw_carry_kernel<uint32_t>, grid, dim3(256), 0, st, ops, static_cast<uint32_t *>(carry), W, save);
  else
    hipLaunchKernelGGL(xl_bankw_carry_kernel<uint64_t>, grid, dim3(256), 0, st, ops, static_cast<uint64_t *>(carry), W, save);
  return (int)hipGetLastError();
}

int xl_bankw_finish(const uint32_t *list, uint32_t nrows, uint32_t *rowmax, float *db, uint8_t *px, uint32_t W, uint32_t N1, uint32_t N2,
                    bool permuted, hipStream_t st) {
  if (nrows == 0) return 0;
  hipLaunchKernelGGL(xl_bankw_finish_kernel, dim3(nrows, (W + 255u) / 256u), dim3(256), 0, st, list, rowmax, db, px, W, N1, N2, permuted);
  return (int)hipGetLastError();
}
