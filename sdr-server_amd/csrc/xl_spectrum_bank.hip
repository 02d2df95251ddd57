// xl_spectrum_bank.hip -- the spectrum bank's kernels (include/xlating_spectrum.h, xlating_spectrum_bank_*): the transforms of MANY
// streams in one ragged launch, the carries of all streams in one launch before and one after it, and the finishing pass over the
// list of rows a feed completed.
//
// What a workgroup does with its pack of transforms is xl_spectrum_dev.h's xl_spec_pack, the one body xl_spectrum.hip calls too: a
// bank row is bit for bit the single object's row.  What differs is the prologue, where a packed transform comes from: a workgroup
// still packs B = xl_spec_b(N) transforms, but transform t of the launch belongs to the run (XlBankRun: one stream's transforms in
// one source buffer) whose running sum tsum covers t, found by a binary search per packed transform; its source pointer, sample
// offset and row slot are kept in LDS.  The shared body flushes the row maximum whenever the row slot changes along the pack; here
// a slot belongs to one stream and, within a launch, to one row: stream or row changes are slot changes.
// SCALAR FP32 ONLY, no matrix instructions (Makefile: SPEC_FLAGS), as xl_spectrum.hip: these launches run behind and beside the
// engine's matrix-core launches.
#include "xl_ragged.h"
#include "xl_spectrum_bank.h"
#include "xl_spectrum_dev.h"

namespace {

template <uint32_t N, int FMT, bool BLUE>
__global__ void __launch_bounds__(xl_spec_nt(N)) xl_bank_kernel(const XlBankArgs a) {
  constexpr uint32_t B = xl_spec_b(N);
  constexpr uint32_t NT = xl_spec_nt(N);
  __shared__ v2f buf[B * N];
  __shared__ const void *src[B];  // the buffer transform b reads
  __shared__ uint32_t off[B];     // its first sample, relative to src[b]
  __shared__ uint32_t slot[B];    // its row's slot; ~0u: past the launch's transforms
  const uint32_t tid = threadIdx.x;
  const uint64_t first = (uint64_t)blockIdx.x * B;
  for (uint32_t b = tid; b < B; b += NT) {
    const uint64_t t = first + b;
    if (t < a.T) {
      const XlBankRun r = a.runs[xl_ragged_find(a.runs, a.nruns, (uint32_t)t, [](const XlBankRun &x) { return x.tsum; })];
      const int64_t g = r.g0 + (int64_t)((uint32_t)t - r.tsum);
      const int64_t row = g / r.F, k = g - row * r.F;
      src[b] = r.src;
      off[b] = (uint32_t)(row * r.sr + k * a.W - r.base);
      slot[b] = r.slot0 + (uint32_t)(row % a.slots);
    } else {
      src[b] = nullptr;
      off[b] = 0u;
      slot[b] = ~0u;
    }
  }
  xl_spec_pack<N, FMT, BLUE>(buf, off, slot, a, [&](uint32_t b) { return src[b]; });
}

// one workgroup per stream of the feed; T: an unsigned type of one complex sample's size
template <typename T>
__global__ void __launch_bounds__(256) xl_bank_carry_kernel(const XlBankCarry *__restrict__ ops, T *__restrict__ carry, const uint32_t W,
                                                            const bool save) {
  const XlBankCarry op = ops[blockIdx.x];
  const T *__restrict__ in = static_cast<const T *>(op.src);
  T *out = carry + (size_t)op.stream * W;
  if (save) {
    for (uint32_t i = threadIdx.x; i < op.save_n; i += 256u) out[i] = in[op.save_off + i];
  } else {
    for (uint32_t i = threadIdx.x; i < op.app; i += 256u) out[op.have + i] = in[i];
  }
}

// spectrogram.c:150-158 and png_util.c:53-63 as xl_spec_finish_kernel, over a list of row slots; row i of the list goes to row i of the
// staging buffers
__global__ void __launch_bounds__(256) xl_bank_finish_kernel(const uint32_t *__restrict__ list, uint32_t *rowmax, float *db, uint8_t *px,
                                                             const uint32_t W) {
  const uint32_t j = blockIdx.y * 256u + threadIdx.x;
  if (j >= W) return;
  xl_spec_finish_bin(rowmax, db, px, W, j, (size_t)list[blockIdx.x] * W, (size_t)blockIdx.x * W);
}

}  // namespace

int xl_bank_launch(const XlBankArgs &a, uint32_t N, bool bluestein, int fmt, hipStream_t st) {
  if (a.T == 0 || a.nruns == 0) return 0;
  return xl_spec_dispatch(N, bluestein, fmt, [&](auto n, auto f, auto blue) {
    constexpr uint32_t B = xl_spec_b(n);
    hipLaunchKernelGGL((xl_bank_kernel<n, f, blue>), dim3((unsigned)(((uint64_t)a.T + B - 1u) / B)), dim3(xl_spec_nt(n)), 0, st, a);
  });
}

int xl_bank_carry(const XlBankCarry *ops, uint32_t n, void *carry, uint32_t W, uint32_t ssz, bool save, hipStream_t st) {
  if (n == 0) return 0;
  if (ssz == 2)
    hipLaunchKernelGGL(xl_bank_carry_kernel<uint16_t>, dim3(n), dim3(256), 0, st, ops, static_cast<uint16_t *>(carry), W, save);
  else if (ssz == 4)
    hipLaunchKernelGGL(xl_bank_carry_kernel<uint32_t>, dim3(n), dim3(256), 0, st, ops, static_cast<uint32_t *>(carry), W, save);
  else
    hipLaunchKernelGGL(xl_bank_carry_kernel<uint64_t>, dim3(n), dim3(256), 0, st, ops, static_cast<uint64_t *>(carry), W, save);
  return (int)hipGetLastError();
}

int xl_bank_finish(const uint32_t *list, uint32_t nrows, uint32_t *rowmax, float *db, uint8_t *px, uint32_t W, hipStream_t st) {
  if (nrows == 0) return 0;
  hipLaunchKernelGGL(xl_bank_finish_kernel, dim3(nrows, (W + 255u) / 256u), dim3(256), 0, st, list, rowmax, db, px, W);
  return (int)hipGetLastError();
}
