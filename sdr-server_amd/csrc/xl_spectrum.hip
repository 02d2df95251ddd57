// xl_spectrum.hip -- the spectrogram's kernels (reference src/spectrogram/spectrogram.c:84-168): batched forward DFTs of W samples,
// their power, the per-row maximum per bin, and the finishing dB / shift / pixel pass.
//
// Transform: a Stockham radix-4 pass sequence (radix-2 on the last pass for odd log2 N) in LDS, in place in ONE buffer per transform:
// every thread reads its butterflies' points into registers, the workgroup meets at a barrier, and only then writes them to their
// Stockham destinations.  Powers of two W <= 8192 run it at N = W.  Every other W runs Bluestein at the power of two N = L >= 2 W - 1:
// a[n] = x[n] c[n] with the chirp c[n] = exp(-i pi (n^2 mod 2W) / W), A = FFT_L(a), conv = conj(FFT_L(conj(A . Bs))) with Bs the
// chirp filter's spectrum over L (host, double), X[k] = c[k] conv[k].  Twiddles, chirp and Bs are float2 tables made on the host in
// double; nothing here evaluates sin / cos.
// Packing: a workgroup holds B = min(256, max(1, 4096 / N)) transforms (P = B N points, P / 16 threads: every thread does 4 radix-4 or
// 8 radix-2 butterflies per pass), so a 64-point transform is not a workgroup on its own.
// Row maximum: per bin, one thread walks the workgroup's transforms in order and keeps a running maximum per row, flushed by an
// unsigned atomicMax on the float's bits whenever the row changes and at the end (powers are positive: bit order = value order;
// a NaN power enters as 0u and so loses, as against the reference's fmaxf: xl_spec_max_bits).
// SCALAR FP32 ONLY: compiled without the SLP vectoriser (Makefile: SPEC_FLAGS) -- these launches may share a chip, and a process,
// with the engine's matrix-core launches, beside which packed FP32 loses lanes (xl_mixh.hip).  No matrix instructions.
#include "xl_spectrum.h"
#include "xl_spectrum_dev.h"

namespace {

template <uint32_t N, int FMT, bool BLUE>
__global__ void __launch_bounds__(xl_spec_nt(N)) xl_spec_kernel(const XlSpecArgs a) {
  constexpr uint32_t B = xl_spec_b(N);
  constexpr uint32_t NT = xl_spec_nt(N);
  __shared__ v2f buf[B * N];
  __shared__ uint32_t off[B];   // first sample of transform b, relative to a.in
  __shared__ uint32_t slot[B];  // its row's ring slot; ~0u: past the launch's transforms
  const uint32_t tid = threadIdx.x;
  const uint64_t first = (uint64_t)blockIdx.x * B;
  for (uint32_t b = tid; b < B; b += NT) {
    const uint64_t t = first + b;
    if (t < a.T) {
      const int64_t g = a.g0 + (int64_t)t;
      const int64_t row = g / a.F, k = g - row * a.F;
      off[b] = (uint32_t)(row * a.sr + k * a.W - a.base);
      slot[b] = (uint32_t)(row % a.cap);
    } else {
      off[b] = 0u;
      slot[b] = ~0u;
    }
  }
  xl_spec_pack<N, FMT, BLUE>(buf, off, slot, a, [&](uint32_t) { return a.in; });
}

// spectrogram.c:150-158 (10 log10f, halves swapped with half = W / 2, an odd W's last bin in place) and png_util.c:53-63 (the pixel)
__global__ void __launch_bounds__(256) xl_spec_finish_kernel(uint32_t *rowmax, float *db, uint8_t *px, const uint32_t W,
                                                             const uint32_t cap, const int64_t r0) {
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  if (j >= W) return;
  const size_t s = (size_t)((r0 + (int64_t)blockIdx.y) % cap) * W;
  xl_spec_finish_bin(rowmax, db, px, W, j, s, s);
}

}  // namespace

int xl_spec_launch(const XlSpecArgs &a, uint32_t N, bool bluestein, int fmt, hipStream_t st) {
  if (a.T == 0) return 0;
  return xl_spec_dispatch(N, bluestein, fmt, [&](auto n, auto f, auto blue) {
    constexpr uint32_t B = xl_spec_b(n);
    hipLaunchKernelGGL((xl_spec_kernel<n, f, blue>), dim3((unsigned)((a.T + B - 1u) / B)), dim3(xl_spec_nt(n)), 0, st, a);
  });
}

int xl_spec_finish(uint32_t *rowmax, float *db, uint8_t *px, uint32_t W, uint32_t cap, int64_t r0, uint32_t nrows, hipStream_t st) {
  if (nrows == 0) return 0;
  hipLaunchKernelGGL(xl_spec_finish_kernel, dim3((W + 255u) / 256u, nrows), dim3(256), 0, st, rowmax, db, px, W, cap, r0);
  return (int)hipGetLastError();
}
