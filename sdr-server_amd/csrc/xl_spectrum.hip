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
// unsigned atomicMax on the float's bits whenever the row changes and at the end (powers are positive: bit order = value order).
// SCALAR FP32 ONLY: compiled without the SLP vectoriser (Makefile: SPEC_FLAGS) -- these launches may share a chip, and a process,
// with the engine's matrix-core launches, beside which packed FP32 loses lanes (xl_mixh.hip).  No matrix instructions.
#include "xl_dev_inline.h"
#include "xl_spectrum.h"

namespace {

constexpr int xl_log2(uint32_t n) { return n <= 1 ? 0 : 1 + xl_log2(n >> 1); }
constexpr uint32_t xl_spec_b(uint32_t N) { return N >= 4096 ? 1u : (4096u / N > 256u ? 256u : 4096u / N); }
constexpr uint32_t xl_spec_nt(uint32_t N) { return xl_spec_b(N) * N / 16u < 16u ? 16u : xl_spec_b(N) * N / 16u; }

XL_DEV v2f cmul(const v2f a, const v2f b) { return (v2f){a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x}; }
XL_DEV v2f cadd(const v2f a, const v2f b) { return (v2f){a.x + b.x, a.y + b.y}; }
XL_DEV v2f csub(const v2f a, const v2f b) { return (v2f){a.x - b.x, a.y - b.y}; }
XL_DEV v2f conj2(const v2f a) { return (v2f){a.x, -a.y}; }

// B forward transforms of N points, in place in buf[b * N + n]
template <uint32_t N, uint32_t B, uint32_t NT>
XL_DEV void xl_fft_lds(v2f *buf, const float2 *__restrict__ tw, const uint32_t tid) {
  constexpr int LOG = xl_log2(N);
  constexpr uint32_t Q = N / 4u > 0 ? N / 4u : 1u;       // (N < 4: no radix-4 pass)
  constexpr uint32_t BF4 = N >= 4 ? B * Q / NT : 0;  // radix-4 butterflies per thread and pass
  uint32_t p = 1;
  for (int s = 0; s < LOG / 2; ++s) {
    v2f x[BF4 > 0 ? BF4 : 1][4];
#pragma unroll
    for (uint32_t u = 0; u < BF4; ++u) {
      const uint32_t idx = tid + u * NT, base = (idx / Q) * N, i = idx % Q;
#pragma unroll
      for (int t = 0; t < 4; ++t) x[u][t] = buf[base + i + t * Q];
    }
    __syncthreads();
#pragma unroll
    for (uint32_t u = 0; u < BF4; ++u) {
      const uint32_t idx = tid + u * NT, base = (idx / Q) * N, i = idx % Q, k = i & (p - 1u);
      const uint32_t step = N / (4u * p);
#pragma unroll
      for (uint32_t t = 1; t < 4; ++t) {
        const float2 w = tw[t * k * step];
        x[u][t] = cmul(x[u][t], (v2f){w.x, w.y});
      }
      const v2f a0 = cadd(x[u][0], x[u][2]), a1 = csub(x[u][0], x[u][2]), a2 = cadd(x[u][1], x[u][3]);
      const v2f d = csub(x[u][1], x[u][3]);
      const v2f a3 = (v2f){d.y, -d.x};  // -i (x1 - x3)
      const uint32_t j = base + (i - k) * 4u + k;
      buf[j] = cadd(a0, a2);
      buf[j + p] = cadd(a1, a3);
      buf[j + 2u * p] = csub(a0, a2);
      buf[j + 3u * p] = csub(a1, a3);
    }
    __syncthreads();
    p *= 4u;
  }
  if constexpr ((LOG & 1) != 0) {
    constexpr uint32_t H = N / 2u;
    constexpr uint32_t BF2 = B * H / NT;
    v2f x[BF2][2];
#pragma unroll
    for (uint32_t u = 0; u < BF2; ++u) {
      const uint32_t idx = tid + u * NT, base = (idx / H) * N, i = idx % H;
      x[u][0] = buf[base + i];
      x[u][1] = buf[base + i + H];
    }
    __syncthreads();
#pragma unroll
    for (uint32_t u = 0; u < BF2; ++u) {
      const uint32_t idx = tid + u * NT, base = (idx / H) * N, i = idx % H;  // p == H here: k = i
      const float2 w = tw[i];
      const v2f x1 = cmul(x[u][1], (v2f){w.x, w.y});
      buf[base + i] = cadd(x[u][0], x1);  // j = (i - k) * 2 + k = i
      buf[base + i + H] = csub(x[u][0], x1);
    }
    __syncthreads();
  }
}

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
  __syncthreads();
  // load (iq_file.c:142-143, 167-168: xl_sample's converters)
  for (uint32_t q = tid; q < B * N; q += NT) {
    const uint32_t b = q / N, n = q % N;
    v2f v = (v2f){0.0f, 0.0f};
    if (slot[b] != ~0u && n < a.W) {
      v = xl_sample(a.in, FMT, off[b] + n);
      if constexpr (BLUE) {
        const float2 c = a.chirp[n];
        v = cmul(v, (v2f){c.x, c.y});
      }
    }
    buf[q] = v;
  }
  __syncthreads();
  xl_fft_lds<N, B, NT>(buf, a.tw, tid);
  if constexpr (BLUE) {
    for (uint32_t q = tid; q < B * N; q += NT) {
      const float2 s = a.bspec[q % N];
      buf[q] = conj2(cmul(buf[q], (v2f){s.x, s.y}));
    }
    __syncthreads();
    xl_fft_lds<N, B, NT>(buf, a.tw, tid);
  }
  // power and row maximum (spectrogram.c:140-144): re, im times 1.0f / W each, re^2 + im^2 + 1e-20f
  for (uint32_t j = tid; j < a.W; j += NT) {
    const v2f cj = BLUE ? (v2f){a.chirp[j].x, a.chirp[j].y} : (v2f){1.0f, 0.0f};
    uint32_t cur = ~0u, m = 0u;
    for (uint32_t b = 0; b < B; ++b) {
      const uint32_t sl = slot[b];
      if (sl == ~0u) break;
      v2f X = buf[b * N + j];
      if constexpr (BLUE) X = cmul(conj2(X), cj);
      const float re = X.x * a.norm, im = X.y * a.norm;
      const float pw = re * re + im * im + 1e-20f;
      if (sl != cur) {
        if (cur != ~0u) atomicMax(a.rowmax + (size_t)cur * a.W + j, m);
        cur = sl;
        m = 0u;
      }
      const uint32_t bits = __float_as_uint(pw);
      m = bits > m ? bits : m;
    }
    if (cur != ~0u) atomicMax(a.rowmax + (size_t)cur * a.W + j, m);
  }
}

// spectrogram.c:150-158 (10 log10f, halves swapped with half = W / 2, an odd W's last bin in place) and png_util.c:53-63 (the pixel)
__global__ void __launch_bounds__(256) xl_spec_finish_kernel(uint32_t *rowmax, float *db, uint8_t *px, const uint32_t W,
                                                             const uint32_t cap, const int64_t r0) {
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  if (j >= W) return;
  const size_t s = (size_t)((r0 + (int64_t)blockIdx.y) % cap) * W;
  const uint32_t half = W / 2u;
  const uint32_t src = j < half ? j + half : (j < 2u * half ? j - half : j);
  const float v = __uint_as_float(rowmax[s + src]);
  rowmax[s + src] = 0u;  // (a permutation: every bin is read and cleared by exactly one thread)
  const float d = 10.0f * log10f(v);
  const float f = d + 255.0f;
  const int pixel = f >= 255.0f ? 255 : (f > 0.0f ? (int)f : 0);
  db[s + j] = d;
  px[s + j] = (uint8_t)pixel;
}

template <uint32_t N, bool BLUE>
int xl_spec_launch_n(const XlSpecArgs &a, int fmt, hipStream_t st) {
  const uint32_t B = xl_spec_b(N);
  const dim3 grid((unsigned)((a.T + B - 1u) / B)), block(xl_spec_nt(N));
  if (fmt == XLF_CU8)
    hipLaunchKernelGGL((xl_spec_kernel<N, XLF_CU8, BLUE>), grid, block, 0, st, a);
  else if (fmt == XLF_CS16)
    hipLaunchKernelGGL((xl_spec_kernel<N, XLF_CS16, BLUE>), grid, block, 0, st, a);
  else
    hipLaunchKernelGGL((xl_spec_kernel<N, XLF_CF32, BLUE>), grid, block, 0, st, a);
  return (int)hipGetLastError();
}

}  // namespace

int xl_spec_launch(const XlSpecArgs &a, uint32_t N, bool bluestein, int fmt, hipStream_t st) {
  if (a.T == 0) return 0;
  if (bluestein) {
    switch (N) {
      case 8: return xl_spec_launch_n<8, true>(a, fmt, st);
      case 16: return xl_spec_launch_n<16, true>(a, fmt, st);
      case 32: return xl_spec_launch_n<32, true>(a, fmt, st);
      case 64: return xl_spec_launch_n<64, true>(a, fmt, st);
      case 128: return xl_spec_launch_n<128, true>(a, fmt, st);
      case 256: return xl_spec_launch_n<256, true>(a, fmt, st);
      case 512: return xl_spec_launch_n<512, true>(a, fmt, st);
      case 1024: return xl_spec_launch_n<1024, true>(a, fmt, st);
      case 2048: return xl_spec_launch_n<2048, true>(a, fmt, st);
      case 4096: return xl_spec_launch_n<4096, true>(a, fmt, st);
      case 8192: return xl_spec_launch_n<8192, true>(a, fmt, st);
      case 16384: return xl_spec_launch_n<16384, true>(a, fmt, st);
    }
    return (int)hipErrorInvalidValue;
  }
  switch (N) {
    case 1: return xl_spec_launch_n<1, false>(a, fmt, st);
    case 2: return xl_spec_launch_n<2, false>(a, fmt, st);
    case 4: return xl_spec_launch_n<4, false>(a, fmt, st);
    case 8: return xl_spec_launch_n<8, false>(a, fmt, st);
    case 16: return xl_spec_launch_n<16, false>(a, fmt, st);
    case 32: return xl_spec_launch_n<32, false>(a, fmt, st);
    case 64: return xl_spec_launch_n<64, false>(a, fmt, st);
    case 128: return xl_spec_launch_n<128, false>(a, fmt, st);
    case 256: return xl_spec_launch_n<256, false>(a, fmt, st);
    case 512: return xl_spec_launch_n<512, false>(a, fmt, st);
    case 1024: return xl_spec_launch_n<1024, false>(a, fmt, st);
    case 2048: return xl_spec_launch_n<2048, false>(a, fmt, st);
    case 4096: return xl_spec_launch_n<4096, false>(a, fmt, st);
    case 8192: return xl_spec_launch_n<8192, false>(a, fmt, st);
  }
  return (int)hipErrorInvalidValue;
}

int xl_spec_finish(uint32_t *rowmax, float *db, uint8_t *px, uint32_t W, uint32_t cap, int64_t r0, uint32_t nrows, hipStream_t st) {
  if (nrows == 0) return 0;
  hipLaunchKernelGGL(xl_spec_finish_kernel, dim3((W + 255u) / 256u, nrows), dim3(256), 0, st, rowmax, db, px, W, cap, r0);
  return (int)hipGetLastError();
}
