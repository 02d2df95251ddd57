// xl_spectrum_dev.h -- the arithmetic of one spectrogram transform, shared by the single stream's kernel (xl_spectrum.hip) and the
// bank's ragged kernel (xl_spectrum_bank.hip): packing constants, the Stockham transform in LDS, the load (sample converter and
// Bluestein pre-multiplication), the Bluestein middle step, the power expression and the finishing dB / pixel.  Both files instantiate
// these and nothing else for a transform's values, with the same compiler flags (Makefile: SPEC_FLAGS, -ffp-contract=off): a row of the
// bank is bit for bit the row of the single object.  See xl_spectrum.hip's header for the method.
#ifndef XL_SPECTRUM_DEV_H_
#define XL_SPECTRUM_DEV_H_

#include "xl_dev_inline.h"

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

// point n (< W) of a transform whose sample 0 is element `off` of `in` (iq_file.c:142-143, 167-168: xl_sample's converters); Bluestein:
// times the chirp
template <int FMT, bool BLUE>
XL_DEV v2f xl_spec_point(const void *__restrict__ in, const uint32_t off, const uint32_t n, const float2 *__restrict__ chirp) {
  v2f v = xl_sample(in, FMT, off + n);
  if constexpr (BLUE) {
    const float2 c = chirp[n];
    v = cmul(v, (v2f){c.x, c.y});
  }
  return v;
}

// Bluestein, between the two transforms: conj(A . Bs)
XL_DEV v2f xl_spec_blue_mid(const v2f A, const float2 s) { return conj2(cmul(A, (v2f){s.x, s.y})); }

// bin j's power from the transform's output X (spectrogram.c:140-144): re, im times 1.0f / W each, re^2 + im^2 + 1e-20f; Bluestein:
// X = c[j] conj(second transform)
template <bool BLUE>
XL_DEV float xl_spec_power(v2f X, const v2f cj, const float norm) {
  if constexpr (BLUE) X = cmul(conj2(X), cj);
  const float re = X.x * norm, im = X.y * norm;
  return re * re + im * im + 1e-20f;
}

// spectrogram.c:150-158: the bin that lands in column j after the halves of half = W / 2 are swapped (an odd W's last bin in place)
XL_DEV uint32_t xl_spec_shift_src(const uint32_t j, const uint32_t W) {
  const uint32_t half = W / 2u;
  return j < half ? j + half : (j < 2u * half ? j - half : j);
}

// spectrogram.c:150 (10 log10f) and png_util.c:53-63 (the pixel) of a row maximum
XL_DEV float xl_spec_db(const float v) { return 10.0f * log10f(v); }
XL_DEV uint8_t xl_spec_pixel(const float d) {
  const float f = d + 255.0f;
  const int pixel = f >= 255.0f ? 255 : (f > 0.0f ? (int)f : 0);
  return (uint8_t)pixel;
}

}  // namespace

#endif  // XL_SPECTRUM_DEV_H_
