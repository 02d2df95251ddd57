// xl_spectrum_dev.h -- everything a workgroup of spectrogram transforms does once it knows where its transforms come from, shared by
// the single stream's kernel (xl_spectrum.hip) and the bank's ragged kernel (xl_spectrum_bank.hip): packing constants, the Stockham
// transform in LDS, xl_spec_pack (load with sample converter and Bluestein pre-multiplication, transform, Bluestein middle step and
// second transform, power, row maximum and its flush), xl_spec_finish_bin (dB, half swap, pixel), and the host-side list of the
// transform lengths that have kernels (xl_spec_dispatch).  A kernel of either file is its LDS, its own prologue (which samples, which
// row slot) and one call; both files are compiled with the same flags (Makefile: SPEC_FLAGS, -ffp-contract=off): a row of the bank is bit
// for bit the row of the single object.  See xl_spectrum.hip's header for the method.
#ifndef XL_SPECTRUM_DEV_H_
#define XL_SPECTRUM_DEV_H_

#include <type_traits>

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

// The bits of a power as they enter a row maximum (spectrogram.c:148: fmaxf(temp[j], power), which a NaN power loses against any number):
// 0u for a NaN, whose own bits (0x7FC.., 0xFFC..) would beat every power in the unsigned order; the float's bits otherwise.  A row
// whose every transform holds a NaN keeps the cleared maximum 0u: dB -Inf, pixel 0.
XL_DEV uint32_t xl_spec_max_bits(const float pw) { return pw != pw ? 0u : __float_as_uint(pw); }

// A workgroup's pack of B = xl_spec_b(N) transforms, after the kernel's prologue has written for each: off[b], its first sample as an
// element index into src(b), and slot[b], the row slot its maxima go to (~0u from the first b past the launch's transforms).  Load,
// transform, power; then per bin one thread walks the pack in order with a running maximum, flushed by an unsigned atomicMax on the
// power's bits (xl_spec_max_bits) whenever the slot changes and at the end.  A slot change is a row or stream change: along a pack the
// transforms of one row of one stream are consecutive.  a: XlSpecArgs or XlBankArgs (W, rowmax, tw, chirp, bspec, norm).
template <uint32_t N, int FMT, bool BLUE, class Args, class Src>
XL_DEV void xl_spec_pack(v2f *buf, const uint32_t *off, const uint32_t *slot, const Args &a, const Src src) {
  constexpr uint32_t B = xl_spec_b(N);
  constexpr uint32_t NT = xl_spec_nt(N);
  const uint32_t tid = threadIdx.x;
  __syncthreads();  // (the prologue's off[] / slot[])
  for (uint32_t q = tid; q < B * N; q += NT) {
    const uint32_t b = q / N, n = q % N;
    v2f v = (v2f){0.0f, 0.0f};
    if (slot[b] != ~0u && n < a.W) v = xl_spec_point<FMT, BLUE>(src(b), off[b], n, a.chirp);
    buf[q] = v;
  }
  __syncthreads();
  xl_fft_lds<N, B, NT>(buf, a.tw, tid);
  if constexpr (BLUE) {
    for (uint32_t q = tid; q < B * N; q += NT) buf[q] = xl_spec_blue_mid(buf[q], a.bspec[q % N]);
    __syncthreads();
    xl_fft_lds<N, B, NT>(buf, a.tw, tid);
  }
  for (uint32_t j = tid; j < a.W; j += NT) {
    const v2f cj = BLUE ? (v2f){a.chirp[j].x, a.chirp[j].y} : (v2f){1.0f, 0.0f};
    uint32_t cur = ~0u, m = 0u;
    for (uint32_t b = 0; b < B; ++b) {
      const uint32_t sl = slot[b];
      if (sl == ~0u) break;
      const float pw = xl_spec_power<BLUE>(buf[b * N + j], cj, a.norm);
      if (sl != cur) {
        if (cur != ~0u) atomicMax(a.rowmax + (size_t)cur * a.W + j, m);
        cur = sl;
        m = 0u;
      }
      const uint32_t bits = xl_spec_max_bits(pw);
      m = bits > m ? bits : m;
    }
    if (cur != ~0u) atomicMax(a.rowmax + (size_t)cur * a.W + j, m);
  }
}

// spectrogram.c:150-158: the bin that lands in column j after the halves of half = W / 2 are swapped (an odd W's last bin in place)
XL_DEV uint32_t xl_spec_shift_src(const uint32_t j, const uint32_t W) {
  const uint32_t half = W / 2u;
  return j < half ? j + half : (j < 2u * half ? j - half : j);
}

// spectrogram.c:150 and png_util.c:53-63 (the pixel) of a row maximum.  The dB is 10 * log10f(v) with the log10f the reference gets from
// its libm, the correctly rounded one.  The device's log10f is an ulp off here and there -- at v = 1e-20f, the floor every bin of a silent
// input sits on, it gives -20.000002 and so pixel 54 where the reference writes 55 -- so this one value per bin and finished row is taken
// in double and rounded once; the product is the float one.  The one definition: the narrow, bank, wide and wide-bank finishing passes.
XL_DEV float xl_spec_db(const float v) { return 10.0f * (float)log10((double)v); }
XL_DEV uint8_t xl_spec_pixel(const float d) {
  const float f = d + 255.0f;
  const int pixel = f >= 255.0f ? 255 : (f > 0.0f ? (int)f : 0);
  return (uint8_t)pixel;
}

// Column j (< W) of the finished row: the maximum of the bin that the half swap brings there, from the row slot at rowmax[s ..], as dB
// to db[o + j] and as a pixel to px[o + j]; the maximum is cleared for the row that reuses the slot (the swap is a permutation: every bin
// is read and cleared by exactly one thread)
XL_DEV void xl_spec_finish_bin(uint32_t *rowmax, float *db, uint8_t *px, const uint32_t W, const uint32_t j, const size_t s,
                               const size_t o) {
  const uint32_t from = xl_spec_shift_src(j, W);
  const float v = __uint_as_float(rowmax[s + from]);
  rowmax[s + from] = 0u;
  const float d = xl_spec_db(v);
  db[o + j] = d;
  px[o + j] = xl_spec_pixel(d);
}

// The transform lengths that have one-workgroup kernels (widths 1 .. 8192; wider ones: xl_spectrum_wide.hip): powers of two 1 .. 8192 as they are, 8 .. 16384 as Bluestein lengths; the three sample formats.
// launch(n, fmt, blue) gets them as std::integral_constants and enqueues its kernel<n, fmt, blue>.  0 or a hipError_t.
template <uint32_t N, bool BLUE, class Launch>
int xl_spec_dispatch_fmt(const int fmt, Launch &launch) {
  const std::integral_constant<uint32_t, N> n;
  const std::integral_constant<bool, BLUE> blue;
  if (fmt == XLF_CU8)
    launch(n, std::integral_constant<int, XLF_CU8>(), blue);
  else if (fmt == XLF_CS16)
    launch(n, std::integral_constant<int, XLF_CS16>(), blue);
  else
    launch(n, std::integral_constant<int, XLF_CF32>(), blue);
  return (int)hipGetLastError();
}

template <class Launch>
int xl_spec_dispatch(const uint32_t N, const bool bluestein, const int fmt, Launch launch) {
  if (bluestein) {
    switch (N) {
      case 8: return xl_spec_dispatch_fmt<8, true>(fmt, launch);
      case 16: return xl_spec_dispatch_fmt<16, true>(fmt, launch);
      case 32: return xl_spec_dispatch_fmt<32, true>(fmt, launch);
      case 64: return xl_spec_dispatch_fmt<64, true>(fmt, launch);
      case 128: return xl_spec_dispatch_fmt<128, true>(fmt, launch);
      case 256: return xl_spec_dispatch_fmt<256, true>(fmt, launch);
      case 512: return xl_spec_dispatch_fmt<512, true>(fmt, launch);
      case 1024: return xl_spec_dispatch_fmt<1024, true>(fmt, launch);
      case 2048: return xl_spec_dispatch_fmt<2048, true>(fmt, launch);
      case 4096: return xl_spec_dispatch_fmt<4096, true>(fmt, launch);
      case 8192: return xl_spec_dispatch_fmt<8192, true>(fmt, launch);
      case 16384: return xl_spec_dispatch_fmt<16384, true>(fmt, launch);
    }
    return (int)hipErrorInvalidValue;
  }
  switch (N) {
    case 1: return xl_spec_dispatch_fmt<1, false>(fmt, launch);
    case 2: return xl_spec_dispatch_fmt<2, false>(fmt, launch);
    case 4: return xl_spec_dispatch_fmt<4, false>(fmt, launch);
    case 8: return xl_spec_dispatch_fmt<8, false>(fmt, launch);
    case 16: return xl_spec_dispatch_fmt<16, false>(fmt, launch);
    case 32: return xl_spec_dispatch_fmt<32, false>(fmt, launch);
    case 64: return xl_spec_dispatch_fmt<64, false>(fmt, launch);
    case 128: return xl_spec_dispatch_fmt<128, false>(fmt, launch);
    case 256: return xl_spec_dispatch_fmt<256, false>(fmt, launch);
    case 512: return xl_spec_dispatch_fmt<512, false>(fmt, launch);
    case 1024: return xl_spec_dispatch_fmt<1024, false>(fmt, launch);
    case 2048: return xl_spec_dispatch_fmt<2048, false>(fmt, launch);
    case 4096: return xl_spec_dispatch_fmt<4096, false>(fmt, launch);
    case 8192: return xl_spec_dispatch_fmt<8192, false>(fmt, launch);
  }
  return (int)hipErrorInvalidValue;
}

}  // namespace

#endif  // XL_SPECTRUM_DEV_H_
