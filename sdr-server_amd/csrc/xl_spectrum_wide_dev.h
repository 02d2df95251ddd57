// xl_spectrum_wide_dev.h -- what a workgroup of the two-level transform (widths above 8192) does in each of its three passes once it
// knows where its transform comes from, shared by the single object's kernels (xl_spectrum_wide.hip) and the bank's ragged kernels
// (xl_spectrum_bank_wide.hip), as xl_spectrum_dev.h is shared by the one-workgroup kernels.  A kernel of either file is its LDS, its own
// prologue -- transform t of the launch: which source buffer, which sample offset, which row slot, which slot of the scratch -- and one
// call; both files are compiled with the same flags (Makefile: SPEC_FLAGS, -ffp-contract=off): a row of the wide bank is bit for bit the
// row of the single wide object.  Also here: the finishing of one column of a wide row (xl_specw_finish_col, with xl_spec_db) and the
// list of the transform lengths that have kernels (xl_specw_dispatch).  See xl_spectrum_wide.hip's header for the method.
#ifndef XL_SPECTRUM_WIDE_DEV_H_
#define XL_SPECTRUM_WIDE_DEV_H_

#include "xl_spectrum_dev.h"
#include "xl_spectrum_wide_plan.h"

namespace {

constexpr uint32_t XL_SPECW_COL_NT = 256;  // xl_spec_nt of a 4096-point pack
constexpr uint32_t xl_specw_pack(uint32_t N1) { return XL_SPECW_PACK_POINTS / N1; }  // adjacent columns per workgroup of a column pass

// Column pass, input side: columns j0 .. j0 + pack - 1 of the transform whose sample 0 is element `off` of `in`; N1-point transforms,
// times w_N^(j2 k1), to out[k1][j2] (the transform's slot of the scratch) in runs of `pack`.
template <uint32_t N1, uint32_t N2, int FMT, bool BLUE>
XL_DEV void xl_specw_col_in(v2f *buf, const void *__restrict__ in, const uint32_t off, const uint32_t j0, float2 *out, const uint32_t W,
                            const float2 *chirp, const float2 *tw1, const float2 *tw) {
  constexpr uint32_t B = xl_specw_pack(N1), P = XL_SPECW_PACK_POINTS, NT = XL_SPECW_COL_NT;
  static_assert(xl_spec_b(N1) == B && xl_spec_nt(N1) == NT, "a column pack is an xl_fft_lds pack");
  const uint32_t tid = threadIdx.x;
  for (uint32_t q = tid; q < P; q += NT) {
    const uint32_t c = q % B, n1 = q / B, n = n1 * N2 + j0 + c;
    v2f v = (v2f){0.0f, 0.0f};
    if (n < W) v = xl_spec_point<FMT, BLUE>(in, off, n, chirp);
    buf[c * N1 + n1] = v;
  }
  __syncthreads();
  xl_fft_lds<N1, B, NT>(buf, tw1, tid);
  for (uint32_t q = tid; q < P; q += NT) {
    const uint32_t c = q % B, k1 = q / B, j2 = j0 + c;
    const float2 t = tw[j2 * k1];
    const v2f v = cmul(buf[c * N1 + k1], (v2f){t.x, t.y});
    out[k1 * N2 + j2] = make_float2(v.x, v.y);
  }
}

// Row pass: rows k10 .. k10 + xl_spec_b(N2) - 1 of one transform, contiguous at `row` in its slot of the scratch.  Plain: N2-point
// transforms, power, maximum into mx()[0 ..] (the row slot's maxima from position k10 * N2 on; mx is only called here).  Bluestein:
// transform, conj(. Bs), transform, times w_N^(k1 m2), back in place.
template <uint32_t N1, uint32_t N2, bool BLUE, class Max>
XL_DEV void xl_specw_row(v2f *buf, float2 *row, const uint32_t k10, const float2 *bspec, const float2 *tw2, const float2 *tw, const float norm,
                         const Max mx) {
  constexpr uint32_t B = xl_spec_b(N2), NT = xl_spec_nt(N2), P = B * N2;
  static_assert(N1 % B == 0, "a pack of rows stays inside one transform");
  const uint32_t tid = threadIdx.x;
  for (uint32_t q = tid; q < P; q += NT) {
    const float2 v = row[q];
    buf[q] = (v2f){v.x, v.y};
  }
  __syncthreads();
  xl_fft_lds<N2, B, NT>(buf, tw2, tid);
  if constexpr (BLUE) {
    const float2 *bs = bspec + (size_t)k10 * N2;
    for (uint32_t q = tid; q < P; q += NT) buf[q] = xl_spec_blue_mid(buf[q], bs[q]);
    __syncthreads();
    xl_fft_lds<N2, B, NT>(buf, tw2, tid);
    for (uint32_t q = tid; q < P; q += NT) {
      const uint32_t k1 = k10 + q / N2, m2 = q % N2;
      const float2 t = tw[k1 * m2];
      const v2f v = cmul(buf[q], (v2f){t.x, t.y});
      row[q] = make_float2(v.x, v.y);
    }
  } else {
    uint32_t *m = mx();
    for (uint32_t q = tid; q < P; q += NT) {
      const float pw = xl_spec_power<false>(buf[q], (v2f){1.0f, 0.0f}, norm);
      atomicMax(m + q, xl_spec_max_bits(pw));
    }
  }
}

// Column pass, output side (Bluestein): columns m0 .. m0 + pack - 1 of the transform at `in` (its slot of the scratch); N1-point
// transforms, X[m] = c[m] conj(.), the power of bins m < W, maximum into mx[m] (the row slot's maxima), natural bin order.
template <uint32_t N1, uint32_t N2>
XL_DEV void xl_specw_col_out(v2f *buf, const float2 *in, const uint32_t m0, uint32_t *mx, const uint32_t W, const float2 *chirp,
                             const float2 *tw1, const float norm) {
  constexpr uint32_t B = xl_specw_pack(N1), P = XL_SPECW_PACK_POINTS, NT = XL_SPECW_COL_NT;
  const uint32_t tid = threadIdx.x;
  for (uint32_t q = tid; q < P; q += NT) {
    const uint32_t c = q % B, k1 = q / B;
    const float2 v = in[k1 * N2 + m0 + c];
    buf[c * N1 + k1] = (v2f){v.x, v.y};
  }
  __syncthreads();
  xl_fft_lds<N1, B, NT>(buf, tw1, tid);
  for (uint32_t q = tid; q < P; q += NT) {
    const uint32_t c = q % B, m1 = q / B, m = m1 * N2 + m0 + c;
    if (m < W) {
      const float2 cj = chirp[m];
      const float pw = xl_spec_power<true>(buf[c * N1 + m1], (v2f){cj.x, cj.y}, norm);
      atomicMax(mx + m, xl_spec_max_bits(pw));
    }
  }
}

// Column j of a finished wide row: the maximum at position `from` of the row slot at rowmax[s ..] (the caller's bin order: a plain
// width's xl_specw_col_pos, else the half swap) as dB to db[o + j] and as a pixel to px[o + j]; cleared for the row that reuses the slot
// (either order is a permutation of the slot: every bin is read and cleared by exactly one thread)
XL_DEV void xl_specw_finish_col(uint32_t *rowmax, float *db, uint8_t *px, const size_t s, const uint32_t from, const size_t o,
                                const uint32_t j) {
  const float v = __uint_as_float(rowmax[s + from]);
  rowmax[s + from] = 0u;
  const float d = xl_spec_db(v);
  db[o + j] = d;
  px[o + j] = xl_spec_pixel(d);
}

// The transform lengths that have two-level kernels: 2^14 .. 2^20 as they are, 2^15 .. 2^21 as Bluestein lengths.  launch(n, blue) gets
// them as std::integral_constants, enqueues its passes and returns 0 or a hipError_t.
template <class Launch>
int xl_specw_dispatch(const uint32_t N, const bool bluestein, Launch launch) {
  const std::true_type blue;
  const std::false_type plain;
  if (bluestein) {
    switch (N) {
      case 1u << 15: return launch(std::integral_constant<uint32_t, (1u << 15)>(), blue);
      case 1u << 16: return launch(std::integral_constant<uint32_t, (1u << 16)>(), blue);
      case 1u << 17: return launch(std::integral_constant<uint32_t, (1u << 17)>(), blue);
      case 1u << 18: return launch(std::integral_constant<uint32_t, (1u << 18)>(), blue);
      case 1u << 19: return launch(std::integral_constant<uint32_t, (1u << 19)>(), blue);
      case 1u << 20: return launch(std::integral_constant<uint32_t, (1u << 20)>(), blue);
      case 1u << 21: return launch(std::integral_constant<uint32_t, (1u << 21)>(), blue);
    }
    return (int)hipErrorInvalidValue;
  }
  switch (N) {
    case 1u << 14: return launch(std::integral_constant<uint32_t, (1u << 14)>(), plain);
    case 1u << 15: return launch(std::integral_constant<uint32_t, (1u << 15)>(), plain);
    case 1u << 16: return launch(std::integral_constant<uint32_t, (1u << 16)>(), plain);
    case 1u << 17: return launch(std::integral_constant<uint32_t, (1u << 17)>(), plain);
    case 1u << 18: return launch(std::integral_constant<uint32_t, (1u << 18)>(), plain);
    case 1u << 19: return launch(std::integral_constant<uint32_t, (1u << 19)>(), plain);
    case 1u << 20: return launch(std::integral_constant<uint32_t, (1u << 20)>(), plain);
  }
  return (int)hipErrorInvalidValue;
}

}  // namespace

#endif  // XL_SPECTRUM_WIDE_DEV_H_
