// xl_wide.hip -- the wide direct FIR: clients whose window image fits no LDS tile of xl_fir_kernel (xl_wide.h), e.g. the
// server's own filter at D > ~1075 (T ~ 12 D).  The work per input sample does not grow with D; what changes is its shape:
// few outputs per block (65 at D = 2000 per 131072 samples), each a T-long chain.
//
// Lane = one output of one client (blockIdx.y), 64 consecutive outputs per wave.  Taps are wave-uniform scalar loads (as in
// xl_fir_kernel); the window is read straight from global memory through L1 / L2 (lanes D samples apart, neighbouring
// outputs' windows overlap T / D ~ 12-fold), converted on the fly with xl_sample and masked like xl_stage_window: samples
// below zero_below (the client is younger than its window) or past the call's samples read as 0.
//   native    one wave per tile, every lane sums its taps strictly in index order with the roundings of XlAcc<0>;
//   optimized the tap range is split over `parts` waves of the workgroup (the chain is the latency), each summing like
//             XlAcc<1>; the partial sums are added in wave order through the LDS;
//   Q15       one wave per tile, the exact float64 sums of xl_fir_q15_batch_kernel.
// SCALAR FP32 ONLY: this file is compiled without the SLP vectoriser (Makefile: WIDE_FLAGS) and its accumulators are written
// as single-lane IEEE operations -- packed FP32 loses lanes 48..63 once in a while next to matrix instructions (xl_mixh.hip,
// DESIGN 3.6), and the wide launch runs in the same call as the engine's matrix-core launches.  The phase steps use the
// scalar xl_nco_role_step (the same IEEE operations as the packed step: bit-identical phases).
#include "xl_dev_inline.h"

// Samples s .. s + 3 of [in0 | in1] as cf32, zero below zb and past n0 + n1.  V16: cf32 in in0 only, s even, in0 16-byte
// aligned (the drop-in's work image at even D): two 16-byte loads when the four samples lie inside.
template <int FMT, bool V16>
XL_DEV void xl_wide_load4(const XlWideArgs &a, const uint32_t zb, const uint32_t s, v2f xs[4]) {
  if (V16 && s >= zb && s + 4u <= a.n0) {
    const v4f *__restrict__ p = reinterpret_cast<const v4f *>(reinterpret_cast<const v2f *>(a.in0) + s);
    const v4f q0 = p[0], q1 = p[1];
    xs[0] = (v2f){q0.x, q0.y};
    xs[1] = (v2f){q0.z, q0.w};
    xs[2] = (v2f){q1.x, q1.y};
    xs[3] = (v2f){q1.z, q1.w};
    return;
  }
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const uint32_t j = s + (uint32_t)u;
    const bool first = j < a.n0;
    const bool ok = j >= zb && (first || j - a.n0 < a.n1);
    const void *src = (first || !ok) ? a.in0 : a.in1;  // in0 always holds >= 1 sample: safe dummy address
    const v2f v = xl_sample(src, FMT, ok ? (first ? j : j - a.n0) : 0u);
    xs[u] = ok ? v : (v2f){0.0f, 0.0f};
  }
}

// the phase of output m: the tabulated one at m rounded down to the stride, stepped like xl_phase_walk
XL_DEV v2f xl_wide_phase(const XlWideArgs &a, const XlDyn &d, const uint32_t D, const uint32_t out_off, const v2f inc,
                         const uint32_t m) {
  XlBnd bnd;
  bnd.j0 = d.j0, bnd.D = D, bnd.S = a.pos.S, bnd.G = a.explicit_dyn ? 1u : a.pos.G, bnd.K = d.K, bnd.flags = a.pos.pad;
  v2f p = (reinterpret_cast<const v2f *>(a.phtab) + (out_off >> XL_PH_SHIFT))[m >> XL_PH_SHIFT];
  uint32_t j = m & ~(XL_PH_STRIDE - 1u);
  uint32_t nb = xl_bnd_next(bnd, j);
  for (; j < m; ++j) {
    p = xl_nco_role_step(p, inc, bnd.flags);
    if (j + 1u == nb) {
      p = xl_nco_renorm(p);
      nb = xl_bnd_next(bnd, j + 1u);
    }
  }
  return p;
}

template <int MODE, int FMT, bool V16>
__global__ __launch_bounds__(64 * XL_WIDE_PARTS_MAX) void xl_wide_kernel(const XlWideArgs a) {
  __shared__ float part_r[XL_WIDE_PARTS_MAX][64], part_i[XL_WIDE_PARTS_MAX][64];
  const cu32_p cd = (cu32_p)(uintptr_t)(a.clients + blockIdx.y);  // XlWideClient as dwords, scalar-loaded
  const uint32_t D = cd[0], T = cd[1], Tpad = cd[2], tap_off = cd[3], out_off = cd[5];
  const XlDyn d = a.explicit_dyn ? a.dyn1 : xl_grid_dyn_cap(D, T, cd[6], cd[7], a.pos, a.hcap);
  const uint32_t K = d.K;
  if (blockIdx.x * 64u >= K) return;  // (uniform over the workgroup: before any barrier)
  const uint32_t w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63u;
  const uint32_t m = blockIdx.x * 64u + lane;
  const uint32_t mm = m < K ? m : K - 1u;  // idle lanes walk a valid window (their sum is dropped)
  // this wave's share of the taps: [i0, i1), a multiple of the 4-tap step
  const uint32_t P = a.parts;
  const uint32_t share = ((Tpad / 4u + P - 1u) / P) * 4u;
  const uint32_t i0 = w * share < Tpad ? w * share : Tpad;
  const uint32_t i1 = i0 + share < Tpad ? i0 + share : Tpad;
  const uint32_t s0 = d.base + mm * D;
  const cfloat_p tp = (cfloat_p)(uintptr_t)(a.taps + tap_off);
  v2f v;
  if (MODE == 0) {
    // XlAcc<0>: pr = xr*hr - xi*hi, pi = xr*hi + xi*hr, s += (pr, pi); every operation rounded once, nothing fused
    float sr = 0.0f, si = 0.0f;
    for (uint32_t i = i0; i < i1; i += 4u) {
      v2f xs[4];
      xl_wide_load4<FMT, V16>(a, d.zero_below, s0 + i, xs);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const float hr = tp[2u * (i + u)], hi = tp[2u * (i + u) + 1u];
        const float p1x = xs[u].x * hr, p1y = xs[u].x * hi;
        const float p2x = xs[u].y * hi, p2y = xs[u].y * hr;
        sr = sr + (p1x - p2x);
        si = si + (p1y + p2y);
      }
    }
    v = (v2f){sr, si};
  } else {
    // XlAcc<1>: a += xr * (hr, hi), b += xi * (hi, hr), value = (a.x - b.x, a.y + b.y)
    float ax = 0.0f, ay = 0.0f, bx = 0.0f, by = 0.0f;
    for (uint32_t i = i0; i < i1; i += 4u) {
      v2f xs[4];
      xl_wide_load4<FMT, V16>(a, d.zero_below, s0 + i, xs);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const float hr = tp[2u * (i + u)], hi = tp[2u * (i + u) + 1u];
        ax = __builtin_fmaf(xs[u].x, hr, ax);
        ay = __builtin_fmaf(xs[u].x, hi, ay);
        bx = __builtin_fmaf(xs[u].y, hi, bx);
        by = __builtin_fmaf(xs[u].y, hr, by);
      }
    }
    float vr = ax - bx, vi = ay + by;
    if (P > 1u) {  // partial sums of the waves, added in wave order (as scalars: a v2f sum here becomes v_pk_add_f32)
      part_r[w][lane] = vr;
      part_i[w][lane] = vi;
      __syncthreads();
      if (w != 0u) return;
      for (uint32_t q = 1u; q < P; ++q) {
        vr = vr + part_r[q][lane];
        vi = vi + part_i[q][lane];
      }
    }
    v = (v2f){vr, vi};
  }
  if (m >= K) return;
  const v2f inc = {__builtin_bit_cast(float, cd[8]), __builtin_bit_cast(float, cd[9])};
  const v2f ph = xl_wide_phase(a, d, D, out_off, inc, m);
  reinterpret_cast<v2f *>(a.out)[out_off + m] = xl_rotate<MODE>(v, ph);
}

typedef const double __attribute__((address_space(4))) *cdouble_wp;

// Q15 family (xlating.c:100-129) per lane, as xl_fir_q15_batch_kernel: int16 x int16 products summed exactly in float64 FMAs,
// >> 15, cut to 32 bits, saturated (xl_q15_narrow.h), rotated by the truncating Q15 phase
template <int FMT>
__global__ __launch_bounds__(64) void xl_wide_q15_kernel(const XlWideArgs a) {
  const cu32_p cd = (cu32_p)(uintptr_t)(a.clients + blockIdx.y);
  const uint32_t D = cd[0], T = cd[1], qtap_off = cd[4], out_off = cd[5], qi = cd[10];
  const XlDyn d = xl_grid_dyn_cap(D, T, cd[6], cd[7], a.pos, a.hcap);
  const uint32_t K = d.K;
  if (blockIdx.x * 64u >= K) return;
  const uint32_t m = blockIdx.x * 64u + threadIdx.x;
  const uint32_t mm = m < K ? m : K - 1u;
  const uint32_t s0 = d.base + mm * D;
  const cdouble_wp tq = (cdouble_wp)(uintptr_t)(a.qtaps + (size_t)qtap_off * 2u);
  double accr = 0.0, acci = 0.0;
  for (uint32_t i = 0; i < T; ++i) {
    const uint32_t j = s0 + i;
    const bool first = j < a.n0;
    const bool ok = j >= d.zero_below && (first || j - a.n0 < a.n1);
    const v2f xs0 = xl_sample_q15((first || !ok) ? a.in0 : a.in1, FMT, ok ? (first ? j : j - a.n0) : 0u);
    const v2f xs = ok ? xs0 : (v2f){0.0f, 0.0f};
    const double xr = (double)xs.x, xi = (double)xs.y;
    const double hr = tq[2u * i], hi = tq[2u * i + 1u];
    accr = __builtin_fma(xr, hr, accr);  // temp_real += ar * br - ai * bi   (xlating.c:114)
    accr = __builtin_fma(-xi, hi, accr);
    acci = __builtin_fma(xr, hi, acci);  // temp_imag += ar * bi + ai * br   (:115)
    acci = __builtin_fma(xi, hr, acci);
  }
  if (m >= K) return;
  const int32_t ar = xl_q15_narrow_sum(accr);  // (xlating.c:118-119; xl_q15_narrow.h)
  const int32_t ai = xl_q15_narrow_sum(acci);
  const short2 p0 = a.qphtab[(out_off >> XL_PH_SHIFT) + (m >> XL_PH_SHIFT)];
  const int32_t ir = (int16_t)(qi & 0xFFFFu), ii = (int16_t)(qi >> 16);
  int32_t pr = p0.x, pi = p0.y;
  for (uint32_t j = m & (XL_PH_STRIDE - 1u); j > 0u; --j) {
    const int32_t tr = pr * ir - pi * ii, ti = pr * ii + pi * ir;
    pr = xl_sat16(tr >> 15);
    pi = xl_sat16(ti >> 15);
  }
  const int32_t orr = ar * pr - ai * pi, oi = ar * pi + ai * pr;  // xlating.c:121-124
  reinterpret_cast<short2 *>(a.out + out_off)[m] = make_short2((short)xl_sat16(orr >> 15), (short)xl_sat16(oi >> 15));
}

uint32_t xl_wide_parts(uint32_t tpad) {
  const uint32_t p = (tpad + 1023u) / 1024u;  // ~1000 taps per wave
  return p < 1u ? 1u : (p > XL_WIDE_PARTS_MAX ? XL_WIDE_PARTS_MAX : p);
}

template <int MODE, int FMT>
static hipError_t xl_wide_go(const XlWideArgs &a, hipStream_t s) {
  const dim3 grid(a.xtiles, a.nclients);
  const dim3 block(64u * (MODE == 1 ? a.parts : 1u));
  if (FMT == XLF_CF32 && (a.flags & 1u) && a.n1 == 0u && ((uintptr_t)a.in0 & 15u) == 0u) {
    hipLaunchKernelGGL((xl_wide_kernel<MODE, FMT, true>), grid, block, 0, s, a);
    return hipGetLastError();
  }
  hipLaunchKernelGGL((xl_wide_kernel<MODE, FMT, false>), grid, block, 0, s, a);
  return hipGetLastError();
}

template <int MODE>
static hipError_t xl_wide_fmt(const XlWideArgs &a, hipStream_t s) {
  switch (a.fmt) {
    case XLF_CU8: return xl_wide_go<MODE, XLF_CU8>(a, s);
    case XLF_CS8: return xl_wide_go<MODE, XLF_CS8>(a, s);
    case XLF_CS16: return xl_wide_go<MODE, XLF_CS16>(a, s);
    case XLF_CF32: return xl_wide_go<MODE, XLF_CF32>(a, s);
    default: return hipErrorInvalidValue;
  }
}

hipError_t xl_launch_wide(int mode, const XlWideArgs &a, hipStream_t s) {
  if (a.nclients == 0u || a.xtiles == 0u) return hipSuccess;
  if (a.parts < 1u || a.parts > XL_WIDE_PARTS_MAX || (mode != 1 && a.parts != 1u)) return hipErrorInvalidValue;
  if (mode == 0) return xl_wide_fmt<0>(a, s);
  if (mode == 1) return xl_wide_fmt<1>(a, s);
  if (mode != 2 || a.explicit_dyn) return hipErrorInvalidValue;
  const dim3 grid(a.xtiles, a.nclients);
  switch (a.fmt) {
    case XLF_CU8: hipLaunchKernelGGL(xl_wide_q15_kernel<XLF_CU8>, grid, dim3(64), 0, s, a); break;
    case XLF_CS8: hipLaunchKernelGGL(xl_wide_q15_kernel<XLF_CS8>, grid, dim3(64), 0, s, a); break;
    case XLF_CS16: hipLaunchKernelGGL(xl_wide_q15_kernel<XLF_CS16>, grid, dim3(64), 0, s, a); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}
