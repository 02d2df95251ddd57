// xl_resample_q15.hip -- the Q15 resampler bank's kernels (include/xlating_resample_q15.h): the new outputs of MANY int16-pair streams,
// each of its own ratio L / M and tap table, in one ragged launch, and the carries of all streams in one launch behind it.
//
// The scheme is xl_resample.hip's: the host writes one run per stream (XlRsQ15Run) with the running sum of workgroups; a workgroup
// finds its run by binary search and computes a tile of XL_RS_TILE consecutive outputs of that ONE stream, one output per thread, at
// t = p0 + k * M on the grid of the input upsampled by L (xl_resample_dev.h: xl_rs_tile, and the carry launch's body, are shared).
// A tile's outputs read the inputs n_first - (Q - 1) .. n_last.  When that window fits XL_RSQ_LDS_SPAN it is staged in LDS once -- the
// part below the feed's first sample from the stream's carry -- one 32-bit word per sample (re low, im high); a wider window (a
// decimating stream of large M / L) is read in place.
//
// What the integer arithmetic allows beside that, because the sum is exact in any arrangement:
//   - the tap table is int16, and one of up to XL_RSQ_LDS_TAPS entries (the admitted second stages: 3 / 5 is 63 entries, 147 / 160 is
//     2058) is staged in LDS beside the window, copied as 32-bit words: a thread's Q taps are then LDS reads, not Q dependent reads
//     of a table in global memory.  A larger table is read in place, Q contiguous int16 per output.
//   - a run whose every phase has sum |c| <= 65535 (the host checks it once per table) sums in 32 bits: |s| <= 65535 * 32768 < 2^31.
//     A run flagged XL_RSQ_WIDE sums in 64 bits.  The products are 32-bit either way (|c|, |x| <= 2^15).
// 24 KiB of LDS per workgroup: six workgroups per CU.
// INTEGER VALU ONLY, no matrix instructions and no packed FP32 (Makefile: RESAMPLE_Q15_FLAGS): these launches run behind and beside
// the engine's matrix-core launches.
#include "xl_resample_dev.h"
#include "xl_resample_q15.h"

namespace {

__device__ __forceinline__ int32_t xl_rsq_sat16(const int32_t v) { return min(max(v, -32768), 32767); }
__device__ __forceinline__ int32_t xl_rsq_sat16(const int64_t v) {
  return (int32_t)(v < -32768 ? (int64_t)-32768 : (v > 32767 ? (int64_t)32767 : v));
}

// y = sat16(sum_q h(q) * x(q) >> 15), re and im separately; Acc is the run's proven accumulator
template <typename Acc, typename H, typename X>
__device__ __forceinline__ xl_cs16 xl_rsq_sum(const uint32_t Q, const H h, const X x) {
  Acc re = 0, im = 0;
  for (uint32_t q = 0u; q < Q; ++q) {
    const int32_t c = h(q);
    const xl_cs16 v = x(q);
    re += (Acc)(c * (int32_t)(int16_t)(v & 0xFFFFu));
    im += (Acc)(c * ((int32_t)v >> 16));
  }
  const uint32_t yr = (uint32_t)xl_rsq_sat16(re >> 15) & 0xFFFFu;  // (>> of a negative value: arithmetic, the floor)
  const uint32_t yi = (uint32_t)xl_rsq_sat16(im >> 15) & 0xFFFFu;
  return yr | (yi << 16);
}

template <typename H, typename X>
__device__ __forceinline__ xl_cs16 xl_rsq_out(const bool wide, const uint32_t Q, const H h, const X x) {
  return wide ? xl_rsq_sum<int64_t>(Q, h, x) : xl_rsq_sum<int32_t>(Q, h, x);
}

__global__ void __launch_bounds__(XL_RS_TILE) xl_rsq_kernel(const XlRsQ15Run *__restrict__ runs, const uint32_t nruns) {
  __shared__ xl_cs16 win[XL_RSQ_LDS_SPAN];
  __shared__ uint32_t tapw[XL_RSQ_LDS_TAPS / 2u];
  const uint32_t tid = threadIdx.x;
  XlRsQ15Run r;
  XlRsTile t;
  if (!xl_rs_tile(runs, nruns, r, t)) return;
  const uint32_t K = t.K;
  const bool wide = (r.flags & XL_RSQ_WIDE) != 0u;
  const uint32_t ntaps = r.L * r.Q;  // <= 4096 * 1024
  const bool taps_lds = ntaps <= XL_RSQ_LDS_TAPS && (r.flags & XL_RSQ_TAPS_IN_PLACE) == 0u;
  const bool win_lds = t.span <= XL_RSQ_LDS_SPAN;
  // (all three are the same in every thread of the workgroup: the barrier below is met by all or by none)
  if (taps_lds) {
    const uint32_t *__restrict__ tw = reinterpret_cast<const uint32_t *>(r.table);  // (padded to whole words by the host)
    for (uint32_t i = tid; i < (ntaps + 1u) / 2u; i += XL_RS_TILE) tapw[i] = tw[i];
  }
  if (win_lds) {
    const int32_t first = t.nt - (int32_t)K;
    for (uint32_t i = tid; i < (uint32_t)t.span; i += XL_RS_TILE) {
      const int32_t idx = first + (int32_t)i;
      win[i] = idx < 0 ? r.carry[(int32_t)K + idx] : r.src[idx];
    }
  }
  if (taps_lds || win_lds) __syncthreads();
  if (tid >= t.nv) return;
  const int16_t *taps = reinterpret_cast<const int16_t *>(tapw) + t.p * r.Q;
  const int16_t *__restrict__ tapg = r.table + (size_t)t.p * r.Q;
  const auto h_lds = [&](const uint32_t q) -> int32_t { return taps[q]; };
  const auto h_mem = [&](const uint32_t q) -> int32_t { return tapg[q]; };
  xl_cs16 y;
  if (win_lds) {
    const uint32_t base = t.dn + K;
    const auto x = [&](const uint32_t q) -> xl_cs16 { return win[base - q]; };
    y = taps_lds ? xl_rsq_out(wide, r.Q, h_lds, x) : xl_rsq_out(wide, r.Q, h_mem, x);
  } else {
    const int32_t n = t.nt + (int32_t)t.dn;
    const auto x = [&](const uint32_t q) -> xl_cs16 {
      const int32_t idx = n - (int32_t)q;
      return idx < 0 ? r.carry[(int32_t)K + idx] : r.src[idx];
    };
    y = taps_lds ? xl_rsq_out(wide, r.Q, h_lds, x) : xl_rsq_out(wide, r.Q, h_mem, x);
  }
  r.out[t.k0 + tid] = y;
}

// one workgroup per stream of the feed (xl_resample_dev.h), with 4-byte samples
__global__ void __launch_bounds__(256) xl_rsq_carry_kernel(const XlRsQ15Run *__restrict__ runs) {
  xl_rs_carry_body<XlRsQ15Run, xl_cs16>(runs);
}

}  // namespace

int xl_rsq_launch(const XlRsQ15Run *runs, uint32_t nruns, uint32_t W, hipStream_t st) {
  if (W == 0u || nruns == 0u) return 0;
  hipLaunchKernelGGL(xl_rsq_kernel, dim3(W), dim3(XL_RS_TILE), 0, st, runs, nruns);
  return (int)hipGetLastError();
}

int xl_rsq_carry(const XlRsQ15Run *runs, uint32_t nruns, hipStream_t st) {
  if (nruns == 0u) return 0;
  hipLaunchKernelGGL(xl_rsq_carry_kernel, dim3(nruns), dim3(256), 0, st, runs);
  return (int)hipGetLastError();
}
