// xl_resample.hip -- the resampler bank's kernels (include/xlating_resample.h): the new outputs of MANY streams, each of its own
// ratio L / M and tap table, in one ragged launch, and the carries of all streams in one launch behind it.
//
// The ragged launch: the host writes one run per stream (XlRsRun) with the running sum of workgroups; a workgroup finds its run by
// binary search (xl_ragged.h) and computes a tile of XL_RS_TILE consecutive outputs of that ONE stream, one output per thread: where
// the tile and the thread's output lie is xl_resample_dev.h's xl_rs_tile, which the Q15 bank's kernel calls too.
// A tile's outputs read the inputs n_first - (Q - 1) .. n_last: a window of (n_last - n_first) + Q samples, about TILE * M / L + Q.
// When it fits XL_RS_LDS_SPAN it is staged in LDS once -- the part below the feed's first sample from the stream's carry -- and the
// dot products read neighbouring LDS addresses (consecutive outputs are M / L inputs apart: for the ratios near 1 the bank exists
// for, a wave reads a contiguous stretch).  A wider window (a decimating stream of large M / L, where windows of neighbouring outputs
// barely overlap) is read in place.  32 KiB of LDS per workgroup: five workgroups per CU.
// The taps are read from the phase-major table: Q contiguous floats per output.
//
// The sum is the definition's: q = 0 .. Q - 1 in order, one multiplication and one addition per term and component, nothing fused
// (-ffp-contract=off), starting at the first product -- bit-identical wherever a tile or a feed boundary falls.
// SCALAR FP32 ONLY, no matrix instructions (Makefile: RESAMPLE_FLAGS): these launches run behind and beside the engine's
// matrix-core launches.
#include "xl_resample_dev.h"

namespace {

__global__ void __launch_bounds__(XL_RS_TILE) xl_rs_kernel(const XlRsRun *__restrict__ runs, const uint32_t nruns) {
  __shared__ float2 win[XL_RS_LDS_SPAN];
  const uint32_t tid = threadIdx.x;
  XlRsRun r;
  XlRsTile t;
  if (!xl_rs_tile(runs, nruns, r, t)) return;
  const uint32_t K = t.K;
  const float *__restrict__ h = r.table + (size_t)t.p * r.Q;
  float2 acc = make_float2(0.0f, 0.0f);
  if (t.span <= XL_RS_LDS_SPAN) {
    const int32_t first = t.nt - (int32_t)K;
    for (uint32_t i = tid; i < (uint32_t)t.span; i += XL_RS_TILE) {
      const int32_t idx = first + (int32_t)i;
      win[i] = idx < 0 ? r.carry[(int32_t)K + idx] : r.src[idx];
    }
    __syncthreads();
    if (tid >= t.nv) return;
    const uint32_t base = t.dn + K;
    {
      const float2 x = win[base];
      const float c = h[0];
      acc.x = c * x.x, acc.y = c * x.y;
    }
    for (uint32_t q = 1u; q < r.Q; ++q) {
      const float2 x = win[base - q];
      const float c = h[q];
      acc.x = acc.x + c * x.x;
      acc.y = acc.y + c * x.y;
    }
  } else {
    if (tid >= t.nv) return;
    const int32_t n = t.nt + (int32_t)t.dn;
    {
      const float2 x = r.src[n];
      const float c = h[0];
      acc.x = c * x.x, acc.y = c * x.y;
    }
    for (uint32_t q = 1u; q < r.Q; ++q) {
      const int32_t idx = n - (int32_t)q;
      const float2 x = idx < 0 ? r.carry[(int32_t)K + idx] : r.src[idx];
      const float c = h[q];
      acc.x = acc.x + c * x.x;
      acc.y = acc.y + c * x.y;
    }
  }
  r.out[t.k0 + tid] = acc;
}

// one workgroup per stream of the feed (xl_resample_dev.h)
__global__ void __launch_bounds__(256) xl_rs_carry_kernel(const XlRsRun *__restrict__ runs) { xl_rs_carry_body<XlRsRun, float2>(runs); }

}  // namespace

int xl_rs_launch(const XlRsRun *runs, uint32_t nruns, uint32_t W, hipStream_t st) {
  if (W == 0u || nruns == 0u) return 0;
  hipLaunchKernelGGL(xl_rs_kernel, dim3(W), dim3(XL_RS_TILE), 0, st, runs, nruns);
  return (int)hipGetLastError();
}

int xl_rs_carry(const XlRsRun *runs, uint32_t nruns, hipStream_t st) {
  if (nruns == 0u) return 0;
  hipLaunchKernelGGL(xl_rs_carry_kernel, dim3(nruns), dim3(256), 0, st, runs);
  return (int)hipGetLastError();
}
