// xl_resample.hip -- the resampler bank's kernels (include/xlating_resample.h): the new outputs of MANY streams, each of its own
// ratio L / M and tap table, in one ragged launch, and the carries of all streams in one launch behind it.
//
// The ragged launch: the host writes one run per stream (XlRsRun) with the running sum of workgroups; a workgroup finds its run by
// binary search (as xl_bank_kernel finds a transform's) and computes a tile of XL_RS_TILE consecutive outputs of that ONE stream, one
// output per thread.  Output k of the run sits at t = p0 + k * M on the grid of the input upsampled by L; with M = Mq * L + Mr a
// thread's position inside the tile needs 32-bit arithmetic only (tid * Mr < 2^20), the tile's own position one 64-bit division.
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
#include "xl_resample.h"

namespace {

__global__ void __launch_bounds__(XL_RS_TILE) xl_rs_kernel(const XlRsRun *__restrict__ runs, const uint32_t nruns) {
  __shared__ float2 win[XL_RS_LDS_SPAN];
  const uint32_t w = blockIdx.x, tid = threadIdx.x;
  uint32_t lo = 0u, hi = nruns;  // the last run with wsum <= w (runs[0].wsum == 0; a run without outputs shares its successor's wsum)
  while (hi - lo > 1u) {
    const uint32_t mid = (lo + hi) / 2u;
    if (runs[mid].wsum <= w) lo = mid; else hi = mid;
  }
  const XlRsRun r = runs[lo];
  const uint32_t k0 = (w - r.wsum) * XL_RS_TILE;  // the tile's first output; < nout < 2^31
  if (k0 >= r.nout) return;                       // (never: the host counts the workgroups from nout)
  const uint32_t nv = min(XL_RS_TILE, r.nout - k0);
  const uint32_t K = r.Q - 1u;
  // the tile's first output: input nt (relative to src, 0 <= nt < cnt), phase pt
  const uint64_t t0 = (uint64_t)r.p0 + (uint64_t)k0 * r.M;
  const int32_t nt = r.n0 + (int32_t)(t0 / r.L);
  const uint32_t pt = (uint32_t)(t0 % r.L);
  const uint32_t Mq = r.M / r.L, Mr = r.M % r.L;
  // this thread's output: input nt + dn, phase p (dn wraps harmlessly in a thread past the tile's outputs, which computes nothing)
  const uint32_t u = pt + tid * Mr;
  const uint32_t dn = tid * Mq + u / r.L;
  const uint32_t p = u % r.L;
  // the window: inputs nt - K .. nt + dn of the tile's last output
  const uint32_t ul = pt + (nv - 1u) * Mr;
  const uint64_t span = (uint64_t)(nv - 1u) * Mq + ul / r.L + r.Q;
  const float *__restrict__ h = r.table + (size_t)p * r.Q;
  float2 acc = make_float2(0.0f, 0.0f);
  if (span <= XL_RS_LDS_SPAN) {
    const int32_t first = nt - (int32_t)K;
    for (uint32_t i = tid; i < (uint32_t)span; i += XL_RS_TILE) {
      const int32_t idx = first + (int32_t)i;
      win[i] = idx < 0 ? r.carry[(int32_t)K + idx] : r.src[idx];
    }
    __syncthreads();
    if (tid >= nv) return;
    const uint32_t base = dn + K;
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
    if (tid >= nv) return;
    const int32_t n = nt + (int32_t)dn;
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
  r.out[k0 + tid] = acc;
}

// one workgroup per stream of the feed: carry = concat(carry, src[0 .. cnt))[-(Q - 1):].  A feed shorter than the carry shifts it,
// and the move overlaps itself: every thread reads its (up to four) samples, the workgroup meets, then they are written.
__global__ void __launch_bounds__(256) xl_rs_carry_kernel(const XlRsRun *__restrict__ runs) {
  const XlRsRun r = runs[blockIdx.x];
  const uint32_t K = r.Q - 1u;
  if (K == 0u || r.cnt == 0u) return;
  float2 v[XL_RS_CARRY_SLOT / 256u];
#pragma unroll
  for (uint32_t j = 0u; j < XL_RS_CARRY_SLOT / 256u; ++j) {
    const uint32_t i = threadIdx.x + j * 256u;
    if (i < K) {
      const uint64_t s = (uint64_t)i + r.cnt;  // position in concat(carry, src)
      v[j] = s < K ? r.carry[s] : r.src[s - K];
    }
  }
  __syncthreads();
#pragma unroll
  for (uint32_t j = 0u; j < XL_RS_CARRY_SLOT / 256u; ++j) {
    const uint32_t i = threadIdx.x + j * 256u;
    if (i < K) r.carry[i] = v[j];
  }
}

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
