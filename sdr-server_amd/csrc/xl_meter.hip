// xl_meter.hip -- the power meter's kernels (include/xlating_meter.h): the mean power of MANY rows of one format in one ragged launch.
//
// The host writes one run per row (XlMeterRun) with the running sum of workgroups; a workgroup finds its run by binary search
// (xl_ragged.h) and measures XL_METER_PIECE consecutive samples of that ONE row.  A thread takes XL_METER_PER_THREAD samples,
// XL_METER_THREADS apart (a wave reads 512 contiguous bytes of a cf32 row at a time), all loads in flight before the first sum; the lane
// sums meet by cross-lane moves at strides 32 .. 1, the four wave sums through 32 bytes of LDS, and thread 0 stores the piece's partial.
// The order of every float32 addition is xl_meter_rule.h's and is the contract; the cs16 sums are integers and have no order.
// Memory-bound: one read of the rows, 8 bytes written per 2048 samples.  The rows are never written.
// SCALAR FP32 ONLY, nothing fused (-ffp-contract=off), no matrix instructions, no scratch (Makefile: METER_FLAGS;
// tests/test_meter_cpu.py reads the code object): the launch runs behind and beside the engine's matrix-core launches.
#include "xl_meter.h"

#include "xl_meter_rule.h"
#include "xl_ragged.h"

namespace {

// (global address space stated: an address that comes out of a table would otherwise be loaded through the flat path)
typedef float XlMeterF2 __attribute__((ext_vector_type(2)));
typedef const XlMeterF2 __attribute__((address_space(1))) *XlMeterSrcF;
typedef const uint32_t __attribute__((address_space(1))) *XlMeterSrcQ;
typedef uint64_t __attribute__((address_space(1))) *XlMeterDst;

__global__ void __launch_bounds__(XL_METER_THREADS) xl_meter_cf32_kernel(const XlMeterRun *__restrict__ runs, const uint32_t nruns,
                                                                          uint64_t *__restrict__ partials) {
  __shared__ float waves[XL_METER_THREADS / 64u];
  const uint32_t w = blockIdx.x, tid = threadIdx.x;
  const uint32_t k = xl_ragged_find(runs, nruns, w, [](const XlMeterRun &r) { return r.wsum; });
  const XlMeterRun r = runs[k];  // (uniform)
  const uint32_t j0 = (w - r.wsum) * XL_METER_PIECE + tid;
  const XlMeterSrcF src = (XlMeterSrcF)(uintptr_t)r.src;
  XlMeterF2 x[XL_METER_PER_THREAD];
#pragma unroll
  for (uint32_t i = 0; i < XL_METER_PER_THREAD; ++i) {
    const uint32_t j = j0 + i * XL_METER_THREADS;
    x[i] = j < r.cnt ? src[j] : XlMeterF2{0.0f, 0.0f};
  }
  // (re and im pass through an empty statement each: the two squares of a loaded pair are otherwise joined into one packed FP32
  // multiply, whatever the vectoriser flags say)
  float p[XL_METER_PER_THREAD];
#pragma unroll
  for (uint32_t i = 0; i < XL_METER_PER_THREAD; ++i) {
    float re = x[i].x, im = x[i].y;
    asm("" : "+v"(re));
    asm("" : "+v"(im));
    p[i] = xl_meter_p_cf32(re, im);
  }
  float s = p[0];
#pragma unroll
  for (uint32_t i = 1; i < XL_METER_PER_THREAD; ++i) s = xl_meter_add(s, p[i]);
  // s[i] <- s[i] + s[i + stride], i < stride (the lanes at and above the stride add what nobody reads)
#pragma unroll
  for (uint32_t stride = 32u; stride >= 1u; stride >>= 1) s = xl_meter_add(s, __shfl_down(s, stride, 64));
  if ((tid & 63u) == 0u) waves[tid >> 6] = s;
  __syncthreads();
  if (tid == 0u) {
    const float p = xl_meter_waves(waves[0], waves[1], waves[2], waves[3]);
    ((XlMeterDst)(uintptr_t)partials)[w] = (uint64_t)__float_as_uint(p);
  }
}

__global__ void __launch_bounds__(XL_METER_THREADS) xl_meter_cs16_kernel(const XlMeterRun *__restrict__ runs, const uint32_t nruns,
                                                                          uint64_t *__restrict__ partials) {
  __shared__ uint64_t waves[XL_METER_THREADS / 64u];
  const uint32_t w = blockIdx.x, tid = threadIdx.x;
  const uint32_t k = xl_ragged_find(runs, nruns, w, [](const XlMeterRun &r) { return r.wsum; });
  const XlMeterRun r = runs[k];  // (uniform)
  const uint32_t j0 = (w - r.wsum) * XL_METER_PIECE + tid;
  const XlMeterSrcQ src = (XlMeterSrcQ)(uintptr_t)r.src;
  uint32_t x[XL_METER_PER_THREAD];
#pragma unroll
  for (uint32_t i = 0; i < XL_METER_PER_THREAD; ++i) {
    const uint32_t j = j0 + i * XL_METER_THREADS;
    x[i] = j < r.cnt ? src[j] : 0u;
  }
  uint64_t s = 0u;
#pragma unroll
  for (uint32_t i = 0; i < XL_METER_PER_THREAD; ++i) s += xl_meter_p_cs16(x[i]);
#pragma unroll
  for (uint32_t stride = 32u; stride >= 1u; stride >>= 1) s += (uint64_t)__shfl_down((unsigned long long)s, stride, 64);
  if ((tid & 63u) == 0u) waves[tid >> 6] = s;
  __syncthreads();
  if (tid == 0u) ((XlMeterDst)(uintptr_t)partials)[w] = waves[0] + waves[1] + waves[2] + waves[3];
}

}  // namespace

int xl_meter_launch(bool cs16, const XlMeterRun *runs, uint32_t nruns, uint32_t W, uint64_t *partials, hipStream_t st) {
  if (W == 0u || nruns == 0u) return 0;
  if (cs16) hipLaunchKernelGGL(xl_meter_cs16_kernel, dim3(W), dim3(XL_METER_THREADS), 0, st, runs, nruns, partials);
  else hipLaunchKernelGGL(xl_meter_cf32_kernel, dim3(W), dim3(XL_METER_THREADS), 0, st, runs, nruns, partials);
  return (int)hipGetLastError();
}
