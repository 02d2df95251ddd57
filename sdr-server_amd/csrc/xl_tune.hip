// xl_tune.hip -- the tuner bank's kernel (include/xlating_tune.h): the rotation of MANY streams, each by its own phase, step and ramp,
// in one ragged launch.
//
// The host writes one run per stream (XlTuneRun) with the running sum of workgroups; a workgroup finds its run by binary search
// (xl_ragged.h) and rotates XL_TUNE_CHUNK consecutive samples of that ONE stream.  A thread takes XL_TUNE_PER_THREAD samples,
// XL_TUNE_THREADS apart (a wave reads and writes 512 contiguous bytes at a time): its first phase by the closed form, the others by
// two 64-bit additions each (xl_tune_rule.h's xl_tune_stride) -- integer arithmetic, so the bits are the closed form's.  All loads of
// a thread are in flight before the first sine.  Sine, cosine and the product are xl_tune_rule.h's text.
// Memory-bound: 8 bytes read and 8 written per sample, as the delivery's pack launch.
// SCALAR FP32 ONLY, nothing fused (-ffp-contract=off), no matrix instructions, no LDS, no scratch (Makefile: TUNE_FLAGS;
// tests/test_tune_cpu.py reads the code object): the launch runs behind and beside the engine's matrix-core launches.
#include "xl_tune.h"

#include "xl_ragged.h"
#include "xl_tune_rule.h"

namespace {

// (global address space stated: an address that comes out of a table would otherwise be loaded through the flat path)
typedef float XlTuneF2 __attribute__((ext_vector_type(2)));
typedef const XlTuneF2 __attribute__((address_space(1))) *XlTuneSrc;
typedef XlTuneF2 __attribute__((address_space(1))) *XlTuneDst;

__global__ void __launch_bounds__(XL_TUNE_THREADS) xl_tune_kernel(const XlTuneRun *__restrict__ runs, const uint32_t nruns) {
  const uint32_t w = blockIdx.x, tid = threadIdx.x;
  const uint32_t k = xl_ragged_find(runs, nruns, w, [](const XlTuneRun &r) { return r.wsum; });
  const XlTuneRun r = runs[k];  // (uniform)
  const uint32_t j0 = (w - r.wsum) * XL_TUNE_CHUNK + tid;
  const XlTuneSrc src = (XlTuneSrc)(uintptr_t)r.src;
  const XlTuneDst out = (XlTuneDst)(uintptr_t)r.out;
  XlTuneF2 x[XL_TUNE_PER_THREAD];
#pragma unroll
  for (uint32_t i = 0; i < XL_TUNE_PER_THREAD; ++i) {
    const uint32_t j = j0 + i * XL_TUNE_THREADS;
    x[i] = j < r.cnt ? src[j] : XlTuneF2{0.0f, 0.0f};
  }
  uint64_t phi = xl_tune_phase(r.P, r.F, r.R, j0);
  uint64_t d = xl_tune_stride(r.F, r.R, j0, XL_TUNE_THREADS);
  const uint64_t dd = (uint64_t)XL_TUNE_THREADS * XL_TUNE_THREADS * (uint64_t)r.R;
#pragma unroll
  for (uint32_t i = 0; i < XL_TUNE_PER_THREAD; ++i) {
    const uint32_t j = j0 + i * XL_TUNE_THREADS;
    float re, im;
    xl_tune_rotate(x[i].x, x[i].y, phi, &re, &im);
    if (j < r.cnt) out[j] = XlTuneF2{re, im};
    phi += d, d += dd;
  }
}

}  // namespace

int xl_tune_launch(const XlTuneRun *runs, uint32_t nruns, uint32_t W, hipStream_t st) {
  if (W == 0u || nruns == 0u) return 0;
  hipLaunchKernelGGL(xl_tune_kernel, dim3(W), dim3(XL_TUNE_THREADS), 0, st, runs, nruns);
  return (int)hipGetLastError();
}
