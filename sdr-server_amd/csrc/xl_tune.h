// xl_tune.h -- the tuner bank's launch (xl_tune.hip) as its host side (xl_tune.cpp) calls it.
// Internal to libxlating_tune.so; the public interface is include/xlating_tune.h, the rule xl_tune_rule.h.
#ifndef XL_TUNE_INTERNAL_H_
#define XL_TUNE_INTERNAL_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

#define XL_TUNE_THREADS 256u
#define XL_TUNE_PER_THREAD 8u  // samples per thread, XL_TUNE_THREADS apart
#define XL_TUNE_CHUNK (XL_TUNE_THREADS * XL_TUNE_PER_THREAD)  // samples of a row per workgroup

// One stream of a feed: out[j] = the rotation of src[j] by phi_j of (P, F, R), j < cnt.  cnt >= 1 (a stream that consumes nothing has
// no run).  The launch's workgroup w belongs to the run with wsum <= w < next wsum and rotates samples
// [(w - wsum) XL_TUNE_CHUNK, min(cnt, (w - wsum + 1) XL_TUNE_CHUNK)).
struct XlTuneRun {
  const float2 *src;
  float2 *out;
  uint64_t P;
  int64_t F, R;
  uint32_t cnt;
  uint32_t wsum;
};

// runs: device.  W: workgroups of the launch (the last run's wsum + its own).  0 or a hipError_t.
int xl_tune_launch(const XlTuneRun *runs, uint32_t nruns, uint32_t W, hipStream_t st);

#endif
