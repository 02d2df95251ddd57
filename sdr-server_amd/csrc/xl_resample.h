// xl_resample.h -- the resampler bank's launches (xl_resample.hip) as its host side (xl_resample.cpp) calls them.
// Internal to libxlating_resample.so; the public interface is include/xlating_resample.h.
#ifndef XL_RESAMPLE_INTERNAL_H_
#define XL_RESAMPLE_INTERNAL_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

#define XL_RS_TILE 256u      // outputs per workgroup = threads per workgroup
#define XL_RS_LDS_SPAN 4096u // input samples a workgroup stages in LDS (32 KiB); a wider window is read in place
#define XL_RS_CARRY_SLOT 1024u  // samples of carry per stream id (>= XLATING_RESAMPLE_MAX_Q - 1)

// One stream of a feed.  Its `nout` new outputs go to out[0 ..]; output k sits at t = p0 + k * M on the upsampled grid counted from
// the phase-0 position of input n0: it reads inputs n0 + t / L - q, q < Q, RELATIVE to src[0]; a negative index i is
// carry[(Q - 1) + i] (the stream's last Q - 1 inputs before this feed, i >= -(Q - 1) always).  table: [L][Q], phase-major.
// The launch's workgroup w belongs to the run with wsum <= w < next wsum (a run of no outputs has no workgroups).
// The carry launch then makes carry = concat(carry, src[0 .. cnt))[-(Q - 1):].
struct XlRsRun {
  const float2 *src;
  float2 *carry;
  const float *table;
  float2 *out;
  int32_t n0;
  uint32_t p0;
  uint32_t Q, L, M;
  uint32_t nout;
  uint32_t wsum;
  uint32_t cnt;
};

// runs: device.  W: workgroups of the launch (the last run's wsum + its own).  0 or a hipError_t.
int xl_rs_launch(const XlRsRun *runs, uint32_t nruns, uint32_t W, hipStream_t st);
int xl_rs_carry(const XlRsRun *runs, uint32_t nruns, hipStream_t st);

#endif
