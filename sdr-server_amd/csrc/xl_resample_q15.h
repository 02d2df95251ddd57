// xl_resample_q15.h -- the Q15 resampler bank's launches (xl_resample_q15.hip) as the banks' host side (xl_resample.cpp) calls them.
// Internal to libxlating_resample.so; the public interface is include/xlating_resample_q15.h.
#ifndef XL_RESAMPLE_Q15_INTERNAL_H_
#define XL_RESAMPLE_Q15_INTERNAL_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "xl_resample.h"  // XL_RS_TILE, XL_RS_CARRY_SLOT: the tiling and the carry slots are the float bank's

#define XL_RSQ_LDS_SPAN 4096u  // input samples (one 32-bit word each) a workgroup stages in LDS (16 KiB); a wider window is read in place
#define XL_RSQ_LDS_TAPS 4096u  // a tap table of up to L * Q = this many int16 is staged in LDS as well (8 KiB)
#define XL_RSQ_WIDE 1u         // XlRsQ15Run::flags: some phase has sum |c| > 65535, the sums take 64 bits
#define XL_RSQ_TAPS_IN_PLACE 2u  // XlRsQ15Run::flags: the tap table is read in place whatever its size (measurements only)

// An int16 (re, im) pair: re in the low half of one 32-bit word, im in the high half (the engine's cs16 rows, little-endian).
typedef uint32_t xl_cs16;

// One stream of a feed: XlRsRun's fields with 4-byte samples and an int16 table ([L][Q], phase-major, padded to a whole number of
// 32-bit words), and the accumulator the host has proven sufficient.
struct XlRsQ15Run {
  const xl_cs16 *src;
  xl_cs16 *carry;
  const int16_t *table;
  xl_cs16 *out;
  int32_t n0;
  uint32_t p0;
  uint32_t Q, L, M;
  uint32_t nout;
  uint32_t wsum;
  uint32_t cnt;
  uint32_t flags;
  uint32_t pad_;
};

// runs: device.  W: workgroups of the launch (the last run's wsum + its own).  0 or a hipError_t.
int xl_rsq_launch(const XlRsQ15Run *runs, uint32_t nruns, uint32_t W, hipStream_t st);
int xl_rsq_carry(const XlRsQ15Run *runs, uint32_t nruns, hipStream_t st);

#endif
