// xl_meter.h -- the power meter's launch (xl_meter.hip) as its host side (xl_meter.cpp) calls it.
// Internal to libxlating_meter.so; the public interface is include/xlating_meter.h, the rule xl_meter_rule.h.
#ifndef XL_METER_INTERNAL_H_
#define XL_METER_INTERNAL_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

// One row of a measurement: cnt >= 1 samples at src (a row of no samples has no run).  The launch's workgroup w belongs to the run with
// wsum <= w < next wsum, measures samples [(w - wsum) XL_METER_PIECE, min(cnt, (w - wsum + 1) XL_METER_PIECE)) and writes partials[w].
struct XlMeterRun {
  const void *src;
  uint32_t cnt;
  uint32_t wsum;
};

// runs, partials (W entries): device.  W: workgroups of the launch (the last run's wsum + its own).  cs16: int16 pairs, otherwise
// float32 pairs.  0 or a hipError_t.
int xl_meter_launch(bool cs16, const XlMeterRun *runs, uint32_t nruns, uint32_t W, uint64_t *partials, hipStream_t st);

#endif
