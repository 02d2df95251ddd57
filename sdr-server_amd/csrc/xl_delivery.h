// xl_delivery.h -- the delivery object's launch (xl_delivery.hip) as its host side (xl_delivery.cpp) calls it.
// Internal to libxlating_serve.so; the public interface is include/xlating_delivery.h, the layout xl_delivery_plan.h.
#ifndef XL_DELIVERY_INTERNAL_H_
#define XL_DELIVERY_INTERNAL_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "xl_delivery_plan.h"

// runs, stage: device.  chunks: xl_dlv_chunks of the image's size; the launch writes image bytes of rows only, all below that size.
// 0 or a hipError_t.
int xl_dlv_launch(const XlDlvRun *runs, uint32_t nruns, uint32_t chunks, void *stage, hipStream_t st);
// The same for the runs of xl_dlv_plan_narrow (xl_delivery_narrow.hip): cf32 sources, read only, their cs16 pairs into the image.
int xl_dlv_narrow_launch(const XlDlvRun *runs, uint32_t nruns, uint32_t chunks, void *stage, hipStream_t st);
// The same image from the runs of xl_dlv_plan_gain (xl_delivery_gain.hip), each run under its gain; levels: the level table on the
// device, XL_DLV_LEVEL_WORDS uint32 a run, ZEROED on st before this launch: the launch adds every run's level to its entry.
int xl_dlv_gain_launch(const XlDlvGainRun *runs, uint32_t nruns, uint32_t chunks, void *stage, uint32_t *levels, hipStream_t st);

#endif
