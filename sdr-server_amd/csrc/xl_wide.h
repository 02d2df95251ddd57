/* xl_wide.h -- the routing rule of the wide direct FIR (xl_wide.hip), as plain C so that the CPU suite can pin it
 * (tests/test_wide_rules.py).  No HIP types.
 *
 * xl_fir_kernel stages one window image per tile in the 160 KiB LDS: (ota - 1) * D + Tpad samples of 8 bytes for ota = 64,
 * 32, 16 or 8 outputs per wave (xl_fir_pick_ota).  A client whose image does not fit even at 8 outputs per wave,
 *     (7 * D + Tpad) * 8 > 160 * 1024,
 * takes the wide kernel instead, which reads its windows straight from global memory.  Tpad = T rounded up to
 * `tap_multiple`: the drop-in pads to 4 taps (XL_TAP_UNROLL), the batch engine checks at 12 (the largest tap step of
 * its tile heights).  This is exactly where xl_fir_pick_ota(D, Tpad, 160 KiB) returns 0. */
#ifndef XL_WIDE_H_
#define XL_WIDE_H_
#include <stdint.h>

#define XL_WIDE_LDS_BUDGET (160u * 1024u)

static inline int xl_fir_needs_wide(uint32_t D, uint32_t T, uint32_t tap_multiple) {
  const uint64_t tpad = ((uint64_t)T + tap_multiple - 1u) / tap_multiple * tap_multiple;
  return ((uint64_t)7u * D + tpad) * 8u > (uint64_t)XL_WIDE_LDS_BUDGET;
}

#endif /* XL_WIDE_H_ */
