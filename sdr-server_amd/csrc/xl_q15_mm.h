// xl_q15_mm.h -- the matrix-core Q15 FIR launch (q15mm/xl_q15_mm.hip; engine option "q15_kernel"): what the host plan builds
// (xl_plan.cpp: xl_build_q15mm) and the launcher takes.  The arithmetic and its proofs: xl_q15_digits.h.
#ifndef XL_Q15_MM_H_
#define XL_Q15_MM_H_

#include "xl_device.h"
#include "xl_q15_digits.h"

// One tile: up to 32 clients of ONE direct class (D, T, grid, valid history) -- the rows of the matrix instruction.
struct XlQmmTile {
  uint32_t D, T, ksteps;
  uint32_t rem0, hv0;   // class record at plan time (xl_grid_dyn)
  uint32_t nc;          // outputs per wave (xl_q15mm_pick_nc): a workgroup covers 8 nc consecutive outputs
  uint32_t nclients;    // 1..32 (the other rows hold zero taps and store nothing)
  uint32_t frag_off;    // the tile's A image, in fragments of XL_QMM_FRAG bytes
  uint32_t out_off[XL_QMM_ROWS];  // per client: float2 index of its output row; / XL_PH_STRIDE into the phase table
  uint32_t qincr[XL_QMM_ROWS];    // per client: Q15 phase increment, packed like XlTile::qincr
  long long corr_r[XL_QMM_ROWS], corr_i[XL_QMM_ROWS];  // per client: xl_q15mm_correction of its two rows (cs16 input)
};

struct XlQmmArgs {
  const void *in0;  // [in0 | in1]: n0 samples of raw history, then n1 new samples (as XlFirArgs)
  const void *in1;
  uint32_t n0, n1;
  int fmt;  // XLF_CU8, XLF_CS8 or XLF_CS16
  XlPos pos;
  const XlQmmTile *tiles;
  uint32_t ntiles;
  uint32_t xtiles;  // workgroups along the outputs: max over the tiles of ceil(K / (8 nc))
  const int8_t *image;
  const short2 *qphtab;
  float2 *out;  // short2 rows at the addresses of the float2 rows
  void *hist_out;  // the call's raw-history roll rides on this launch when it is the call's first (null: no roll), as XlFirArgs
  uint32_t hist_units, block_units;
};

// window image bytes of a tile for input format fmt
static inline size_t xl_q15mm_lds_bytes(const XlQmmTile &t, int fmt) {
  const size_t plane = (size_t)((xl_q15mm_span(t.D, t.ksteps, t.nc) + 7u) & ~(uint64_t)7u) * 2u;
  return plane * (fmt == XLF_CS16 ? 2u : 1u);
}

// lds_bytes: xl_q15mm_lds_bytes maximised over the tiles
hipError_t xl_launch_q15_mm(const XlQmmArgs &a, size_t lds_bytes, hipStream_t s);

#endif  // XL_Q15_MM_H_
