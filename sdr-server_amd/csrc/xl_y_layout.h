// xl_y_layout.h -- where an element of the mixed-spectra image Y lies: what the four mix kernels write (xl_mixh.hip, xl_mixh2.hip,
// xl_mixf32.hip) and the three inverse kernels read (xl_polyphase.hip, xl_inv8.hip, xl_inv32.hip), and what the engine allocates
// (xl_batch.cpp).  Compiled for the host too: tests/c/test_y_layout.cpp holds the writers' address against the readers'.
//
// Y[c][s][m] = the sum over the branches for client column c, segment s, spectrum bin m: one complex float32 element of 8 bytes, in
//
//   [column group cg][segment s < nseg_cap][sub][bin m < M][CW columns]        sub < XLY_COLS / CW, CW = xly_tile_columns(M)
//
// A column group is XLY_COLS = 128 adjacent client columns; column `col` of it is column col % CW of the group's tile col / CW.  One
// TILE -- (cg, s, sub): all M bins of CW columns, M x CW x 8 bytes = 32 KB -- is contiguous: it is one inverse workgroup's input,
// read as whole lines, and a mix wave's store instruction writes 256-byte runs of it.  nseg_cap is the plan's segment capacity, not
// the call's segment count: a column group's part of the image does not move with the call's length.
#ifndef XL_Y_LAYOUT_H_
#define XL_Y_LAYOUT_H_
#include "xl_mix_layout.h"

#define XLY_COLS 128u  // client columns per column group (XLP_COLS)

// columns of one tile: 16 (M = 256), 32 (M = 128), 64 (M = 64)  (constexpr: the inverse kernels size their LDS by it)
XLM_FN constexpr uint32_t xly_tile_columns(uint32_t M) { return M == 256u ? 16u : (M == 64u ? 64u : 32u); }
// elements from a segment of a column group to the next one (its XLY_COLS / CW tiles)
XLM_FN size_t xly_seg_stride(uint32_t M) { return (size_t)(XLY_COLS / xly_tile_columns(M)) * M * xly_tile_columns(M); }
// first element of tile (cg, s, sub): the inverse kernels' view; element (bin m, column cc of the tile) is m * CW + cc behind it
XLM_FN size_t xly_tile(uint32_t nseg_cap, uint32_t M, uint32_t cg, uint32_t s, uint32_t sub) {
  const uint32_t CW = xly_tile_columns(M), NSUB = XLY_COLS / CW;
  return ((((size_t)cg * nseg_cap + s) * NSUB + sub) * M) * CW;
}
// element (segment s, column col < XLY_COLS of the group, bin m): the mix kernels' view (they take s = 0 and step by xly_seg_stride),
// as the bin's row of the column's tile plus the column's place in it (two terms: the kernels add them to the image pointer one
// after the other, which compiles to the code these launches were measured with; summed in an integer first it does not)
XLM_FN size_t xly_row(uint32_t nseg_cap, uint32_t M, uint32_t cg, uint32_t s, uint32_t col, uint32_t m) {
  const uint32_t CW = xly_tile_columns(M), NSUB = XLY_COLS / CW;
  return ((((size_t)cg * nseg_cap + s) * NSUB + col / CW) * M + m) * CW;
}
XLM_FN uint32_t xly_col_in_tile(uint32_t M, uint32_t col) { return col % xly_tile_columns(M); }
XLM_FN size_t xly_elem(uint32_t nseg_cap, uint32_t M, uint32_t cg, uint32_t s, uint32_t col, uint32_t m) {
  return xly_row(nseg_cap, M, cg, s, col, m) + xly_col_in_tile(M, col);
}
// bytes of the image for ncg_cap column groups
XLM_FN size_t xly_bytes(uint32_t ncg_cap, uint32_t nseg_cap, uint32_t M) { return (size_t)ncg_cap * nseg_cap * xly_seg_stride(M) * 8u; }

#endif  // XL_Y_LAYOUT_H_
