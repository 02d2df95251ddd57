// xl_xop_layout.h -- index bookkeeping of the OPERAND-FORM image of the shared spectra: what xlp_forward_kernel<M, 4, true> writes and
// xlp_mix_mfma_kernel<NKB, false, true> stages into LDS (xl_polyphase.hip, xl_mixh.hip), built from xl_mix_layout.h and, like it,
// compiled for the host too: tests/c/test_xop_layout.cpp stages an image written through these functions and compares the LDS
// contents, byte for byte, with what the converting staging of xlp_mix_mfma_kernel writes for the same float32 spectra.
//
// The image holds, per (pass, bin m), the RE rows of the A operands of the bin's matrix products, scaled and split:
//
//   [pass][m][term 2][group of four branches 2 nkb][segment 16][8 halves]        16-byte slots; nkb KB per (pass, bin)
//
// A slot holds the four adjacent branches 4 g .. 4 g + 3 (g = 2 k-block + h) of one segment's re row, one dword each: the halves of
// (X.re, X.im) times XLP_H_XSCALE, first halves in term 0 and second halves in term 1.  The segment's im row (X.im, -X.re) is the same
// dword rotated by 16 bits with the sign of its high half flipped (xop_im_dword): the mix's staging writes both -- one 16-byte load,
// two 16-byte LDS writes, two vector instructions per dword -- and the image is no larger than the float32 spectra (the first form of
// this image stored both rows: twice the bytes through the L2s, and the mix launch, bound by its streams, was 8 % slower for it).
// The 16 segments of one (m, term, group) are 256 contiguous bytes: a forward workgroup -- (pass, group of four branches) -- writes
// whole 128-byte lines and never a part of another workgroup's slot.  Branches >= D of a written group are written as zeros, and
// groups that no workgroup writes (up to 2 nkb - 1) stay as the zeros the image was cleared to once.
#ifndef XL_XOP_LAYOUT_H_
#define XL_XOP_LAYOUT_H_
#include "xl_mix_layout.h"

#define XOP_GROUP 4u  // adjacent branches per 16-byte slot = per forward workgroup
#define XOP_SEG 16u   // segments of a pass (XLP_SEG)

// 16-byte slots of one (pass, bin): what a mix workgroup loads per pass
XLM_FN uint32_t xop_bin_slots(uint32_t nkb) { return 2u * 2u * nkb * XOP_SEG; }
// bytes of the image for `passes` passes
XLM_FN size_t xop_bytes(uint32_t passes, uint32_t M, uint32_t nkb) { return (size_t)passes * M * xop_bin_slots(nkb) * 16u; }
// first slot of (pass, bin m)
XLM_FN size_t xop_bin_base(uint32_t M, uint32_t nkb, uint32_t pass, uint32_t m) { return ((size_t)pass * M + m) * xop_bin_slots(nkb); }
// slot within the bin's part of (term, group g of four branches, segment sl of the pass)
XLM_FN uint32_t xop_in_bin(uint32_t nkb, uint32_t term, uint32_t g, uint32_t sl) { return (term * 2u * nkb + g) * XOP_SEG + sl; }
// the mix launch's view of slot i < xop_bin_slots(nkb) of the bin's part: where its re row and its im row go in the A operands
// xs[term][k-block][LDS slot] taken as ONE array of 16-byte slots
XLM_FN uint32_t xop_lds_index(uint32_t i, uint32_t comp) {
  const uint32_t sl = i % XOP_SEG, g = i / XOP_SEG;  // (g counts on through the terms: term * 2 nkb + group)
  return (g >> 1) * 64u + xlm_lds_slot(xlm_lane(g & 1u, xlm_row(sl, comp)));
}
// the dword of one branch in its re row, from the 16-bit patterns of the halves of (X.re, X.im) of one term: low half-word = the
// factor of R.re, high half-word = the factor of -R.im ...
XLM_FN uint32_t xop_re_dword(uint32_t re16, uint32_t im16) { return re16 | (im16 << 16); }
// ... and the same branch in the im row, (X.im, -X.re): the sign bit, as a negation does
XLM_FN uint32_t xop_im_dword(uint32_t re_dword) { return ((re_dword >> 16) | (re_dword << 16)) ^ 0x80000000u; }

#endif  // XL_XOP_LAYOUT_H_
