// xl_q15_mm.hip -- the Q15 family's FIR on the matrix cores (engine option "q15_kernel" = 1): xlating.c:92-140 for every client the
// host proved eligible (xl_q15_digits.h), bit for bit, from int8 digit products summed by v_mfma_i32_32x32x32_i8.
//
//   rows (A operand)      the 32 clients of a tile; per client a real-part row [cr, -ci] and an imaginary-part row [ci, cr], each in a
//                         high and a low digit: four fragments per k-step, read from the tile's image in global memory (L2)
//   columns (B operand)   32 outputs of a wave; a lane's fragment is 8 consecutive samples [xr, xi] of the window image in LDS
//   K                     the interleaved tap index, 16 complex taps per instruction
// A workgroup of 8 waves covers 8 nc consecutive outputs of one tile (nc = 32 unless the window image would not fit) and stages their
// common window once, as one (cu8, cs8) or two (cs16) planes of int8 digit pairs.  Wave w takes the outputs i = r mod P, r = w mod P,
// P = 8 / gcd(D, 8): their window starts i D share one residue mod 8, the tile's image holds the taps delayed by that residue, and every
// window read is a 16-byte-aligned LDS read.
//
// This file issues matrix instructions: it is compiled without the SLP vectoriser (Makefile: Q15MM_FLAGS), its source holds integer
// arithmetic only (the one scalar v_mul_f32 of its code object is the compiler's reciprocal for xl_grid_dyn's divisions by D), and it lives in a directory of its own (tests/test_q15_matrix_cpu.py checks the code object).
#include "../xl_dev_inline.h"
#include "../xl_q15_mm.h"

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));

// one raw sample -> its digit pairs (low byte = real part).  PL = 1: d0 is the single digit of cu8 (v - 128) / cs8 (v); PL = 2: d0 the
// high, d1 the low digits of cs16.  A sample that does not exist is the VALUE 0: (0, 0) in the 8-bit formats, hi = 0, lo = -128 in cs16.
template <int PL>
XL_DEV void xl_qmm_digits(const void *__restrict__ in0, const void *__restrict__ in1, uint32_t n0, uint32_t n1, int fmt, uint32_t sidx,
                          uint32_t zero_below, uint16_t *d0, uint16_t *d1) {
  const bool first = sidx < n0;
  const bool ok = sidx >= zero_below && (first || sidx - n0 < n1);
  const void *__restrict__ p = first ? in0 : in1;
  const uint32_t i = first ? sidx : sidx - n0;
  if (PL == 1) {
    uint32_t v = 0u;
    if (ok) v = reinterpret_cast<const uint16_t *>(p)[i] ^ (fmt == XLF_CU8 ? 0x8080u : 0u);
    *d0 = (uint16_t)v;
    *d1 = 0;
  } else {
    uint32_t v = 0u;
    if (ok) v = reinterpret_cast<const uint32_t *>(p)[i];
    *d0 = (uint16_t)(((v >> 8) & 0xFFu) | ((v >> 24) << 8));
    *d1 = (uint16_t)(((v & 0xFFu) | (((v >> 16) & 0xFFu) << 8)) ^ 0x8080u);
  }
}

template <int PL>
__global__ __launch_bounds__(64 * XL_QMM_WAVES) void xl_q15_mm_kernel(const XlQmmArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint16_t xl_qmm_win[];
  // raw-history roll, as in xl_fir_kernel: the call's first launch carries it
  {
    const uint32_t b = blockIdx.y * gridDim.x + blockIdx.x, nb = gridDim.x * gridDim.y;
    const uint32_t roll_blocks = nb < XL_ROLL_BLOCKS ? nb : XL_ROLL_BLOCKS;
    if (a.hist_out != nullptr && b < roll_blocks) {
      const uint16_t *__restrict__ h0 = reinterpret_cast<const uint16_t *>(a.in0);
      const uint16_t *__restrict__ h1 = reinterpret_cast<const uint16_t *>(a.in1);
      uint16_t *__restrict__ ho = reinterpret_cast<uint16_t *>(a.hist_out);
      for (uint32_t j = b * blockDim.x + threadIdx.x; j < a.hist_units; j += roll_blocks * blockDim.x) {
        const uint32_t sidx = a.block_units + j;
        ho[j] = (sidx < a.hist_units) ? h0[sidx] : h1[sidx - a.hist_units];
      }
    }
  }
  const XlQmmTile *__restrict__ t = a.tiles + blockIdx.y;
  const uint32_t D = t->D, T = t->T, ksteps = t->ksteps, nc = t->nc, ncl = t->nclients;
  const XlDyn d = xl_grid_dyn(D, T, t->rem0, t->hv0, a.pos);
  const uint32_t K = d.K;
  const uint32_t m0 = blockIdx.x * XL_QMM_WAVES * nc;
  if (m0 >= K) return;
  const uint32_t span = (XL_QMM_WAVES * nc - 1u) * D + XL_QMM_KTAPS * ksteps;
  const uint32_t plane = (span + 7u) & ~7u;  // in samples (uint16 digit pairs): plane 1 starts 16-byte aligned
  {
    const uint32_t origin = d.base + m0 * D;
    for (uint32_t j = threadIdx.x; j < span; j += blockDim.x) {
      uint16_t d0, d1;
      xl_qmm_digits<PL>(a.in0, a.in1, a.n0, a.n1, a.fmt, origin + j, d.zero_below, &d0, &d1);
      xl_qmm_win[j] = d0;
      if (PL == 2) xl_qmm_win[plane + j] = d1;
    }
  }
  __syncthreads();
  const uint32_t w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63u;
  const uint32_t P = xl_q15mm_residues(D);
  const uint32_t r = w & (P - 1u), q = w >> __builtin_ctz(P);  // (P is 1, 2, 4 or 8)
  if (m0 + q * nc * P + r >= K) return;  // (the wave's first output: the others lie behind it)
  const uint32_t col = lane & 31u, h = lane >> 5;
  const uint32_t i = (q * nc + (col < nc ? col : 0u)) * P + r;  // this lane's output of the workgroup (idle columns read column 0's window)
  const uint32_t start = i * D - xl_q15mm_shift(D, r);           // a multiple of 8 samples
  const v4i *__restrict__ b0 = reinterpret_cast<const v4i *>(xl_qmm_win + start + 8u * h);
  const v4i *__restrict__ b1 = reinterpret_cast<const v4i *>(xl_qmm_win + plane + start + 8u * h);
  // the tile's image: [residue][real hi, real lo, imag hi, imag lo][kstep][lane]
  const v4i *__restrict__ A = reinterpret_cast<const v4i *>(a.image) + ((size_t)t->frag_off + (size_t)r * 4u * ksteps) * 64u + lane;
  const size_t ap = (size_t)ksteps * 64u;
  v16i rh = {}, rl = {}, ih = {}, il = {};  // PL = 1: S(hi, d), S(lo, d).  PL = 2: rh = S(hi,hi), rl = S(lo,lo), and the middle sums:
  v16i rm = {}, im = {};                    // S(hi,lo) + S(lo,hi)
  for (uint32_t kk = 0; kk < ksteps; ++kk) {
    const v4i arh = A[(size_t)kk * 64u], arl = A[ap + (size_t)kk * 64u], aih = A[2u * ap + (size_t)kk * 64u],
              ail = A[3u * ap + (size_t)kk * 64u];
    const v4i x0 = b0[2u * kk];
    rh = __builtin_amdgcn_mfma_i32_32x32x32_i8(arh, x0, rh, 0, 0, 0);
    ih = __builtin_amdgcn_mfma_i32_32x32x32_i8(aih, x0, ih, 0, 0, 0);
    if (PL == 1) {
      rl = __builtin_amdgcn_mfma_i32_32x32x32_i8(arl, x0, rl, 0, 0, 0);
      il = __builtin_amdgcn_mfma_i32_32x32x32_i8(ail, x0, il, 0, 0, 0);
    } else {
      const v4i x1 = b1[2u * kk];
      rm = __builtin_amdgcn_mfma_i32_32x32x32_i8(arl, x0, rm, 0, 0, 0);
      im = __builtin_amdgcn_mfma_i32_32x32x32_i8(ail, x0, im, 0, 0, 0);
      rm = __builtin_amdgcn_mfma_i32_32x32x32_i8(arh, x1, rm, 0, 0, 0);
      im = __builtin_amdgcn_mfma_i32_32x32x32_i8(aih, x1, im, 0, 0, 0);
      rl = __builtin_amdgcn_mfma_i32_32x32x32_i8(arl, x1, rl, 0, 0, 0);
      il = __builtin_amdgcn_mfma_i32_32x32x32_i8(ail, x1, il, 0, 0, 0);
    }
  }
  const uint32_t m = m0 + i;
  if (col >= nc || m >= K) return;
  // C/D map of the 32x32 forms: the lane holds column `col`, register g holds row (g & 3) + 8 (g >> 2) + 4 h
#pragma unroll
  for (int g = 0; g < 16; ++g) {
    const uint32_t row = (uint32_t)(g & 3) + 8u * (uint32_t)(g >> 2) + 4u * h;
    if (row >= ncl) continue;
    long long sr, si;
    if (PL == 1) {
      sr = xl_q15mm_combine8(rh[g], rl[g]);
      si = xl_q15mm_combine8(ih[g], il[g]);
    } else {
      sr = xl_q15mm_combine16(rh[g], rm[g], rl[g], t->corr_r[row]);
      si = xl_q15mm_combine16(ih[g], im[g], il[g], t->corr_i[row]);
    }
    // >> 15 of the int64 sums, cut to 32 bits, saturated (xlating.c:118-119; xl_q15_narrow.h)
    xl_q15_rotate_store(a.qphtab, a.out, t->out_off[row], t->qincr[row], m, xl_q15_narrow_sum64(sr), xl_q15_narrow_sum64(si));
  }
}

template <int PL>
static hipError_t xl_q15_mm_go(const XlQmmArgs &a, size_t lds, hipStream_t s) {
  static bool attr_done = false;
  if (!attr_done) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&xl_q15_mm_kernel<PL>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       160 * 1024);
    if (e != hipSuccess) return e;
    attr_done = true;
  }
  hipLaunchKernelGGL((xl_q15_mm_kernel<PL>), dim3(a.xtiles, a.ntiles), dim3(64 * XL_QMM_WAVES), lds, s, a);
  return hipGetLastError();
}

hipError_t xl_launch_q15_mm(const XlQmmArgs &a, size_t lds_bytes, hipStream_t s) {
  if (a.ntiles == 0 || a.xtiles == 0) return hipSuccess;
  if (lds_bytes > 160 * 1024 || a.ntiles > 65535u || (a.fmt != XLF_CU8 && a.fmt != XLF_CS8 && a.fmt != XLF_CS16)) return hipErrorInvalidValue;
  return a.fmt == XLF_CS16 ? xl_q15_mm_go<2>(a, lds_bytes, s) : xl_q15_mm_go<1>(a, lds_bytes, s);
}
