// xl_resample_dev.h -- what the kernels of the two resampler banks share (xl_resample.hip: XlRsRun, float2 samples;
// xl_resample_q15.hip: XlRsQ15Run, xl_cs16 samples): where a workgroup's tile of outputs lies, and the carry launch's body.  Templated
// on the run type; only the fields the two runs have in common are used.  The FIR sums are the files' own.
#ifndef XL_RESAMPLE_DEV_H_
#define XL_RESAMPLE_DEV_H_

#include "xl_ragged.h"
#include "xl_resample.h"

// A workgroup's tile of XL_RS_TILE consecutive outputs of one run, and this thread's output in it.
struct XlRsTile {
  uint32_t k0, nv;  // the tile's first output (< nout < 2^31) and its outputs: thread tid < nv computes output k0 + tid
  uint32_t K;       // Q - 1
  int32_t nt;       // the tile's first output reads input nt (relative to src, 0 <= nt < cnt) ..
  uint32_t dn, p;   // .. this thread's reads input nt + dn at phase p (dn wraps harmlessly in a thread past the tile's outputs)
  uint64_t span;    // the window: inputs nt - K .. nt + dn of the tile's last output
};

// The run of workgroup blockIdx.x and its tile.  false: the tile has no outputs (never: the host counts the workgroups from nout).
// Output k of a run sits at t = p0 + k * M on the grid of the input upsampled by L; with M = Mq * L + Mr a thread's position inside
// the tile needs 32-bit arithmetic only (tid * Mr < 2^20), the tile's own position one 64-bit division.
template <typename Run>
__device__ __forceinline__ bool xl_rs_tile(const Run *__restrict__ runs, const uint32_t nruns, Run &r, XlRsTile &t) {
  const uint32_t w = blockIdx.x, tid = threadIdx.x;
  r = runs[xl_ragged_find(runs, nruns, w, [](const Run &x) { return x.wsum; })];
  t.k0 = (w - r.wsum) * XL_RS_TILE;
  if (t.k0 >= r.nout) return false;
  t.nv = min(XL_RS_TILE, r.nout - t.k0);
  t.K = r.Q - 1u;
  const uint64_t t0 = (uint64_t)r.p0 + (uint64_t)t.k0 * r.M;
  t.nt = r.n0 + (int32_t)(t0 / r.L);
  const uint32_t pt = (uint32_t)(t0 % r.L);  // the phase of the tile's first output
  const uint32_t Mq = r.M / r.L, Mr = r.M % r.L;
  const uint32_t u = pt + tid * Mr, ul = pt + (t.nv - 1u) * Mr;
  t.dn = tid * Mq + u / r.L;
  t.p = u % r.L;
  t.span = (uint64_t)(t.nv - 1u) * Mq + ul / r.L + r.Q;
  return true;
}

// The carry launch, one workgroup of 256 threads per run: carry = concat(carry, src[0 .. cnt))[-(Q - 1):].  A feed shorter than the
// carry shifts it, and the move overlaps itself: every thread reads its (up to four) samples, the workgroup meets, then they are
// written.
template <typename Run, typename Sample>
__device__ __forceinline__ void xl_rs_carry_body(const Run *__restrict__ runs) {
  const Run r = runs[blockIdx.x];
  const uint32_t K = r.Q - 1u;
  if (K == 0u || r.cnt == 0u) return;
  Sample v[XL_RS_CARRY_SLOT / 256u];
#pragma unroll
  for (uint32_t j = 0u; j < XL_RS_CARRY_SLOT / 256u; ++j) {
    const uint32_t i = threadIdx.x + j * 256u;
    if (i < K) {
      const uint64_t s = (uint64_t)i + r.cnt;  // position in concat(carry, src)
      v[j] = s < K ? r.carry[s] : r.src[s - K];
    }
  }
  __syncthreads();
#pragma unroll
  for (uint32_t j = 0u; j < XL_RS_CARRY_SLOT / 256u; ++j) {
    const uint32_t i = threadIdx.x + j * 256u;
    if (i < K) r.carry[i] = v[j];
  }
}

#endif
