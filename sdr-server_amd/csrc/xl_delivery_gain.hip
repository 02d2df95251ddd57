// xl_delivery_gain.hip -- the narrowing pack kernel WITH A GAIN AND A METER (xlating_delivery_pack_device_cs16_gain): ONE launch turns
// every cf32 row of a batch into its cs16 row of the dense image, each row under its own power-of-two gain, and reports every row's
// level -- peak_bits, clipped, nans -- in a table behind the image that the batch's one device-to-host copy takes along.  It has the
// shape of xl_dlv_narrow_kernel (xl_delivery_narrow.hip): the layout is xl_delivery_plan.h's and the arithmetic xl_dlv_gain.h's, and
// nothing here decides any of either.  A workgroup takes chunk blockIdx.x of the image, finds its first run (xl_ragged_find +
// xl_dlv_gain_first) and moves xl_dlv_span of every run up to the chunk's end.  A whole 16-byte slot of the image inside a row is two
// aligned 16-byte loads, eight conversions, one aligned 16-byte store; a slot a row covers in part moves sample by sample.  All of a
// thread's loads of a run are issued before its first store.  The gain is the RUN's: short rows that share a slot are converted each
// under their own, in their own pass of the loop.
// The level: every thread keeps the maximum and the two counts of the floats it converted for the run (floats outside the row are read
// as zeros, which offer the peak 0 and count nowhere); the lanes of a wave combine them by DPP rotations inside the rows of 16 lanes and
// four lane reads -- no LDS, so the four waves of a workgroup do not meet -- and one lane a wave adds what is not zero to the run's
// entry of the level table with device-scope atomics (an unsigned max, two adds; no value is returned).  Integer maxima and sums: the
// table does not depend on which wave or workgroup comes first.  The host zeroes the table before the launch.
// Integer instructions only: no floating-point instruction, scalar or packed (the kernel may run beside the engine's matrix-core
// launches; tests/test_delivery_gain_cpu.py reads the code object).  The sources are only read.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "xl_delivery.h"
#include "xl_dlv_gain.h"
#include "xl_ragged.h"

namespace {

// (global address space stated: an address that comes out of a table would otherwise be loaded through the flat path)
typedef uint32_t XlDlv16 __attribute__((ext_vector_type(4)));
typedef uint32_t XlDlv8 __attribute__((ext_vector_type(2)));
typedef const XlDlv16 __attribute__((address_space(1))) *XlDlvSrc16;
typedef const XlDlv8 __attribute__((address_space(1))) *XlDlvSrc8;
typedef uint32_t __attribute__((address_space(1))) *XlDlvLevels;

struct XlDlvSpan32 {  // the 32 source bytes of one image slot: four samples
  XlDlv16 lo, hi;
};

struct XlDlvMeter {  // of one thread and one run
  uint32_t peak;     // the largest magnitude's bits
  uint32_t counts;   // clipped in the low half, nans in the high half: a thread converts 32 floats a run, a wave 2048
};

static_assert(XL_DLV_SLOTS_PER_THREAD == 4u, "the kernel body names four slots per thread");
static_assert(XL_DLV_SLOTS_PER_THREAD * 8u * 64u < 65536u, "a wave's counts fit the halves of one dword");

// one cf32 sample (re, im) under gain g -> the dword of its cs16 pair, re in the low half; the meter takes both floats
__device__ static inline uint32_t xl_dlv_gain_pair(const uint32_t re, const uint32_t im, const int32_t g, XlDlvMeter &m) {
  uint32_t cr, ci;
  const uint32_t lo = (uint32_t)xl_dlv_gain_narrow(re, g, &cr) & 0xFFFFu, hi = (uint32_t)xl_dlv_gain_narrow(im, g, &ci) << 16;
  const uint32_t a = xl_dlv_gain_mag(re), b = xl_dlv_gain_mag(im), ab = a > b ? a : b;
  m.peak = m.peak > ab ? m.peak : ab;
  m.counts += cr + ci + ((xl_dlv_gain_nan(re) + xl_dlv_gain_nan(im)) << 16);
  return lo | hi;
}

// v of the lane kRor places to the right in its row of 16 lanes (a DPP row rotation: a vector move, no LDS)
template <int kRor>
__device__ static inline uint32_t xl_dlv_ror(const uint32_t v) {
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x120 + kRor, 0xF, 0xF, false);
}

// over the 64 lanes of the wave, which are all active (the walk over the runs is uniform): the same value in every lane
template <typename Op>
__device__ static inline uint32_t xl_dlv_wave(uint32_t v, const Op op) {
  v = op(v, xl_dlv_ror<1>(v)), v = op(v, xl_dlv_ror<2>(v)), v = op(v, xl_dlv_ror<4>(v)), v = op(v, xl_dlv_ror<8>(v));  // each row's
  const uint32_t r0 = (uint32_t)__builtin_amdgcn_readlane((int)v, 0), r1 = (uint32_t)__builtin_amdgcn_readlane((int)v, 16);
  const uint32_t r2 = (uint32_t)__builtin_amdgcn_readlane((int)v, 32), r3 = (uint32_t)__builtin_amdgcn_readlane((int)v, 48);
  return op(op(r0, r1), op(r2, r3));
}

__global__ void __launch_bounds__(XL_DLV_THREADS) xl_dlv_gain_kernel(const XlDlvGainRun *__restrict__ runs, const uint32_t nruns,
                                                                      char *__restrict__ stage, uint32_t *__restrict__ levels) {
  const uint32_t c = blockIdx.x, tid = threadIdx.x;
  const uint64_t hi = ((uint64_t)c + 1u) * XL_DLV_CHUNK;
  const uint32_t found = xl_ragged_find(runs, nruns, c * (XL_DLV_CHUNK / 16u), [](const XlDlvGainRun &g) { return g.r.s16; });
  for (uint32_t k = xl_dlv_gain_first(runs, found, c); k < nruns; ++k) {
    const XlDlvGainRun gr = runs[k];  // (uniform)
    const XlDlvRun r = gr.r;
    if (r.off >= hi) break;
    uint64_t a, b;
    if (!xl_dlv_span(&r, c, &a, &b)) continue;
    // the slots [sa, sb) of the image that hold [a, b): inside the chunk, so at most four per thread; slot j of this thread is at p(j)
    const uint64_t sa = a & ~(uint64_t)15, sb = (b + 15u) & ~(uint64_t)15;
    const auto p = [&](uint32_t j) { return sa + 16u * (tid + XL_DLV_THREADS * j); };
    const auto whole = [&](uint32_t j) { return p(j) >= a && p(j) + 16u <= b; };
    const auto in_row = [&](uint64_t q) { return q >= a && q < b; };
    // sample d of slot j, or zeros where the row does not cover it (only samples of the row are read)
    const auto sample = [&](uint32_t j, uint32_t d) {
      const uint64_t q = p(j) + 4u * d;
      return in_row(q) ? *(XlDlvSrc8)xl_dlv_narrow_src(&r, q) : XlDlv8{0u, 0u};
    };
    const auto load = [&](uint32_t j) {
      XlDlvSpan32 v;
      if (whole(j)) {
        const XlDlvSrc16 s = (XlDlvSrc16)xl_dlv_narrow_src(&r, p(j));
        v.lo = s[0], v.hi = s[1];
      } else {  // a slot the row covers in part, or not at all
        const XlDlv8 s0 = sample(j, 0), s1 = sample(j, 1), s2 = sample(j, 2), s3 = sample(j, 3);
        v.lo = XlDlv16{s0.x, s0.y, s1.x, s1.y}, v.hi = XlDlv16{s2.x, s2.y, s3.x, s3.y};
      }
      return v;
    };
    XlDlvMeter m = {0u, 0u};
    const auto store = [&](uint32_t j, const XlDlvSpan32 &v) {
      const XlDlv16 w = {xl_dlv_gain_pair(v.lo.x, v.lo.y, gr.gain, m), xl_dlv_gain_pair(v.lo.z, v.lo.w, gr.gain, m),
                         xl_dlv_gain_pair(v.hi.x, v.hi.y, gr.gain, m), xl_dlv_gain_pair(v.hi.z, v.hi.w, gr.gain, m)};
      if (whole(j)) {
        *reinterpret_cast<XlDlv16 *>(stage + p(j)) = w;
      } else if (p(j) < sb) {
        for (uint32_t d = 0; d < 4u; ++d) {
          const uint64_t q = p(j) + 4u * d;
          if (in_row(q)) *reinterpret_cast<uint32_t *>(stage + q) = w[d];
        }
      }
    };
    const XlDlvSpan32 v0 = load(0), v1 = load(1), v2 = load(2), v3 = load(3);  // (the loads in flight together)
    store(0, v0), store(1, v1), store(2, v2), store(3, v3);
    // the run's level over this wave; what is zero changes nothing in the table
    const uint32_t peak = xl_dlv_wave(m.peak, [](uint32_t x, uint32_t y) { return x > y ? x : y; });
    const uint32_t counts = xl_dlv_wave(m.counts, [](uint32_t x, uint32_t y) { return x + y; });
    if (tid % 64u == 0u) {
      const XlDlvLevels e = (XlDlvLevels)(levels + (uint64_t)XL_DLV_LEVEL_WORDS * gr.lvl);
      if (peak != 0u) (void)__hip_atomic_fetch_max(e + XL_DLV_LEVEL_PEAK, peak, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (counts % 65536u != 0u)
        (void)__hip_atomic_fetch_add(e + XL_DLV_LEVEL_CLIPPED, counts % 65536u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (counts / 65536u != 0u)
        (void)__hip_atomic_fetch_add(e + XL_DLV_LEVEL_NANS, counts / 65536u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

}  // namespace

int xl_dlv_gain_launch(const XlDlvGainRun *runs, uint32_t nruns, uint32_t chunks, void *stage, uint32_t *levels, hipStream_t st) {
  if (chunks == 0u || nruns == 0u) return 0;
  hipLaunchKernelGGL(xl_dlv_gain_kernel, dim3(chunks), dim3(XL_DLV_THREADS), 0, st, runs, nruns, static_cast<char *>(stage), levels);
  return (int)hipGetLastError();
}
