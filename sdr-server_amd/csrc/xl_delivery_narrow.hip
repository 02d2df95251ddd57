// xl_delivery_narrow.hip -- the narrowing pack kernel of the delivery object (xlating_delivery_pack_device_cs16): ONE launch turns every
// cf32 row of a batch into the cs16 row of the dense image that one device-to-host copy then moves, half the bytes of the plain pack
// (xl_delivery.hip).  The layout is xl_delivery_plan.h's and the arithmetic xl_dlv_narrow.h's; nothing here decides any of either: a
// workgroup takes chunk blockIdx.x of the image, finds its first run (xl_ragged_find + xl_dlv_first) and moves xl_dlv_span of every run
// up to the chunk's end, reading image offset p of a run from xl_dlv_narrow_src.  A whole 16-byte slot of the image inside a row is one
// 32-byte-aligned span of the source: two aligned 16-byte loads, eight conversions, one aligned 16-byte store; a slot a row covers in
// part (its head, its tail, a slot shared by short rows) moves sample by sample, one 8-byte load and one dword store each.  All of a
// thread's loads are issued before its first store.  Integer instructions only: the conversion works on the floats' bit fields, so
// there is no floating-point instruction, scalar or packed (the kernel may run beside the engine's matrix-core launches, DESIGN
// section 5; tests/test_delivery_narrow_cpu.py reads the code object).  The sources are only read.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "xl_delivery.h"
#include "xl_dlv_narrow.h"
#include "xl_ragged.h"

namespace {

// (global address space stated: an address that comes out of a table would otherwise be loaded through the flat path)
typedef uint32_t XlDlv16 __attribute__((ext_vector_type(4)));
typedef uint32_t XlDlv8 __attribute__((ext_vector_type(2)));
typedef const XlDlv16 __attribute__((address_space(1))) *XlDlvSrc16;
typedef const XlDlv8 __attribute__((address_space(1))) *XlDlvSrc8;

struct XlDlvSpan32 {  // the 32 source bytes of one image slot: four samples
  XlDlv16 lo, hi;
};

static_assert(XL_DLV_SLOTS_PER_THREAD == 4u, "the kernel body names four slots per thread");

// one cf32 sample (re, im) -> the dword of its cs16 pair, re in the low half
__device__ static inline uint32_t xl_dlv_narrow_pair(const uint32_t re, const uint32_t im) {
  return ((uint32_t)xl_dlv_narrow(re) & 0xFFFFu) | ((uint32_t)xl_dlv_narrow(im) << 16);
}

__global__ void __launch_bounds__(XL_DLV_THREADS) xl_dlv_narrow_kernel(const XlDlvRun *__restrict__ runs, const uint32_t nruns,
                                                                        char *__restrict__ stage) {
  const uint32_t c = blockIdx.x, tid = threadIdx.x;
  const uint64_t hi = ((uint64_t)c + 1u) * XL_DLV_CHUNK;
  const uint32_t found = xl_ragged_find(runs, nruns, c * (XL_DLV_CHUNK / 16u), [](const XlDlvRun &r) { return r.s16; });
  for (uint32_t k = xl_dlv_first(runs, found, c); k < nruns; ++k) {
    const XlDlvRun r = runs[k];  // (uniform)
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
    const auto store = [&](uint32_t j, const XlDlvSpan32 &v) {
      const XlDlv16 w = {xl_dlv_narrow_pair(v.lo.x, v.lo.y), xl_dlv_narrow_pair(v.lo.z, v.lo.w), xl_dlv_narrow_pair(v.hi.x, v.hi.y),
                         xl_dlv_narrow_pair(v.hi.z, v.hi.w)};
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
  }
}

}  // namespace

int xl_dlv_narrow_launch(const XlDlvRun *runs, uint32_t nruns, uint32_t chunks, void *stage, hipStream_t st) {
  if (chunks == 0u || nruns == 0u) return 0;
  hipLaunchKernelGGL(xl_dlv_narrow_kernel, dim3(chunks), dim3(XL_DLV_THREADS), 0, st, runs, nruns, static_cast<char *>(stage));
  return (int)hipGetLastError();
}
