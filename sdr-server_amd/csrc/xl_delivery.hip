// xl_delivery.hip -- the ragged pack kernel of the delivery object (include/xlating_delivery.h): ONE launch copies every row of a batch
// into the dense image that one device-to-host copy then moves.  The layout is xl_delivery_plan.h's and nothing here decides any of
// it: a workgroup takes chunk blockIdx.x of the image, finds its first run (xl_ragged_find + xl_dlv_first) and moves xl_dlv_span of
// every run up to the chunk's end.  A run's image offset is congruent to its source address mod 16, so a whole 16-byte slot of the
// image inside a row is one aligned 16-byte load and one aligned 16-byte store; a slot a row covers in part (its head, its tail, a
// slot shared by short rows) moves dword by dword.  Dwords only: no floating-point instruction, scalar or packed (the kernel may run
// beside the engine's matrix-core launches; tests/test_delivery_cpu.py reads the code object).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "xl_delivery.h"
#include "xl_ragged.h"

namespace {

// (global address space stated: an address that comes out of a table would otherwise be loaded through the flat path)
typedef uint32_t XlDlv16 __attribute__((ext_vector_type(4)));
typedef const XlDlv16 __attribute__((address_space(1))) *XlDlvSrc16;
typedef const uint32_t __attribute__((address_space(1))) *XlDlvSrc4;

static_assert(XL_DLV_SLOTS_PER_THREAD == 4u, "the kernel body names four slots per thread");

__global__ void __launch_bounds__(XL_DLV_THREADS) xl_dlv_pack_kernel(const XlDlvRun *__restrict__ runs, const uint32_t nruns,
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
    const uint64_t src = r.src - r.off;  // (mod 2^64) image offset p of this row is the byte at address src + p
    const auto p = [&](uint32_t j) { return sa + 16u * (tid + XL_DLV_THREADS * j); };
    const auto whole = [&](uint32_t j) { return p(j) >= a && p(j) + 16u <= b; };
    const auto load = [&](uint32_t j) { return whole(j) ? *(XlDlvSrc16)(src + p(j)) : XlDlv16{0u, 0u, 0u, 0u}; };
    const auto store = [&](uint32_t j, const XlDlv16 v) {
      if (whole(j)) {
        *reinterpret_cast<XlDlv16 *>(stage + p(j)) = v;
      } else if (p(j) < sb) {  // a slot the row covers in part: its head, its tail
        for (uint32_t d = 0; d < 4u; ++d) {
          const uint64_t q = p(j) + 4u * d;
          if (q >= a && q < b) *reinterpret_cast<uint32_t *>(stage + q) = *(XlDlvSrc4)(src + q);
        }
      }
    };
    const XlDlv16 v0 = load(0), v1 = load(1), v2 = load(2), v3 = load(3);  // (the loads in flight together)
    store(0, v0), store(1, v1), store(2, v2), store(3, v3);
  }
}

}  // namespace

int xl_dlv_launch(const XlDlvRun *runs, uint32_t nruns, uint32_t chunks, void *stage, hipStream_t st) {
  if (chunks == 0u || nruns == 0u) return 0;
  hipLaunchKernelGGL(xl_dlv_pack_kernel, dim3(chunks), dim3(XL_DLV_THREADS), 0, st, runs, nruns, static_cast<char *>(stage));
  return (int)hipGetLastError();
}
