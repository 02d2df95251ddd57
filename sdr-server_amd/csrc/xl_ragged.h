// xl_ragged.h -- the search of a ragged launch: which run a workgroup (or a packed transform) belongs to.  Header-only, no runtime
// calls.  The host writes one run per stream with the running sum of the units (workgroups, transforms) before it; unit `key` of the
// launch belongs to the LAST run whose sum is <= key.  runs[0]'s sum is 0, so there is one; a run without units shares its successor's
// sum and is never found.  Called by xl_rs_kernel, xl_rsq_kernel (sum: wsum) and xl_bank_kernel (sum: tsum).
#ifndef XL_RAGGED_H_
#define XL_RAGGED_H_

#include <stdint.h>

// sum: the run's running sum, e.g. [](const XlRsRun &r) { return r.wsum; }.  nruns >= 1.
// (hi before lo, each assigned by a select: with this spelling the three kernels' instruction text is what
// profiles/banks_shared_vs_parent.txt records; others move one operand or one select)
template <typename Run, typename Sum>
__device__ static inline __attribute__((always_inline)) uint32_t xl_ragged_find(const Run *runs, const uint32_t nruns, const uint32_t key, const Sum sum) {
  uint32_t hi = nruns, lo = 0u;
  while (hi - lo > 1u) {
    const uint32_t mid = (lo + hi) / 2u;
    const bool le = sum(runs[mid]) <= key;
    hi = le ? hi : mid;
    lo = le ? mid : lo;
  }
  return lo;
}

#endif
