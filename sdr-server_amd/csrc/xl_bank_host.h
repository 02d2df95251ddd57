// xl_bank_host.h -- the host-side scheme the banks share (xl_resample.cpp: both resampler banks; xl_spectrum_bank.cpp): the ring of
// pinned tables behind the single device table, and the per-stream device arrays that grow as streams are added.  Header-only,
// included by libxlating_resample.so and libxlating_spectrum.so; nothing here is exported.
// THE RULES (stated here once; the banks' files point here):
//   - A bank has ONE device table.  Every feed is ordered behind the previous feed's work by the bank's event `last` (waited for on
//     the feed's stream before its first operation, recorded behind its last), so an upload cannot overtake the launches that still
//     read the table.
//   - The host writes a table into one of XL_BANK_TABLES pinned buffers, taken in turn.  A buffer's event is recorded behind the copy
//     that read it; xl_ring_acquire waits for THAT event before the buffer is written again, and for nothing else: a feed waits for
//     the upload XL_BANK_TABLES back, not for the previous one.  A buffer too small is freed (after that wait) and allocated at
//     max(2 * bytes, 64 KiB); a failed allocation leaves the slot empty and usable.
//   - Before the DEVICE table is replaced (d_cap < bytes) the caller waits for what reads it, because the banks differ: the resampler
//     bank uploads once per feed and waits for `last`; the spectrum bank uploads once per round and synchronises the feed's stream
//     (this feed's earlier rounds read the table, and they lie behind `last`).  xl_ring_dev_grow then frees and allocates 2 * bytes;
//     when that fails the ring holds no device table (d_cap == 0).
//   - Before the PER-STREAM arrays are replaced the caller waits for `last`.  xl_streams_grow allocates all new arrays, zeroes those
//     flagged, copies the old contents over on the bank's own stream and synchronises it.  On any failure every NEW array is freed and
//     the old ones stay in place, capacity unchanged; only on success are they swapped and the old ones freed.
#ifndef XL_BANK_HOST_H_
#define XL_BANK_HOST_H_

#include <algorithm>

#include "xl_common.h"

#define XL_BANK_TABLES 4

struct XlRingTable {
  void *h = nullptr;  // pinned
  size_t cap = 0;
  hipEvent_t ev = nullptr;  // behind the latest copy out of h
  bool used = false;
};

struct XlTableRing {
  XlRingTable tab[XL_BANK_TABLES];
  int next = 0;
  void *d_tab = nullptr;  // the device table
  size_t d_cap = 0;
};

static inline hipError_t xl_ring_init(XlTableRing *g) {
  hipError_t e = hipSuccess;
  for (int i = 0; i < XL_BANK_TABLES && e == hipSuccess; ++i) e = hipEventCreateWithFlags(&g->tab[i].ev, hipEventDisableTiming);
  return e;
}

// a pinned table of at least `bytes`, free for writing
static inline hipError_t xl_ring_acquire(XlTableRing *g, size_t bytes, XlRingTable **out) {
  XlRingTable &t = g->tab[g->next];
  g->next = (g->next + 1) % XL_BANK_TABLES;
  hipError_t e = t.used ? hipEventSynchronize(t.ev) : hipSuccess;
  if (e == hipSuccess && t.cap < bytes) {
    if (t.h) (void)hipHostFree(t.h);
    t.h = nullptr, t.cap = 0;
    const size_t cap = std::max<size_t>(bytes * 2, 1u << 16);
    if ((e = hipHostMalloc(&t.h, cap, hipHostMallocDefault)) == hipSuccess) t.cap = cap;
  }
  *out = &t;
  return e;
}

// replaces the device table by one of 2 * bytes; the caller has waited for everything that reads the present one
static inline hipError_t xl_ring_dev_grow(XlTableRing *g, size_t bytes) {
  if (g->d_tab) (void)hipFree(g->d_tab);
  g->d_tab = nullptr, g->d_cap = 0;
  const hipError_t e = hipMalloc(&g->d_tab, bytes * 2);
  if (e == hipSuccess) g->d_cap = bytes * 2;
  return e;
}

// t's first `bytes` to the device table on st; t is busy until that copy is through
static inline hipError_t xl_ring_upload(XlTableRing *g, XlRingTable *t, size_t bytes, hipStream_t st) {
  hipError_t e = hipMemcpyAsync(g->d_tab, t->h, bytes, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipEventRecord(t->ev, st);
  if (e == hipSuccess) t->used = true;
  return e;
}

// (the caller has waited for the bank's work)
static inline void xl_ring_destroy(XlTableRing *g) {
  for (XlRingTable &t : g->tab) {
    if (t.h) (void)hipHostFree(t.h);
    if (t.ev) (void)hipEventDestroy(t.ev);
  }
  if (g->d_tab) (void)hipFree(g->d_tab);
}

struct XlStreamArray {
  void **d;       // the bank's pointer to the array: [capacity][stride bytes]
  size_t stride;  // bytes per stream
  bool zero;      // a new array starts zeroed (one that does not is written before it is read)
};

// room for `need` streams in every array of a[]: the capacity doubles from `first` (64; fewer where a stream's state is large: the wide
// spectrum bank) until it fits.  The caller has found need > *cap and has waited for `last`.  what: names the bank and the arrays in the
// error line.
template <size_t N>
static inline int xl_streams_grow(uint32_t *cap, uint32_t need, const XlStreamArray (&a)[N], hipStream_t own, const char *what,
                                  uint32_t first = 64u) {
  uint32_t ncap = *cap ? *cap * 2u : first;
  while (ncap < need) ncap *= 2u;
  void *fresh[N] = {};
  hipError_t e = hipSuccess;
  for (size_t i = 0; i < N && e == hipSuccess; ++i) e = hipMalloc(&fresh[i], a[i].stride * ncap);
  for (size_t i = 0; i < N && e == hipSuccess; ++i)
    if (a[i].zero) e = hipMemsetAsync(fresh[i], 0, a[i].stride * ncap, own);
  for (size_t i = 0; i < N && e == hipSuccess && *cap > 0; ++i)
    e = hipMemcpyAsync(fresh[i], *a[i].d, a[i].stride * *cap, hipMemcpyDeviceToDevice, own);
  if (e == hipSuccess) e = hipStreamSynchronize(own);
  if (e != hipSuccess) {
    xl_last_hip_error = e;
    XL_LOG_ERR("%s of %u streams: %s", what, ncap, hipGetErrorString(e));
    for (void *p : fresh)
      if (p) (void)hipFree(p);
    return e == hipErrorOutOfMemory ? -ENOMEM : -EIO;
  }
  for (size_t i = 0; i < N; ++i) {
    if (*a[i].d) (void)hipFree(*a[i].d);
    *a[i].d = fresh[i];
  }
  *cap = ncap;
  return 0;
}

#endif
