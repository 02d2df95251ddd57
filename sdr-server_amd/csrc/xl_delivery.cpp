// xl_delivery.cpp -- the delivery object (include/xlating_delivery.h): device rows -> one dense image per batch -> pinned host memory.
// A batch takes a free slot (its device staging, its pinned buffer, its event), lays its rows out (xl_delivery_plan.h), writes the table
// of runs into the banks' ring of pinned tables (xl_bank_host.h) and enqueues: on the caller's stream the table's upload and the pack
// launch (xl_delivery.hip, or for a narrowing batch xl_delivery_narrow.hip, with gains and levels xl_delivery_gain.hip, whose level table
// behind the image is zeroed on the caller's stream first), on the object's copy stream, behind the event `last`, the image's
// device-to-host copy and the slot's event.
// Ordering: `last` is recorded behind every launch and waited for on the next batch's stream before its upload, so the single device
// table is not replaced under a launch that reads it (the banks' rule); the copy stream is one queue, so tickets complete in order.
#include "../../include/xlating_delivery.h"

#include <errno.h>
#include <limits.h>

#include <algorithm>
#include <new>
#include <utility>
#include <vector>

#include "xl_bank_host.h"
#include "xl_common.h"
#include "xl_delivery.h"

#define XL_DLV_MAX_ROWS ((size_t)1 << 24)

namespace {

struct XlDlvSlot {
  char *d_stage = nullptr;  // the image on the device
  char *h_buf = nullptr;    // and in pinned memory
  size_t cap = 0;           // bytes of each
  hipEvent_t done = nullptr;  // behind the image's copy
  int ticket = -1;          // >= 0: in flight or unreleased
  bool copied = false;      // the batch issued a copy (an empty one is done at once)
  bool seen_done = false;
  std::vector<std::pair<int, size_t>> by_key;  // (key, row index), sorted
  std::vector<uint64_t> off, bytes;            // per row
  bool leveled = false;                        // a batch of pack_device_cs16_gain: the level table lies at lvl_off of the image
  uint64_t lvl_off = 0;
  std::vector<uint32_t> lvl;                   // per row: its entry of the level table, or XL_DLV_NO_LEVEL
};

}  // namespace

struct xlating_delivery_t {
  int device = 0;
  hipStream_t copy = nullptr;
  hipEvent_t last = nullptr;  // behind the latest pack launch
  bool packed = false, broken = false;
  XlTableRing ring;
  std::vector<XlDlvSlot> slots;
  int next_ticket = 0;
  unsigned launches = 0, copies = 0;
  uint64_t d2h_bytes = 0;
  std::vector<uint64_t> src, count;  // (scratch of a call)
  std::vector<XlDlvRun> runs;
  std::vector<XlDlvGainRun> gruns;
};

static XlDlvSlot *xl_dlv_slot(xlating_delivery *d, int ticket) {
  if (d == nullptr || ticket < 0) return nullptr;
  for (XlDlvSlot &s : d->slots)
    if (s.ticket == ticket) return &s;
  return nullptr;
}

// 1 done, 0 not yet, -EIO
static int xl_dlv_done(xlating_delivery *d, XlDlvSlot *s) {
  if (!s->copied || s->seen_done) return 1;
  const hipError_t e = hipEventQuery(s->done);
  if (e == hipErrorNotReady) {
    (void)hipGetLastError();  // (not an error: clear the sticky code)
    return 0;
  }
  if (e != hipSuccess) {
    d->broken = true;
    return -EIO;
  }
  s->seen_done = true;
  return 1;
}

extern "C" int xlating_delivery_create(unsigned slots, xlating_delivery **out) {
  if (out == nullptr) return -EINVAL;
  *out = nullptr;
  if (slots < 2u || slots > 16u) return -EINVAL;
  const int device = xl_hip_select_device(-1);
  if (device < 0) {
    XL_LOG_ERR("xlating_delivery_create: no usable HIP device (%s); there is no CPU path", xlating_hip_device_info());
    return -ENODEV;
  }
  xlating_delivery *d = new (std::nothrow) xlating_delivery_t();
  if (d == nullptr) return -ENOMEM;
  d->device = device;
  hipError_t e = hipSuccess;
  try {
    d->slots.resize(slots);
  } catch (const std::bad_alloc &) {
    delete d;
    return -ENOMEM;
  }
  e = hipSetDevice(device);
  if (e == hipSuccess) e = hipStreamCreateWithFlags(&d->copy, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&d->last, hipEventDisableTiming);
  if (e == hipSuccess) e = xl_ring_init(&d->ring);
  for (XlDlvSlot &s : d->slots)
    if (e == hipSuccess) e = hipEventCreateWithFlags(&s.done, hipEventDisableTiming);
  if (e != hipSuccess) {
    xl_last_hip_error = e;
    XL_LOG_ERR("xlating_delivery_create: %s", hipGetErrorString(e));
    const int rc = xl_errno_of_last_hip_error();
    xlating_delivery_destroy(d);
    return rc;
  }
  *out = d;
  return 0;
}

// the slot's buffers hold `need` bytes; on failure the slot holds none and stays usable
static int xl_dlv_reserve(XlDlvSlot *s, size_t need) {
  if (need <= s->cap) return 0;
  if (s->d_stage) (void)hipFree(s->d_stage);
  if (s->h_buf) (void)hipHostFree(s->h_buf);
  s->d_stage = s->h_buf = nullptr, s->cap = 0;
  const size_t cap = std::max<size_t>(need + need / 8, 1u << 16);
  hipError_t e = hipMalloc(reinterpret_cast<void **>(&s->d_stage), cap);
  if (e == hipSuccess) e = hipHostMalloc(reinterpret_cast<void **>(&s->h_buf), cap, hipHostMallocDefault);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    XL_LOG_ERR("delivery: staging of %zu bytes: %s", cap, hipGetErrorString(e));
    if (s->d_stage) (void)hipFree(s->d_stage);
    s->d_stage = s->h_buf = nullptr;
    return -ENOMEM;
  }
  s->cap = cap;
  return 0;
}

// count: a row's bytes, or with `narrow` its cf32 samples, which cross as cs16; gain (narrow only): per row, or nullptr for the plain rule
static int xl_dlv_pack(xlating_delivery *d, bool narrow, size_t n, const int *keys, const void *const *dev_rows, const size_t *count,
                       const int8_t *gain, hipStream_t st) {
  XlDlvSlot *s = nullptr;
  for (XlDlvSlot &c : d->slots)
    if (c.ticket < 0 && s == nullptr) s = &c;
  if (s == nullptr) return -EAGAIN;
  // the layout, and the keys in order
  s->by_key.resize(n), s->off.resize(n), s->bytes.resize(n), d->src.resize(n), d->count.resize(n), d->runs.resize(n);
  for (size_t i = 0; i < n; ++i) {
    s->by_key[i] = std::make_pair(keys[i], i);
    d->count[i] = count[i], d->src[i] = count[i] > 0 ? (uint64_t)reinterpret_cast<uintptr_t>(dev_rows[i]) : 0u;
  }
  std::sort(s->by_key.begin(), s->by_key.end());
  for (size_t i = 1; i < n; ++i)
    if (s->by_key[i].first == s->by_key[i - 1].first) return -EINVAL;
  size_t nruns = 0;
  uint64_t total = 0, lvl_off = 0, full = 0;  // (full: what crosses to the host -- the image, with gains also the level table)
  if (gain != nullptr) s->lvl.resize(n), d->gruns.resize(n);
  const int planned = gain != nullptr ? xl_dlv_plan_gain(n, d->src.data(), d->count.data(), gain, s->off.data(), s->lvl.data(),
                                                         d->runs.data(), d->gruns.data(), &nruns, &total, &lvl_off, &full)
                      : narrow        ? xl_dlv_plan_narrow(n, d->src.data(), d->count.data(), s->off.data(), d->runs.data(), &nruns, &total)
                                      : xl_dlv_plan(n, d->src.data(), d->count.data(), s->off.data(), d->runs.data(), &nruns, &total);
  if (planned != 0) return -EINVAL;
  if (gain == nullptr) full = total;
  for (size_t i = 0; i < n; ++i) s->bytes[i] = narrow ? 4u * d->count[i] : d->count[i];  // (of the delivered row)
  XlRingTable *t = nullptr;
  const size_t tbytes = nruns * (gain != nullptr ? sizeof(XlDlvGainRun) : sizeof(XlDlvRun));
  if (nruns > 0) {
    XL_TRY_RET(hipSetDevice(d->device));
    const int rc = xl_dlv_reserve(s, (size_t)full);
    if (rc != 0) return rc;
    const hipError_t ea = xl_ring_acquire(&d->ring, tbytes, &t);
    if (ea == hipErrorOutOfMemory) {  // (the pinned table could not grow: nothing was done)
      (void)hipGetLastError();
      return -ENOMEM;
    }
    XL_TRY_RET(ea);  // (anything else, e.g. the wait for the table's previous upload: -EIO, the object is broken)
    if (d->ring.d_cap < tbytes) {
      if (d->packed) XL_TRY_RET(hipEventSynchronize(d->last));  // (the previous launch reads the table that is replaced)
      if (xl_ring_dev_grow(&d->ring, tbytes) != hipSuccess) {
        (void)hipGetLastError();
        return -ENOMEM;  // (the ring holds no device table now; the next batch allocates one)
      }
    }
  }
  // from here on the batch exists
  d->launches = d->copies = 0, d->d2h_bytes = 0;
  s->copied = false, s->seen_done = false;
  s->leveled = gain != nullptr, s->lvl_off = lvl_off;
  const int ticket = d->next_ticket;
  if (nruns > 0) {
    if (gain != nullptr) std::copy(d->gruns.begin(), d->gruns.begin() + (ptrdiff_t)nruns, static_cast<XlDlvGainRun *>(t->h));
    else std::copy(d->runs.begin(), d->runs.begin() + (ptrdiff_t)nruns, static_cast<XlDlvRun *>(t->h));
    if (d->packed) XL_TRY_RET(hipStreamWaitEvent(st, d->last, 0));
    XL_TRY_RET(xl_ring_upload(&d->ring, t, tbytes, st));
    d->copies += 1;
    if (gain != nullptr) {  // the level table starts at zero: a memset node on the launch's stream, counted with the copies
      XL_TRY_RET(hipMemsetAsync(s->d_stage + lvl_off, 0, (size_t)(full - lvl_off), st));
      d->copies += 1;
      XL_TRY_RET(xl_dlv_gain_launch(static_cast<const XlDlvGainRun *>(d->ring.d_tab), (uint32_t)nruns, xl_dlv_chunks(total), s->d_stage,
                                    reinterpret_cast<uint32_t *>(s->d_stage + lvl_off), st));
    } else {
      XL_TRY_RET((narrow ? xl_dlv_narrow_launch : xl_dlv_launch)(static_cast<const XlDlvRun *>(d->ring.d_tab), (uint32_t)nruns,
                                                                 xl_dlv_chunks(total), s->d_stage, st));
    }
    d->launches += 1;
    XL_TRY_RET(hipEventRecord(d->last, st));
    d->packed = true;
    XL_TRY_RET(hipStreamWaitEvent(d->copy, d->last, 0));
    XL_TRY_RET(hipMemcpyAsync(s->h_buf, s->d_stage, (size_t)full, hipMemcpyDeviceToHost, d->copy));
    d->copies += 1, d->d2h_bytes = full;
    XL_TRY_RET(hipEventRecord(s->done, d->copy));
    s->copied = true;
  }
  s->ticket = ticket;
  d->next_ticket = ticket == INT_MAX ? 0 : ticket + 1;
  return ticket;
}

static int xl_dlv_pack_checked(xlating_delivery *d, bool narrow, size_t n, const int *keys, const void *const *dev_rows,
                               const size_t *count, const int8_t *gain, void *hip_stream) {
  if (d == nullptr || n > XL_DLV_MAX_ROWS || (n > 0 && (keys == nullptr || dev_rows == nullptr || count == nullptr))) return -EINVAL;
  if (d->broken) return -EIO;
  int rc;
  try {
    rc = xl_dlv_pack(d, narrow, n, keys, dev_rows, count, gain, static_cast<hipStream_t>(hip_stream));
  } catch (const std::bad_alloc &) {  // (the call's vectors are sized before anything is enqueued)
    rc = -ENOMEM;
  }
  if (rc == -EIO) d->broken = true;
  return rc;
}

extern "C" int xlating_delivery_pack_device(xlating_delivery *d, size_t n, const int *keys, const void *const *dev_rows,
                                            const size_t *bytes, void *hip_stream) {
  return xl_dlv_pack_checked(d, false, n, keys, dev_rows, bytes, nullptr, hip_stream);
}

extern "C" int xlating_delivery_pack_device_cs16(xlating_delivery *d, size_t n, const int *keys, const void *const *dev_rows,
                                                 const size_t *n_complex, void *hip_stream) {
  return xl_dlv_pack_checked(d, true, n, keys, dev_rows, n_complex, nullptr, hip_stream);
}

extern "C" int xlating_delivery_pack_device_cs16_gain(xlating_delivery *d, size_t n, const int *keys, const void *const *dev_rows,
                                                      const size_t *n_complex, const int8_t *gain_log2, void *hip_stream) {
  static const int8_t none = 0;  // (n == 0: no gain is read)
  if (n > 0 && gain_log2 == nullptr) return -EINVAL;
  return xl_dlv_pack_checked(d, true, n, keys, dev_rows, n_complex, n > 0 ? gain_log2 : &none, hip_stream);
}

extern "C" int xlating_delivery_query(xlating_delivery *d, int ticket) {
  XlDlvSlot *s = xl_dlv_slot(d, ticket);
  if (s == nullptr) return -EINVAL;
  if (d->broken) return -EIO;
  return xl_dlv_done(d, s);
}

extern "C" int xlating_delivery_wait(xlating_delivery *d, int ticket) {
  XlDlvSlot *s = xl_dlv_slot(d, ticket);
  if (s == nullptr) return -EINVAL;
  if (d->broken) return -EIO;
  if (!s->copied || s->seen_done) return 0;
  if (hipEventSynchronize(s->done) != hipSuccess) {
    d->broken = true;
    return -EIO;
  }
  s->seen_done = true;
  return 0;
}

extern "C" int xlating_delivery_row(xlating_delivery *d, int ticket, int key, const void **host, size_t *bytes) {
  XlDlvSlot *s = xl_dlv_slot(d, ticket);
  if (s == nullptr || host == nullptr || bytes == nullptr) return -EINVAL;
  if (d->broken) return -EIO;
  const auto it = std::lower_bound(s->by_key.begin(), s->by_key.end(), std::make_pair(key, (size_t)0));
  if (it == s->by_key.end() || it->first != key) return -EINVAL;
  const int done = xl_dlv_done(d, s);
  if (done <= 0) return done < 0 ? done : -EBUSY;
  const size_t i = it->second;
  *host = s->bytes[i] > 0 ? s->h_buf + s->off[i] : nullptr;
  *bytes = (size_t)s->bytes[i];
  return 0;
}

extern "C" int xlating_delivery_row_level(xlating_delivery *d, int ticket, int key, uint32_t *peak_bits, uint32_t *clipped,
                                          uint32_t *nans) {
  XlDlvSlot *s = xl_dlv_slot(d, ticket);
  if (s == nullptr || peak_bits == nullptr || clipped == nullptr || nans == nullptr) return -EINVAL;
  if (d->broken) return -EIO;
  const auto it = std::lower_bound(s->by_key.begin(), s->by_key.end(), std::make_pair(key, (size_t)0));
  if (it == s->by_key.end() || it->first != key) return -EINVAL;
  if (!s->leveled) return -ENODATA;
  const int done = xl_dlv_done(d, s);
  if (done <= 0) return done < 0 ? done : -EBUSY;
  const uint32_t at = s->lvl[it->second];
  *peak_bits = *clipped = *nans = 0u;
  if (at == XL_DLV_NO_LEVEL) return 0;  // (an empty row)
  const uint32_t *e = reinterpret_cast<const uint32_t *>(s->h_buf + s->lvl_off) + (size_t)XL_DLV_LEVEL_WORDS * at;
  *peak_bits = e[XL_DLV_LEVEL_PEAK], *clipped = e[XL_DLV_LEVEL_CLIPPED], *nans = e[XL_DLV_LEVEL_NANS];
  return 0;
}

extern "C" int xlating_delivery_release(xlating_delivery *d, int ticket) {
  XlDlvSlot *s = xl_dlv_slot(d, ticket);
  if (s == nullptr) return -EINVAL;
  if (!d->broken) {
    const int done = xl_dlv_done(d, s);
    if (done <= 0) return done < 0 ? done : -EBUSY;
  }
  s->ticket = -1;
  return d->broken ? -EIO : 0;
}

extern "C" int xlating_delivery_last_ops(const xlating_delivery *d, unsigned *launches, unsigned *copies, uint64_t *d2h_bytes) {
  if (d == nullptr) return -EINVAL;
  if (launches) *launches = d->launches;
  if (copies) *copies = d->copies;
  if (d2h_bytes) *d2h_bytes = d->d2h_bytes;
  return 0;
}

extern "C" unsigned xlating_delivery_chunk_bytes(void) { return XL_DLV_CHUNK; }

extern "C" void xlating_delivery_destroy(xlating_delivery *d) {
  if (d == nullptr) return;
  (void)hipSetDevice(d->device);
  if (d->packed) (void)hipEventSynchronize(d->last);
  if (d->copy) (void)hipStreamSynchronize(d->copy);
  xl_ring_destroy(&d->ring);
  for (XlDlvSlot &s : d->slots) {
    if (s.d_stage) (void)hipFree(s.d_stage);
    if (s.h_buf) (void)hipHostFree(s.h_buf);
    if (s.done) (void)hipEventDestroy(s.done);
  }
  if (d->last) (void)hipEventDestroy(d->last);
  if (d->copy) (void)hipStreamDestroy(d->copy);
  delete d;
}
