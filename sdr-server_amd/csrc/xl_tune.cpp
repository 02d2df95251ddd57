// xl_tune.cpp -- the tuner bank (include/xlating_tune.h): many independent complex float32 streams, each rotated by its own
// phase-continuous shift, advanced by one feed of one launch and one table copy.  The rule is xl_tune_rule.h's; the kernel xl_tune.hip.
//
// A stream's state (P, F, R) lives on the HOST alone: a feed writes it into the stream's run and advances it by the closed form, so
// add, remove, set and state never touch the device.  Device state: one output arena, carved per feed from the counts, which holds
// the latest feed's rows and grows (after a wait) when a feed needs more.  One feed = one table of runs written into pinned memory and
// uploaded by one copy, and the ragged launch.  The ring of pinned tables and the single device table, with the rules of their
// lifetimes, are xl_bank_host.h's (shared with the resampler banks, the spectrum bank and the delivery); a feed does not wait for the
// previous one.
#include "../../include/xlating_tune.h"

#include <errno.h>

#include <algorithm>
#include <new>
#include <vector>

#include "xl_bank_host.h"
#include "xl_common.h"
#include "xl_tune.h"
#include "xl_tune_hz.h"
#include "xl_tune_rule.h"

#define XL_TUNE_MAX_STREAMS 65536

namespace {

struct XlTuneStream {
  bool live = false;
  uint64_t P = 0;
  int64_t F = 0, R = 0;
  uint64_t consumed = 0;
  uint64_t mark = 0;    // the feed that named this stream last (duplicate check)
  uint64_t out_no = 0;  // the arena generation its latest row is in
  size_t out_off = 0, out_n = 0;
};

}  // namespace

struct xlating_tune_bank {
  int device = 0;
  hipEvent_t last = nullptr;  // behind the latest feed's work
  bool fed = false, broken = false;
  std::vector<XlTuneStream> streams;
  std::vector<int> free_ids;
  uint64_t feed_no = 0;
  XlTableRing ring;  // the feeds' tables of runs
  float2 *d_out = nullptr;  // the arena
  size_t out_cap = 0;
  uint64_t out_no = 0;  // generation: the feed whose rows the arena holds
  unsigned launches = 0, copies = 0;
};

static bool xl_tune_live(const xlating_tune_bank *b, int id) {
  return b != nullptr && id >= 0 && (size_t)id < b->streams.size() && b->streams[(size_t)id].live;
}

static int xl_tune_feed(xlating_tune_bank *b, size_t n, const int *ids, const void *const *dev_samples, const size_t *counts,
                        hipStream_t st) {
  b->feed_no++;
  b->launches = b->copies = 0;  // (a refused feed issued nothing)
  for (size_t i = 0; i < n; ++i) {
    if (!xl_tune_live(b, ids[i]) || counts[i] > XL_TUNE_COUNT_MAX || (counts[i] > 0 && dev_samples[i] == nullptr) ||
        ((uintptr_t)dev_samples[i] & 7u) != 0u)
      return -EINVAL;
    XlTuneStream &s = b->streams[(size_t)ids[i]];
    if (s.mark == b->feed_no) return -EINVAL;  // named twice
    s.mark = b->feed_no;
  }
  size_t need = 0, nruns = 0;
  uint64_t wgs = 0;
  for (size_t i = 0; i < n; ++i) {
    need += counts[i];
    wgs += (counts[i] + XL_TUNE_CHUNK - 1u) / XL_TUNE_CHUNK;
    nruns += counts[i] > 0;
  }
  if (wgs >= ((uint64_t)1 << 31)) return -ENOMEM;  // (the ragged launch counts its workgroups in 32 bits)
  XL_TRY_RET(hipSetDevice(b->device));
  // the arena grows.  The bank waits for its own feeds, which write the present one; a caller's launch that still reads it (the serve
  // object's pack, later on the same stream) is covered by hipFree alone, which synchronises the device before it frees
  if (need > b->out_cap) {
    if (b->fed) XL_TRY_RET(hipEventSynchronize(b->last));
    if (b->d_out) (void)hipFree(b->d_out);
    b->d_out = nullptr, b->out_cap = 0, b->out_no = 0;
    const size_t cap = std::max<size_t>(need + need / 2, 1024);
    const hipError_t e = hipMalloc(reinterpret_cast<void **>(&b->d_out), cap * sizeof(float2));
    if (e != hipSuccess) {
      (void)hipGetLastError();
      XL_LOG_ERR("tuner bank: output arena of %zu samples: %s", cap, hipGetErrorString(e));
      return -ENOMEM;  // (nothing consumed)
    }
    b->out_cap = cap;
  }
  const size_t bytes = nruns * sizeof(XlTuneRun);
  XlRingTable *t = nullptr;
  if (nruns > 0) {
    const hipError_t e = xl_ring_acquire(&b->ring, bytes, &t);
    if (e == hipErrorOutOfMemory) {
      (void)hipGetLastError();
      return -ENOMEM;  // (nothing consumed)
    }
    XL_TRY_RET(e);
    if (b->ring.d_cap < bytes) {
      if (b->fed) XL_TRY_RET(hipEventSynchronize(b->last));  // (the previous feed reads the table that is replaced)
      XL_TRY_RET(xl_ring_dev_grow(&b->ring, bytes));
    }
  }
  b->out_no = b->feed_no;
  XlTuneRun *runs = nruns > 0 ? static_cast<XlTuneRun *>(t->h) : nullptr;
  uint32_t W = 0;
  size_t off = 0, k = 0;
  for (size_t i = 0; i < n; ++i) {
    XlTuneStream &s = b->streams[(size_t)ids[i]];
    s.out_no = b->out_no, s.out_off = off, s.out_n = counts[i];
    if (counts[i] == 0) continue;
    XlTuneRun &r = runs[k++];
    r.src = static_cast<const float2 *>(dev_samples[i]);
    r.out = b->d_out + off;
    r.P = s.P, r.F = s.F, r.R = s.R;
    r.cnt = (uint32_t)counts[i], r.wsum = W;
    W += (uint32_t)((counts[i] + XL_TUNE_CHUNK - 1u) / XL_TUNE_CHUNK);
    off += counts[i];
    xl_tune_advance(&s.P, &s.F, s.R, counts[i]);
    s.consumed += counts[i];
  }
  if (nruns == 0) return 0;
  if (b->fed) XL_TRY_RET(hipStreamWaitEvent(st, b->last, 0));
  XL_TRY_RET(xl_ring_upload(&b->ring, t, bytes, st));
  b->copies += 1;
  XL_TRY_RET(xl_tune_launch(static_cast<const XlTuneRun *>(b->ring.d_tab), (uint32_t)nruns, W, st));
  b->launches += 1;
  XL_TRY_RET(hipEventRecord(b->last, st));
  b->fed = true;
  return 0;
}

extern "C" int xlating_tune_bank_create(xlating_tune_bank **out) {
  if (out == nullptr) return -EINVAL;
  *out = nullptr;
  const int device = xl_hip_select_device(-1);
  if (device < 0) {
    XL_LOG_ERR("xlating_tune_bank_create: no usable HIP device (%s); there is no CPU path", xlating_hip_device_info());
    return -ENODEV;
  }
  xlating_tune_bank *b = new (std::nothrow) xlating_tune_bank();
  if (b == nullptr) return -ENOMEM;
  b->device = device;
  hipError_t e = hipSetDevice(device);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&b->last, hipEventDisableTiming);
  if (e == hipSuccess) e = xl_ring_init(&b->ring);
  if (e != hipSuccess) {
    xl_last_hip_error = e;
    XL_LOG_ERR("xlating_tune_bank_create: %s", hipGetErrorString(e));
    const int rc = xl_errno_of_last_hip_error();
    xlating_tune_bank_destroy(b);
    return rc;
  }
  *out = b;
  return 0;
}

extern "C" int xlating_tune_bank_add(xlating_tune_bank *b, uint64_t P, int64_t F, int64_t R) {
  if (b == nullptr) return -EINVAL;
  try {
    const bool reuse = !b->free_ids.empty();
    const size_t id = reuse ? (size_t)b->free_ids.back() : b->streams.size();
    if (id >= XL_TUNE_MAX_STREAMS) return -ENOMEM;
    if (reuse)
      b->free_ids.pop_back();
    else
      b->streams.emplace_back();
    XlTuneStream &s = b->streams[id];
    s = XlTuneStream();
    s.live = true, s.P = P, s.F = F, s.R = R;
    return (int)id;
  } catch (const std::bad_alloc &) {
    return -ENOMEM;
  }
}

extern "C" int xlating_tune_bank_remove(xlating_tune_bank *b, int stream_id) {
  if (!xl_tune_live(b, stream_id)) return -EINVAL;
  XlTuneStream &s = b->streams[(size_t)stream_id];
  s.live = false, s.out_n = 0;
  try {
    b->free_ids.push_back(stream_id);
  } catch (const std::bad_alloc &) {  // (the id is then not reused)
  }
  return 0;
}

extern "C" int xlating_tune_bank_set(xlating_tune_bank *b, int stream_id, int64_t F, int64_t R) {
  if (!xl_tune_live(b, stream_id)) return -EINVAL;
  XlTuneStream &s = b->streams[(size_t)stream_id];
  s.F = F, s.R = R;
  return 0;
}

extern "C" int xlating_tune_bank_feed_device(xlating_tune_bank *b, size_t n, const int *ids, const void *const *dev_samples,
                                             const size_t *counts, void *hip_stream) {
  if (b == nullptr || (n > 0 && (ids == nullptr || dev_samples == nullptr || counts == nullptr))) return -EINVAL;
  if (b->broken) return -EIO;
  const int rc = xl_tune_feed(b, n, ids, dev_samples, counts, static_cast<hipStream_t>(hip_stream));
  if (rc != 0 && rc != -EINVAL && rc != -ENOMEM) b->broken = true;  // (-EINVAL and -ENOMEM are decided before anything is consumed)
  return rc;
}

extern "C" int xlating_tune_bank_output_device(xlating_tune_bank *b, int stream_id, const void **d_out, size_t *n_complex) {
  if (!xl_tune_live(b, stream_id) || d_out == nullptr || n_complex == nullptr) return -EINVAL;
  if (b->broken) return -EIO;
  const XlTuneStream &s = b->streams[(size_t)stream_id];
  const bool have = s.out_no == b->out_no && b->out_no != 0 && s.out_n > 0;
  *d_out = have ? b->d_out + s.out_off : nullptr;
  *n_complex = have ? s.out_n : 0;
  return 0;
}

extern "C" int xlating_tune_bank_state(const xlating_tune_bank *b, int stream_id, uint64_t *P, int64_t *F, int64_t *R,
                                       uint64_t *consumed) {
  if (!xl_tune_live(b, stream_id)) return -EINVAL;
  const XlTuneStream &s = b->streams[(size_t)stream_id];
  if (P) *P = s.P;
  if (F) *F = s.F;
  if (R) *R = s.R;
  if (consumed) *consumed = s.consumed;
  return 0;
}

extern "C" int xlating_tune_bank_last_feed_ops(const xlating_tune_bank *b, unsigned *launches, unsigned *copies) {
  if (b == nullptr) return -EINVAL;
  if (launches) *launches = b->launches;
  if (copies) *copies = b->copies;
  return 0;
}

extern "C" void xlating_tune_bank_destroy(xlating_tune_bank *b) {
  if (b == nullptr) return;
  (void)hipSetDevice(b->device);
  if (b->fed) (void)hipEventSynchronize(b->last);
  xl_ring_destroy(&b->ring);
  if (b->d_out) (void)hipFree(b->d_out);
  if (b->last) (void)hipEventDestroy(b->last);
  delete b;
}

extern "C" void xlating_tune_cs(uint32_t p, float *c, float *s) {
  float cc, ss;
  xl_tune_cs(p, &cc, &ss);
  if (c) *c = cc;
  if (s) *s = ss;
}

extern "C" int xlating_tune_from_hz(double shift_hz, double ramp_hz_per_s, double rate, int64_t *F, int64_t *R) {
  if (F == nullptr || R == nullptr) return -EINVAL;
  return xl_tune_from_hz(shift_hz, ramp_hz_per_s, rate, F, R);
}

extern "C" unsigned xlating_tune_chunk_samples(void) { return XL_TUNE_CHUNK; }
