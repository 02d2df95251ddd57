// xl_resample.cpp -- the resampler bank (include/xlating_resample.h): many independent complex float32 streams, each resampled by its
// own rational factor, advanced by one feed of two launches and one table copy.  Kernels: xl_resample.hip; what a feed of n samples
// holds for a stream: xl_resample_cut.h.
//
// Device state: per stream id a carry slot of XL_RS_CARRY_SLOT samples (the last Q - 1 inputs; zero for a new stream), in one array
// that grows as streams are added; per distinct (L, M, taps) one phase-major tap table, reference-counted; one output arena, carved per
// feed from the host-computed output counts, which holds the latest feed's outputs and grows (after a wait) when a feed needs more.
// One feed = one table of runs written into pinned memory and uploaded by one copy, the ragged resampling launch, the carry launch.
// The pinned tables are multi-buffered behind events, so a feed does not wait for the previous one; every feed is ordered behind the
// previous feed's work by an event, so the single device table, the carries and the arena need no copies of their own.
#include "../../include/xlating_resample.h"

#include <errno.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <new>
#include <vector>

#include "xl_common.h"
#include "xl_resample.h"
#include "xl_resample_cut.h"

#define XL_RS_TABLES 4
#define XL_RS_MAX_STREAMS 65536
#define XL_RS_COUNT_MAX ((size_t)1 << 30)

#define XL_RS_TRY(expr)                                                                         \
  do {                                                                                          \
    hipError_t xl_e_ = (hipError_t)(expr);                                                      \
    if (xl_e_ != hipSuccess) {                                                                  \
      xl_last_hip_error = xl_e_;                                                                \
      XL_LOG_ERR("%s failed: %s (%s:%d)", #expr, hipGetErrorString(xl_e_), __FILE__, __LINE__); \
      return xl_e_ == hipErrorOutOfMemory ? -ENOMEM : -EIO;                                     \
    }                                                                                           \
  } while (0)

namespace {

struct XlRsTaps {  // one device tap table and the streams' common definition
  uint32_t L = 0, M = 0, Q = 0;
  std::vector<float> taps;
  float *d = nullptr;  // [L][Q]
  size_t bytes = 0;
  unsigned refs = 0;
};

struct XlRsStream {
  bool live = false;
  XlRsTaps *t = nullptr;
  uint64_t P = 0;      // samples consumed
  uint64_t mark = 0;   // the feed that named this stream last (duplicate check)
  uint64_t out_no = 0; // the arena generation its latest outputs are in
  size_t out_off = 0, out_n = 0;
};

struct XlRsPinned {
  void *h = nullptr;
  size_t cap = 0;
  hipEvent_t ev = nullptr;
  bool used = false;
};

}  // namespace

struct xlating_resample_bank {
  int device = 0;
  hipStream_t own = nullptr;  // growth and clearing of the per-stream state, the fetch
  hipEvent_t last = nullptr;  // behind the latest feed's work
  bool fed = false, broken = false;
  uint32_t cap_streams = 0;
  float2 *d_carry = nullptr;  // [cap_streams][XL_RS_CARRY_SLOT]
  std::vector<XlRsStream> streams;
  std::vector<int> free_ids;
  unsigned nlive = 0;
  std::vector<XlRsTaps *> tables;
  uint64_t feed_no = 0;
  XlRsPinned tab[XL_RS_TABLES];
  int tab_i = 0;
  void *d_tab = nullptr;
  size_t d_tab_cap = 0;
  float2 *d_out = nullptr;  // the arena
  size_t out_cap = 0, out_used = 0;
  uint64_t out_no = 0;      // generation: the feed whose outputs the arena holds
  float2 *h_out = nullptr;  // the fetched copy
  size_t h_cap = 0;
  uint64_t h_no = 0;
  unsigned launches = 0, copies = 0;
  std::vector<XlRsRun> runs;
  std::vector<XlResampleCut> cuts;
};

static bool xl_rs_live(const xlating_resample_bank *b, int id) {
  return b != nullptr && id >= 0 && (size_t)id < b->streams.size() && b->streams[(size_t)id].live;
}

static uint32_t xl_rs_gcd(uint32_t a, uint32_t c) {
  while (c != 0u) {
    const uint32_t r = a % c;
    a = c, c = r;
  }
  return a;
}

// carry slots for `need` streams: the array is replaced by a larger one and the present streams' carries move over
static int xl_rs_reserve_streams(xlating_resample_bank *b, uint32_t need) {
  if (need <= b->cap_streams) return 0;
  uint32_t cap = b->cap_streams ? b->cap_streams * 2u : 64u;
  while (cap < need) cap *= 2u;
  const size_t slot = (size_t)XL_RS_CARRY_SLOT * sizeof(float2);
  if (b->fed) XL_RS_TRY(hipEventSynchronize(b->last));
  float2 *carry = nullptr;
  hipError_t e = hipMalloc(&carry, slot * cap);
  if (e == hipSuccess) e = hipMemsetAsync(carry, 0, slot * cap, b->own);
  if (e == hipSuccess && b->cap_streams > 0) e = hipMemcpyAsync(carry, b->d_carry, slot * b->cap_streams, hipMemcpyDeviceToDevice, b->own);
  if (e == hipSuccess) e = hipStreamSynchronize(b->own);
  if (e != hipSuccess) {
    xl_last_hip_error = e;
    XL_LOG_ERR("resampler bank: carries of %u streams: %s", cap, hipGetErrorString(e));
    if (carry) (void)hipFree(carry);
    return e == hipErrorOutOfMemory ? -ENOMEM : -EIO;
  }
  if (b->d_carry) (void)hipFree(b->d_carry);
  b->d_carry = carry, b->cap_streams = cap;
  return 0;
}

// the table of (L, M, taps): the one that exists, or a new one uploaded phase-major
static int xl_rs_taps(xlating_resample_bank *b, uint32_t L, uint32_t M, const float *taps, size_t len, XlRsTaps **out) {
  for (XlRsTaps *t : b->tables)
    if (t->L == L && t->M == M && t->taps.size() == len && memcmp(t->taps.data(), taps, len * sizeof(float)) == 0) {
      *out = t;
      return 0;
    }
  XlRsTaps *t = new XlRsTaps();
  t->L = L, t->M = M, t->Q = (uint32_t)((len + L - 1u) / L);
  t->bytes = (size_t)L * t->Q * sizeof(float);
  int rc = 0;
  try {
    t->taps.assign(taps, taps + len);
    std::vector<float> pm((size_t)L * t->Q, 0.0f);
    for (size_t i = 0; i < len; ++i) pm[(i % L) * t->Q + i / L] = taps[i];
    hipError_t e = hipMalloc(&t->d, t->bytes);
    if (e == hipSuccess) e = hipMemcpy(t->d, pm.data(), t->bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
      xl_last_hip_error = e;
      XL_LOG_ERR("resampler bank: tap table of %u x %u: %s", L, t->Q, hipGetErrorString(e));
      rc = e == hipErrorOutOfMemory ? -ENOMEM : -EIO;
    }
    if (rc == 0) b->tables.push_back(t);
  } catch (const std::bad_alloc &) {
    rc = -ENOMEM;
  }
  if (rc != 0) {
    if (t->d) (void)hipFree(t->d);
    delete t;
    return rc;
  }
  *out = t;
  return 0;
}

static void xl_rs_taps_release(xlating_resample_bank *b, XlRsTaps *t) {
  if (t == nullptr || --t->refs > 0) return;
  b->tables.erase(std::find(b->tables.begin(), b->tables.end(), t));
  if (t->d) (void)hipFree(t->d);
  delete t;
}

// a pinned table of at least `bytes`, free for writing
static int xl_rs_pinned(xlating_resample_bank *b, size_t bytes, XlRsPinned **out) {
  XlRsPinned &t = b->tab[b->tab_i];
  b->tab_i = (b->tab_i + 1) % XL_RS_TABLES;
  if (t.used) XL_RS_TRY(hipEventSynchronize(t.ev));
  if (t.cap < bytes) {
    if (t.h) (void)hipHostFree(t.h);
    t.h = nullptr, t.cap = 0;
    const size_t cap = std::max<size_t>(bytes * 2, 1u << 16);
    XL_RS_TRY(hipHostMalloc(&t.h, cap, hipHostMallocDefault));
    t.cap = cap;
  }
  *out = &t;
  return 0;
}

static int xl_rs_feed(xlating_resample_bank *b, size_t n, const int *ids, const void *const *dev_samples, const size_t *counts,
                      hipStream_t st) {
  b->feed_no++;
  for (size_t i = 0; i < n; ++i) {
    if (!xl_rs_live(b, ids[i]) || counts[i] > XL_RS_COUNT_MAX || (counts[i] > 0 && dev_samples[i] == nullptr)) return -EINVAL;
    XlRsStream &s = b->streams[(size_t)ids[i]];
    if (s.mark == b->feed_no) return -EINVAL;  // named twice
    s.mark = b->feed_no;
  }
  // what the feed holds, per stream; the arena it needs
  b->cuts.resize(n);
  b->runs.reserve(n);
  size_t need = 0;
  uint64_t wgs = 0;
  bool any = false, any_carry = false;
  for (size_t i = 0; i < n; ++i) {
    const XlRsStream &s = b->streams[(size_t)ids[i]];
    b->cuts[i] = xl_resample_cut(s.t->L, s.t->M, s.t->Q, s.P, counts[i]);
    if (b->cuts[i].count >= ((uint64_t)1 << 31)) return -ENOMEM;
    need += (size_t)b->cuts[i].count;
    wgs += (b->cuts[i].count + XL_RS_TILE - 1u) / XL_RS_TILE;
    any |= counts[i] > 0, any_carry |= counts[i] > 0 && s.t->Q > 1u;
  }
  if (wgs >= ((uint64_t)1 << 31)) return -ENOMEM;  // (the ragged launch counts its workgroups in 32 bits)
  XL_RS_TRY(hipSetDevice(b->device));
  if (need > b->out_cap) {  // the arena grows, once the feeds that write and the callers that read the present one are through
    if (b->fed) XL_RS_TRY(hipEventSynchronize(b->last));
    if (b->d_out) (void)hipFree(b->d_out);
    b->d_out = nullptr, b->out_cap = 0, b->out_used = 0, b->out_no = 0;
    const size_t cap = std::max<size_t>(need + need / 2, 1024);
    const hipError_t e = hipMalloc(&b->d_out, cap * sizeof(float2));
    if (e != hipSuccess) {
      (void)hipGetLastError();
      XL_LOG_ERR("resampler bank: output arena of %zu samples: %s", cap, hipGetErrorString(e));
      return -ENOMEM;  // (nothing consumed)
    }
    b->out_cap = cap;
  }
  b->launches = b->copies = 0;
  b->out_no = b->feed_no, b->out_used = need;
  b->runs.clear();
  uint32_t W = 0;
  size_t off = 0;
  for (size_t i = 0; i < n; ++i) {
    XlRsStream &s = b->streams[(size_t)ids[i]];
    const XlResampleCut &c = b->cuts[i];
    s.out_no = b->out_no, s.out_off = off, s.out_n = (size_t)c.count;
    if (counts[i] == 0) continue;
    XlRsRun r;
    r.src = static_cast<const float2 *>(dev_samples[i]);
    r.carry = b->d_carry + (size_t)ids[i] * XL_RS_CARRY_SLOT;
    r.table = s.t->d;
    r.out = b->d_out + off;
    r.n0 = (int32_t)c.n_first, r.p0 = c.p_first;
    r.Q = s.t->Q, r.L = s.t->L, r.M = s.t->M;
    r.nout = (uint32_t)c.count, r.wsum = W, r.cnt = (uint32_t)counts[i];
    b->runs.push_back(r);
    W += (uint32_t)((c.count + XL_RS_TILE - 1u) / XL_RS_TILE);
    off += (size_t)c.count;
    s.P += counts[i];
  }
  if (!any) return 0;
  const size_t bytes = b->runs.size() * sizeof(XlRsRun);
  XlRsPinned *t = nullptr;
  int rc = xl_rs_pinned(b, bytes, &t);
  if (rc != 0) return rc == -ENOMEM ? -EIO : rc;  // (samples are consumed: the bank cannot go on)
  if (b->d_tab_cap < bytes) {
    if (b->fed) XL_RS_TRY(hipEventSynchronize(b->last));  // (the previous feed reads the table that is replaced)
    if (b->d_tab) (void)hipFree(b->d_tab);
    b->d_tab = nullptr, b->d_tab_cap = 0;
    if (hipMalloc(&b->d_tab, bytes * 2) != hipSuccess) return -EIO;
    b->d_tab_cap = bytes * 2;
  }
  if (b->fed) XL_RS_TRY(hipStreamWaitEvent(st, b->last, 0));
  memcpy(t->h, b->runs.data(), bytes);
  XL_RS_TRY(hipMemcpyAsync(b->d_tab, t->h, bytes, hipMemcpyHostToDevice, st));
  XL_RS_TRY(hipEventRecord(t->ev, st));
  t->used = true;
  b->copies += 1;
  const XlRsRun *d_runs = static_cast<const XlRsRun *>(b->d_tab);
  if (W > 0) {
    XL_RS_TRY(xl_rs_launch(d_runs, (uint32_t)b->runs.size(), W, st));
    b->launches += 1;
  }
  if (any_carry) {
    XL_RS_TRY(xl_rs_carry(d_runs, (uint32_t)b->runs.size(), st));
    b->launches += 1;
  }
  XL_RS_TRY(hipEventRecord(b->last, st));
  b->fed = true;
  return 0;
}

// ---------------------------------------------------------------------------------------------------------- C API
extern "C" int xlating_resample_bank_create(xlating_resample_bank **out) {
  if (out == nullptr) return -EINVAL;
  *out = nullptr;
  const int device = xl_hip_select_device(-1);
  if (device < 0) {
    XL_LOG_ERR("xlating_resample_bank_create: no usable HIP device (%s); there is no CPU path", xlating_hip_device_info());
    return -ENODEV;
  }
  xlating_resample_bank *b = new (std::nothrow) xlating_resample_bank();
  if (b == nullptr) return -ENOMEM;
  b->device = device;
  hipError_t e = hipSetDevice(device);
  if (e == hipSuccess) e = hipStreamCreateWithFlags(&b->own, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&b->last, hipEventDisableTiming);
  for (int i = 0; i < XL_RS_TABLES && e == hipSuccess; ++i) e = hipEventCreateWithFlags(&b->tab[i].ev, hipEventDisableTiming);
  if (e != hipSuccess) {
    xl_last_hip_error = e;
    XL_LOG_ERR("xlating_resample_bank_create: %s", hipGetErrorString(e));
    const int rc = xl_errno_of_last_hip_error();
    xlating_resample_bank_destroy(b);
    return rc;
  }
  *out = b;
  return 0;
}

extern "C" int xlating_resample_bank_add(xlating_resample_bank *b, uint32_t L, uint32_t M, const float *taps, size_t taps_len) {
  if (b == nullptr || L == 0u || M == 0u || L > XLATING_RESAMPLE_MAX_L || M >= (1u << 31) || taps == nullptr || taps_len == 0 ||
      (taps_len + L - 1u) / L > XLATING_RESAMPLE_MAX_Q || xl_rs_gcd(L, M) != 1u)
    return -EINVAL;
  if (b->broken) return -EIO;
  try {
    const bool reuse = !b->free_ids.empty();
    const size_t id = reuse ? (size_t)b->free_ids.back() : b->streams.size();
    if (id >= XL_RS_MAX_STREAMS) return -ENOMEM;
    XL_RS_TRY(hipSetDevice(b->device));
    int rc = xl_rs_reserve_streams(b, (uint32_t)id + 1u);
    if (rc != 0) return rc;
    XlRsTaps *t = nullptr;
    if ((rc = xl_rs_taps(b, L, M, taps, taps_len, &t)) != 0) return rc;
    if (reuse)
      b->free_ids.pop_back();
    else
      b->streams.emplace_back();
    t->refs++;
    XlRsStream &s = b->streams[id];
    s.live = true, s.t = t, s.P = 0, s.out_no = 0, s.out_off = 0, s.out_n = 0;
    b->nlive++;
    return (int)id;
  } catch (const std::bad_alloc &) {
    return -ENOMEM;
  }
}

extern "C" int xlating_resample_bank_remove(xlating_resample_bank *b, int stream_id) {
  if (!xl_rs_live(b, stream_id)) return -EINVAL;
  XlRsStream &s = b->streams[(size_t)stream_id];
  if (!b->broken) XL_RS_TRY(hipSetDevice(b->device));
  if (s.P > 0 && !b->broken) {  // the id's next use starts from zero history
    if (b->fed) XL_RS_TRY(hipEventSynchronize(b->last));
    XL_RS_TRY(hipMemsetAsync(b->d_carry + (size_t)stream_id * XL_RS_CARRY_SLOT, 0, XL_RS_CARRY_SLOT * sizeof(float2), b->own));
    XL_RS_TRY(hipStreamSynchronize(b->own));
  }  // (a stream that consumed nothing was in no launch: its table, if it is the last user, is read by nothing)
  xl_rs_taps_release(b, s.t);
  s.live = false, s.t = nullptr, s.out_n = 0;
  b->nlive--;
  try {
    b->free_ids.push_back(stream_id);
  } catch (const std::bad_alloc &) {  // (the id is then not reused)
  }
  return 0;
}

extern "C" int xlating_resample_bank_feed_device(xlating_resample_bank *b, size_t n, const int *ids, const void *const *dev_samples,
                                                 const size_t *counts, void *hip_stream) {
  if (b == nullptr || (n > 0 && (ids == nullptr || dev_samples == nullptr || counts == nullptr))) return -EINVAL;
  if (b->broken) return -EIO;
  int rc;
  try {
    rc = xl_rs_feed(b, n, ids, dev_samples, counts, static_cast<hipStream_t>(hip_stream));
  } catch (const std::bad_alloc &) {  // (the feed's vectors are sized before anything is consumed)
    rc = -ENOMEM;
  }
  if (rc != 0 && rc != -EINVAL && rc != -ENOMEM) b->broken = true;  // (-EINVAL and -ENOMEM are decided before anything is consumed)
  return rc;
}

extern "C" int xlating_resample_bank_output_device(xlating_resample_bank *b, int stream_id, const void **d_out, size_t *n_complex) {
  if (!xl_rs_live(b, stream_id) || d_out == nullptr || n_complex == nullptr) return -EINVAL;
  if (b->broken) return -EIO;
  const XlRsStream &s = b->streams[(size_t)stream_id];
  const bool have = s.out_no == b->out_no && b->out_no != 0 && s.out_n > 0;
  *d_out = have ? b->d_out + s.out_off : nullptr;
  *n_complex = have ? s.out_n : 0;
  return 0;
}

extern "C" int xlating_resample_bank_fetch(xlating_resample_bank *b) {
  if (b == nullptr) return -EINVAL;
  if (b->broken) return -EIO;
  XL_RS_TRY(hipSetDevice(b->device));
  if (b->fed) XL_RS_TRY(hipEventSynchronize(b->last));
  if (b->out_used > b->h_cap) {
    if (b->h_out) (void)hipHostFree(b->h_out);
    b->h_out = nullptr, b->h_cap = 0;
    const size_t cap = std::max<size_t>(b->out_used + b->out_used / 2, 1u << 16);
    XL_RS_TRY(hipHostMalloc(reinterpret_cast<void **>(&b->h_out), cap * sizeof(float2), hipHostMallocDefault));
    b->h_cap = cap;
  }
  if (b->out_used > 0) {
    XL_RS_TRY(hipMemcpyAsync(b->h_out, b->d_out, b->out_used * sizeof(float2), hipMemcpyDeviceToHost, b->own));
    XL_RS_TRY(hipStreamSynchronize(b->own));
  }
  b->h_no = b->out_no;
  return 0;
}

extern "C" int xlating_resample_bank_output_host(xlating_resample_bank *b, int stream_id, const float **out, size_t *n_complex) {
  if (!xl_rs_live(b, stream_id) || out == nullptr || n_complex == nullptr) return -EINVAL;
  const XlRsStream &s = b->streams[(size_t)stream_id];
  const bool have = b->h_no != 0 && s.out_no == b->h_no && s.out_n > 0 && b->h_out != nullptr;
  *out = have ? reinterpret_cast<const float *>(b->h_out + s.out_off) : nullptr;
  *n_complex = have ? s.out_n : 0;
  return 0;
}

extern "C" uint64_t xlating_resample_bank_produced(const xlating_resample_bank *b, int stream_id) {
  if (!xl_rs_live(b, stream_id)) return 0;
  const XlRsStream &s = b->streams[(size_t)stream_id];
  return xl_resample_produced(s.t->L, s.t->M, s.P);
}

extern "C" int xlating_resample_bank_last_feed_ops(const xlating_resample_bank *b, unsigned *launches, unsigned *copies) {
  if (b == nullptr) return -EINVAL;
  if (launches) *launches = b->launches;
  if (copies) *copies = b->copies;
  return 0;
}

extern "C" int xlating_resample_bank_stats(const xlating_resample_bank *b, unsigned *streams, unsigned *tables, size_t *table_bytes) {
  if (b == nullptr) return -EINVAL;
  size_t bytes = 0;
  for (const XlRsTaps *t : b->tables) bytes += t->bytes;
  if (streams) *streams = b->nlive;
  if (tables) *tables = (unsigned)b->tables.size();
  if (table_bytes) *table_bytes = bytes;
  return 0;
}

extern "C" void xlating_resample_bank_destroy(xlating_resample_bank *b) {
  if (b == nullptr) return;
  (void)hipSetDevice(b->device);
  if (b->fed) (void)hipEventSynchronize(b->last);
  if (b->own) (void)hipStreamSynchronize(b->own);
  for (XlRsTaps *t : b->tables) {
    if (t->d) (void)hipFree(t->d);
    delete t;
  }
  for (XlRsPinned &t : b->tab) {
    if (t.h) (void)hipHostFree(t.h);
    if (t.ev) (void)hipEventDestroy(t.ev);
  }
  if (b->d_tab) (void)hipFree(b->d_tab);
  if (b->d_out) (void)hipFree(b->d_out);
  if (b->h_out) (void)hipHostFree(b->h_out);
  if (b->d_carry) (void)hipFree(b->d_carry);
  if (b->last) (void)hipEventDestroy(b->last);
  if (b->own) (void)hipStreamDestroy(b->own);
  delete b;
}
