// xl_resample.cpp -- the resampler banks (include/xlating_resample.h, include/xlating_resample_q15.h): many independent complex
// streams, each resampled by its own rational factor, advanced by one feed of two launches and one table copy.  ONE implementation
// for both families: a bank is float32 (8-byte samples, float taps, kernels xl_resample.hip) or Q15 (4-byte int16 pairs, int16 taps,
// kernels xl_resample_q15.hip) from its creation on, and differs in the sample size, the table's element and the pair of launches
// (XlRsF32 / XlRsQ15 below); the entry points of both headers are thin.  What a feed of n samples holds for a stream:
// xl_resample_cut.h; the Q15 taps: xl_resample_q15_quant.h.
//
// Device state: per stream id a carry slot of XL_RS_CARRY_SLOT samples (the last Q - 1 inputs; zero for a new stream), in one array
// that grows as streams are added; per distinct (L, M, taps) one phase-major tap table, reference-counted; one output arena, carved per
// feed from the host-computed output counts, which holds the latest feed's outputs and grows (after a wait) when a feed needs more.
// One feed = one table of runs written into pinned memory and uploaded by one copy, the ragged resampling launch, the carry launch.
// The ring of pinned tables, the single device table and the growth of the carry array, with the rules of their lifetimes, are
// xl_bank_host.h's (shared with the spectrum bank); a feed does not wait for the previous one.
#include "../../include/xlating_resample.h"
#include "../../include/xlating_resample_q15.h"

#include <errno.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <new>
#include <vector>

#include "xl_bank_host.h"
#include "xl_common.h"
#include "xl_resample.h"
#include "xl_resample_cut.h"
#include "xl_resample_q15.h"
#include "xl_resample_q15_quant.h"

#define XL_RS_MAX_STREAMS 65536
#define XL_RS_COUNT_MAX ((size_t)1 << 30)

namespace {

struct XlRsTaps {  // one device tap table and the streams' common definition
  uint32_t L = 0, M = 0, Q = 0;
  std::vector<float> taps;
  void *d = nullptr;   // [L][Q]: float, or int16 (the quantised taps)
  size_t bytes = 0;
  bool wide = false;   // Q15: some phase has sum |c| > 65535, the sums need 64 bits
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

}  // namespace

struct xlating_resample_bank {
  int device = 0;
  hipStream_t own = nullptr;  // growth and clearing of the per-stream state, the fetch
  hipEvent_t last = nullptr;  // behind the latest feed's work
  bool q15 = false;           // the family: which header's functions take this handle
  size_t esz = sizeof(float2);  // bytes per complex sample
  uint32_t exp_flags = 0;       // Q15, measurement knob XL_EXP_RSQ: run flags forced on every run (XL_RSQ_WIDE, XL_RSQ_TAPS_IN_PLACE)
  bool fed = false, broken = false;
  uint32_t cap_streams = 0;
  void *d_carry = nullptr;  // [cap_streams][XL_RS_CARRY_SLOT] samples
  std::vector<XlRsStream> streams;
  std::vector<int> free_ids;
  unsigned nlive = 0;
  std::vector<XlRsTaps *> tables;
  uint64_t feed_no = 0;
  XlTableRing ring;  // the feeds' tables of runs
  char *d_out = nullptr;  // the arena (samples)
  size_t out_cap = 0, out_used = 0;
  uint64_t out_no = 0;      // generation: the feed whose outputs the arena holds
  char *h_out = nullptr;  // the fetched copy
  size_t h_cap = 0;
  uint64_t h_no = 0;
  unsigned launches = 0, copies = 0;
  std::vector<XlResampleCut> cuts;
};

namespace {

// the two families: the run a launch reads, and the launches
struct XlRsF32 {
  typedef XlRsRun Run;
  typedef float2 Sample;
  typedef float Tap;
  static void flags(Run &, const XlRsTaps &, uint32_t) {}
  static int launch(const Run *runs, uint32_t nruns, uint32_t W, hipStream_t st) { return xl_rs_launch(runs, nruns, W, st); }
  static int carry(const Run *runs, uint32_t nruns, hipStream_t st) { return xl_rs_carry(runs, nruns, st); }
};

struct XlRsQ15 {
  typedef XlRsQ15Run Run;
  typedef xl_cs16 Sample;
  typedef int16_t Tap;
  static void flags(Run &r, const XlRsTaps &t, uint32_t forced) { r.flags = (t.wide ? XL_RSQ_WIDE : 0u) | forced, r.pad_ = 0u; }
  static int launch(const Run *runs, uint32_t nruns, uint32_t W, hipStream_t st) { return xl_rsq_launch(runs, nruns, W, st); }
  static int carry(const Run *runs, uint32_t nruns, hipStream_t st) { return xl_rsq_carry(runs, nruns, st); }
};

}  // namespace

// a handle of the family the called function belongs to
static bool xl_rs_is(const xlating_resample_bank *b, bool q15) { return b != nullptr && b->q15 == q15; }

static bool xl_rs_live(const xlating_resample_bank *b, bool q15, int id) {
  return xl_rs_is(b, q15) && id >= 0 && (size_t)id < b->streams.size() && b->streams[(size_t)id].live;
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
  if (b->fed) XL_TRY_RET(hipEventSynchronize(b->last));
  const XlStreamArray a[] = {{&b->d_carry, (size_t)XL_RS_CARRY_SLOT * b->esz, true}};
  return xl_streams_grow(&b->cap_streams, need, a, b->own, "resampler bank: carries");
}

// [p][q] = v[p + q L], zero beyond len; `pad` more zero elements behind it
template <typename T>
static std::vector<T> xl_rs_phase_major(uint32_t L, uint32_t Q, const T *v, size_t len, size_t pad) {
  std::vector<T> pm((size_t)L * Q + pad, (T)0);
  for (size_t i = 0; i < len; ++i) pm[(i % L) * Q + i / L] = v[i];
  return pm;
}

// the table of (L, M, taps): the one that exists, or a new one uploaded phase-major -- of the float taps, or, in a Q15 bank, of
// their quantised values c[0 .. len)
static int xl_rs_taps(xlating_resample_bank *b, uint32_t L, uint32_t M, const float *taps, size_t len, const int16_t *c,
                      XlRsTaps **out) {
  for (XlRsTaps *t : b->tables)
    if (t->L == L && t->M == M && t->taps.size() == len && memcmp(t->taps.data(), taps, len * sizeof(float)) == 0) {
      *out = t;
      return 0;
    }
  XlRsTaps *t = new XlRsTaps();
  t->L = L, t->M = M, t->Q = (uint32_t)((len + L - 1u) / L);
  t->bytes = (size_t)L * t->Q * (c ? sizeof(int16_t) : sizeof(float));
  int rc = 0;
  try {
    t->taps.assign(taps, taps + len);
    const std::vector<float> pf = c ? std::vector<float>() : xl_rs_phase_major(L, t->Q, taps, len, 0);
    const std::vector<int16_t> pq = c ? xl_rs_phase_major(L, t->Q, c, len, 1) : std::vector<int16_t>();  // (read as whole words)
    for (size_t p = 0; c && p < L; ++p) {
      uint32_t sum = 0;  // <= 1024 * 32768
      for (uint32_t q = 0; q < t->Q; ++q) sum += (uint32_t)abs((int)pq[p * t->Q + q]);
      t->wide |= sum > 65535u;
    }
    const void *src = c ? static_cast<const void *>(pq.data()) : static_cast<const void *>(pf.data());
    const size_t up = c ? (t->bytes + 3u) / 4u * 4u : t->bytes;
    hipError_t e = hipMalloc(&t->d, up);
    if (e == hipSuccess) e = hipMemcpy(t->d, src, up, hipMemcpyHostToDevice);
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

template <class K>
static int xl_rs_feed(xlating_resample_bank *b, size_t n, const int *ids, const void *const *dev_samples, const size_t *counts,
                      hipStream_t st) {
  typedef typename K::Run Run;
  typedef typename K::Sample Sample;
  b->feed_no++;
  for (size_t i = 0; i < n; ++i) {
    if (!xl_rs_live(b, b->q15, ids[i]) || counts[i] > XL_RS_COUNT_MAX || (counts[i] > 0 && dev_samples[i] == nullptr)) return -EINVAL;
    XlRsStream &s = b->streams[(size_t)ids[i]];
    if (s.mark == b->feed_no) return -EINVAL;  // named twice
    s.mark = b->feed_no;
  }
  // what the feed holds, per stream; the arena it needs
  b->cuts.resize(n);
  size_t need = 0, nruns = 0;
  uint64_t wgs = 0;
  bool any_carry = false;
  for (size_t i = 0; i < n; ++i) {
    const XlRsStream &s = b->streams[(size_t)ids[i]];
    b->cuts[i] = xl_resample_cut(s.t->L, s.t->M, s.t->Q, s.P, counts[i]);
    if (b->cuts[i].count >= ((uint64_t)1 << 31)) return -ENOMEM;
    need += (size_t)b->cuts[i].count;
    wgs += (b->cuts[i].count + XL_RS_TILE - 1u) / XL_RS_TILE;
    nruns += counts[i] > 0, any_carry |= counts[i] > 0 && s.t->Q > 1u;
  }
  if (wgs >= ((uint64_t)1 << 31)) return -ENOMEM;  // (the ragged launch counts its workgroups in 32 bits)
  XL_TRY_RET(hipSetDevice(b->device));
  if (need > b->out_cap) {  // the arena grows, once the feeds that write and the callers that read the present one are through
    if (b->fed) XL_TRY_RET(hipEventSynchronize(b->last));
    if (b->d_out) (void)hipFree(b->d_out);
    b->d_out = nullptr, b->out_cap = 0, b->out_used = 0, b->out_no = 0;
    const size_t cap = std::max<size_t>(need + need / 2, 1024);
    const hipError_t e = hipMalloc(&b->d_out, cap * sizeof(Sample));
    if (e != hipSuccess) {
      (void)hipGetLastError();
      XL_LOG_ERR("resampler bank: output arena of %zu samples: %s", cap, hipGetErrorString(e));
      return -ENOMEM;  // (nothing consumed)
    }
    b->out_cap = cap;
  }
  // the table of runs: written in pinned memory, one run per stream that consumes anything
  const size_t bytes = nruns * sizeof(Run);
  XlRingTable *t = nullptr;
  if (nruns > 0) {
    XL_TRY_RET(xl_ring_acquire(&b->ring, bytes, &t));  // (-ENOMEM: nothing consumed)
    if (b->ring.d_cap < bytes) {
      if (b->fed) XL_TRY_RET(hipEventSynchronize(b->last));  // (the previous feed reads the table that is replaced)
      // (an oddity kept as it is: -EIO whatever the error, the bank broken, and xl_last_hip_error not set)
      if (xl_ring_dev_grow(&b->ring, bytes) != hipSuccess) return -EIO;
    }
  }
  b->launches = b->copies = 0;
  b->out_no = b->feed_no, b->out_used = need;
  Run *runs = nruns > 0 ? static_cast<Run *>(t->h) : nullptr;
  Sample *const d_out = reinterpret_cast<Sample *>(b->d_out), *const d_carry = static_cast<Sample *>(b->d_carry);
  uint32_t W = 0;
  size_t off = 0, k = 0;
  for (size_t i = 0; i < n; ++i) {
    XlRsStream &s = b->streams[(size_t)ids[i]];
    const XlResampleCut &c = b->cuts[i];
    s.out_no = b->out_no, s.out_off = off, s.out_n = (size_t)c.count;
    if (counts[i] == 0) continue;
    Run &r = runs[k++];
    r.src = static_cast<const Sample *>(dev_samples[i]);
    r.carry = d_carry + (size_t)ids[i] * XL_RS_CARRY_SLOT;
    r.table = static_cast<const typename K::Tap *>(s.t->d);
    r.out = d_out + off;
    r.n0 = (int32_t)c.n_first, r.p0 = c.p_first;
    r.Q = s.t->Q, r.L = s.t->L, r.M = s.t->M;
    r.nout = (uint32_t)c.count, r.wsum = W, r.cnt = (uint32_t)counts[i];
    K::flags(r, *s.t, b->exp_flags);
    W += (uint32_t)((c.count + XL_RS_TILE - 1u) / XL_RS_TILE);
    off += (size_t)c.count;
    s.P += counts[i];
  }
  if (nruns == 0) return 0;
  if (b->fed) XL_TRY_RET(hipStreamWaitEvent(st, b->last, 0));
  XL_TRY_RET(xl_ring_upload(&b->ring, t, bytes, st));
  b->copies += 1;
  const Run *d_runs = static_cast<const Run *>(b->ring.d_tab);
  if (W > 0) {
    XL_TRY_RET(K::launch(d_runs, (uint32_t)nruns, W, st));
    b->launches += 1;
  }
  if (any_carry) {
    XL_TRY_RET(K::carry(d_runs, (uint32_t)nruns, st));
    b->launches += 1;
  }
  XL_TRY_RET(hipEventRecord(b->last, st));
  b->fed = true;
  return 0;
}

// ------------------------------------------------------------------------------------- the banks' functions, for either family
static void xl_rs_destroy(xlating_resample_bank *b);

static int xl_rs_create(bool q15, const char *who, xlating_resample_bank **out) {
  if (out == nullptr) return -EINVAL;
  *out = nullptr;
  const int device = xl_hip_select_device(-1);
  if (device < 0) {
    XL_LOG_ERR("%s: no usable HIP device (%s); there is no CPU path", who, xlating_hip_device_info());
    return -ENODEV;
  }
  xlating_resample_bank *b = new (std::nothrow) xlating_resample_bank();
  if (b == nullptr) return -ENOMEM;
  b->device = device;
  b->q15 = q15, b->esz = q15 ? sizeof(xl_cs16) : sizeof(float2);
  if (const char *e = xl_exp_getenv("XL_EXP_RSQ"))  // what the 32-bit sums and the LDS tap table buy (tools/resample_bank_bench.py)
    b->exp_flags = q15 ? (uint32_t)atoi(e) & (XL_RSQ_WIDE | XL_RSQ_TAPS_IN_PLACE) : 0u;
  hipError_t e = hipSetDevice(device);
  if (e == hipSuccess) e = hipStreamCreateWithFlags(&b->own, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&b->last, hipEventDisableTiming);
  if (e == hipSuccess) e = xl_ring_init(&b->ring);
  if (e != hipSuccess) {
    xl_last_hip_error = e;
    XL_LOG_ERR("%s: %s", who, hipGetErrorString(e));
    const int rc = xl_errno_of_last_hip_error();
    xl_rs_destroy(b);
    return rc;
  }
  *out = b;
  return 0;
}

// the arguments have been checked; c: the quantised taps of a Q15 bank
static int xl_rs_add(xlating_resample_bank *b, uint32_t L, uint32_t M, const float *taps, size_t taps_len, const int16_t *c) {
  if (b->broken) return -EIO;
  try {
    const bool reuse = !b->free_ids.empty();
    const size_t id = reuse ? (size_t)b->free_ids.back() : b->streams.size();
    if (id >= XL_RS_MAX_STREAMS) return -ENOMEM;
    XL_TRY_RET(hipSetDevice(b->device));
    int rc = xl_rs_reserve_streams(b, (uint32_t)id + 1u);
    if (rc != 0) return rc;
    XlRsTaps *t = nullptr;
    if ((rc = xl_rs_taps(b, L, M, taps, taps_len, c, &t)) != 0) return rc;
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

static int xl_rs_remove(xlating_resample_bank *b, bool q15, int stream_id) {
  if (!xl_rs_live(b, q15, stream_id)) return -EINVAL;
  XlRsStream &s = b->streams[(size_t)stream_id];
  if (!b->broken) XL_TRY_RET(hipSetDevice(b->device));
  if (s.P > 0 && !b->broken) {  // the id's next use starts from zero history
    const size_t slot = (size_t)XL_RS_CARRY_SLOT * b->esz;
    if (b->fed) XL_TRY_RET(hipEventSynchronize(b->last));
    XL_TRY_RET(hipMemsetAsync(static_cast<char *>(b->d_carry) + (size_t)stream_id * slot, 0, slot, b->own));
    XL_TRY_RET(hipStreamSynchronize(b->own));
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

static int xl_rs_feed_device(xlating_resample_bank *b, bool q15, size_t n, const int *ids, const void *const *dev_samples,
                             const size_t *counts, void *hip_stream) {
  if (!xl_rs_is(b, q15) || (n > 0 && (ids == nullptr || dev_samples == nullptr || counts == nullptr))) return -EINVAL;
  if (b->broken) return -EIO;
  const hipStream_t st = static_cast<hipStream_t>(hip_stream);
  int rc;
  try {
    rc = q15 ? xl_rs_feed<XlRsQ15>(b, n, ids, dev_samples, counts, st) : xl_rs_feed<XlRsF32>(b, n, ids, dev_samples, counts, st);
  } catch (const std::bad_alloc &) {  // (the feed's vectors are sized before anything is consumed)
    rc = -ENOMEM;
  }
  if (rc != 0 && rc != -EINVAL && rc != -ENOMEM) b->broken = true;  // (-EINVAL and -ENOMEM are decided before anything is consumed)
  return rc;
}

static int xl_rs_output_device(xlating_resample_bank *b, bool q15, int stream_id, const void **d_out, size_t *n_complex) {
  if (!xl_rs_live(b, q15, stream_id) || d_out == nullptr || n_complex == nullptr) return -EINVAL;
  if (b->broken) return -EIO;
  const XlRsStream &s = b->streams[(size_t)stream_id];
  const bool have = s.out_no == b->out_no && b->out_no != 0 && s.out_n > 0;
  *d_out = have ? b->d_out + s.out_off * b->esz : nullptr;
  *n_complex = have ? s.out_n : 0;
  return 0;
}

static int xl_rs_fetch(xlating_resample_bank *b, bool q15) {
  if (!xl_rs_is(b, q15)) return -EINVAL;
  if (b->broken) return -EIO;
  XL_TRY_RET(hipSetDevice(b->device));
  if (b->fed) XL_TRY_RET(hipEventSynchronize(b->last));
  if (b->out_used > b->h_cap) {
    if (b->h_out) (void)hipHostFree(b->h_out);
    b->h_out = nullptr, b->h_cap = 0;
    const size_t cap = std::max<size_t>(b->out_used + b->out_used / 2, 1u << 16);
    XL_TRY_RET(hipHostMalloc(reinterpret_cast<void **>(&b->h_out), cap * b->esz, hipHostMallocDefault));
    b->h_cap = cap;
  }
  if (b->out_used > 0) {
    XL_TRY_RET(hipMemcpyAsync(b->h_out, b->d_out, b->out_used * b->esz, hipMemcpyDeviceToHost, b->own));
    XL_TRY_RET(hipStreamSynchronize(b->own));
  }
  b->h_no = b->out_no;
  return 0;
}

static int xl_rs_output_host(xlating_resample_bank *b, bool q15, int stream_id, const void **out, size_t *n_complex) {
  if (!xl_rs_live(b, q15, stream_id) || out == nullptr || n_complex == nullptr) return -EINVAL;
  const XlRsStream &s = b->streams[(size_t)stream_id];
  const bool have = b->h_no != 0 && s.out_no == b->h_no && s.out_n > 0 && b->h_out != nullptr;
  *out = have ? b->h_out + s.out_off * b->esz : nullptr;
  *n_complex = have ? s.out_n : 0;
  return 0;
}

static uint64_t xl_rs_produced(const xlating_resample_bank *b, bool q15, int stream_id) {
  if (!xl_rs_live(b, q15, stream_id)) return 0;
  const XlRsStream &s = b->streams[(size_t)stream_id];
  return xl_resample_produced(s.t->L, s.t->M, s.P);
}

static int xl_rs_last_feed_ops(const xlating_resample_bank *b, bool q15, unsigned *launches, unsigned *copies) {
  if (!xl_rs_is(b, q15)) return -EINVAL;
  if (launches) *launches = b->launches;
  if (copies) *copies = b->copies;
  return 0;
}

static int xl_rs_stats(const xlating_resample_bank *b, bool q15, unsigned *streams, unsigned *tables, size_t *table_bytes) {
  if (!xl_rs_is(b, q15)) return -EINVAL;
  size_t bytes = 0;
  for (const XlRsTaps *t : b->tables) bytes += t->bytes;
  if (streams) *streams = b->nlive;
  if (tables) *tables = (unsigned)b->tables.size();
  if (table_bytes) *table_bytes = bytes;
  return 0;
}

static void xl_rs_destroy(xlating_resample_bank *b) {
  if (b == nullptr) return;
  (void)hipSetDevice(b->device);
  if (b->fed) (void)hipEventSynchronize(b->last);
  if (b->own) (void)hipStreamSynchronize(b->own);
  for (XlRsTaps *t : b->tables) {
    if (t->d) (void)hipFree(t->d);
    delete t;
  }
  xl_ring_destroy(&b->ring);
  if (b->d_out) (void)hipFree(b->d_out);
  if (b->h_out) (void)hipHostFree(b->h_out);
  if (b->d_carry) (void)hipFree(b->d_carry);
  if (b->last) (void)hipEventDestroy(b->last);
  if (b->own) (void)hipStreamDestroy(b->own);
  delete b;
}

// ---------------------------------------------------------------------------------------------------------- C API: float32
extern "C" int xlating_resample_bank_create(xlating_resample_bank **out) {
  return xl_rs_create(false, "xlating_resample_bank_create", out);
}

extern "C" int xlating_resample_bank_add(xlating_resample_bank *b, uint32_t L, uint32_t M, const float *taps, size_t taps_len) {
  if (b == nullptr || L == 0u || M == 0u || L > XLATING_RESAMPLE_MAX_L || M >= (1u << 31) || taps == nullptr || taps_len == 0 ||
      (taps_len + L - 1u) / L > XLATING_RESAMPLE_MAX_Q || xl_rs_gcd(L, M) != 1u)
    return -EINVAL;
  if (b->q15) return -EINVAL;  // (a Q15 bank's handle)
  return xl_rs_add(b, L, M, taps, taps_len, nullptr);  // (whose hipSetDevice is the first the device hears of the stream)
}

extern "C" int xlating_resample_bank_remove(xlating_resample_bank *b, int stream_id) { return xl_rs_remove(b, false, stream_id); }

extern "C" int xlating_resample_bank_feed_device(xlating_resample_bank *b, size_t n, const int *ids, const void *const *dev_samples,
                                                 const size_t *counts, void *hip_stream) {
  return xl_rs_feed_device(b, false, n, ids, dev_samples, counts, hip_stream);
}

extern "C" int xlating_resample_bank_output_device(xlating_resample_bank *b, int stream_id, const void **d_out, size_t *n_complex) {
  return xl_rs_output_device(b, false, stream_id, d_out, n_complex);
}

extern "C" int xlating_resample_bank_fetch(xlating_resample_bank *b) { return xl_rs_fetch(b, false); }

extern "C" int xlating_resample_bank_output_host(xlating_resample_bank *b, int stream_id, const float **out, size_t *n_complex) {
  const void *p = nullptr;
  const int rc = xl_rs_output_host(b, false, stream_id, out ? &p : nullptr, n_complex);
  if (rc == 0) *out = static_cast<const float *>(p);
  return rc;
}

extern "C" uint64_t xlating_resample_bank_produced(const xlating_resample_bank *b, int stream_id) {
  return xl_rs_produced(b, false, stream_id);
}

extern "C" int xlating_resample_bank_last_feed_ops(const xlating_resample_bank *b, unsigned *launches, unsigned *copies) {
  return xl_rs_last_feed_ops(b, false, launches, copies);
}

extern "C" int xlating_resample_bank_stats(const xlating_resample_bank *b, unsigned *streams, unsigned *tables, size_t *table_bytes) {
  return xl_rs_stats(b, false, streams, tables, table_bytes);
}

extern "C" void xlating_resample_bank_destroy(xlating_resample_bank *b) {
  if (xl_rs_is(b, false)) xl_rs_destroy(b);
}

// ---------------------------------------------------------------------------------------------------------- C API: Q15
// (a xlating_resample_q15_bank is the same object, created as the other family)
static xlating_resample_bank *xl_rs_q(xlating_resample_q15_bank *b) { return reinterpret_cast<xlating_resample_bank *>(b); }
static const xlating_resample_bank *xl_rs_q(const xlating_resample_q15_bank *b) {
  return reinterpret_cast<const xlating_resample_bank *>(b);
}

extern "C" int xlating_resample_q15_quantize(const float *taps, size_t len, int16_t *out) {
  return xl_resample_q15_quantize(taps, len, out);
}

extern "C" int xlating_resample_q15_bank_create(xlating_resample_q15_bank **out) {
  return xl_rs_create(true, "xlating_resample_q15_bank_create", reinterpret_cast<xlating_resample_bank **>(out));
}

extern "C" int xlating_resample_q15_bank_add(xlating_resample_q15_bank *q, uint32_t L, uint32_t M, const float *taps, size_t taps_len) {
  xlating_resample_bank *b = xl_rs_q(q);
  if (b == nullptr || L == 0u || M == 0u || L > XLATING_RESAMPLE_MAX_L || M >= (1u << 31) || taps == nullptr || taps_len == 0 ||
      (taps_len + L - 1u) / L > XLATING_RESAMPLE_MAX_Q || xl_rs_gcd(L, M) != 1u || !b->q15)
    return -EINVAL;
  try {
    std::vector<int16_t> c(taps_len);
    const int rc = xl_resample_q15_quantize(taps, taps_len, c.data());
    if (rc != 0) return rc;  // -ERANGE
    return xl_rs_add(b, L, M, taps, taps_len, c.data());
  } catch (const std::bad_alloc &) {
    return -ENOMEM;
  }
}

extern "C" int xlating_resample_q15_bank_remove(xlating_resample_q15_bank *b, int stream_id) {
  return xl_rs_remove(xl_rs_q(b), true, stream_id);
}

extern "C" int xlating_resample_q15_bank_feed_device(xlating_resample_q15_bank *b, size_t n, const int *ids,
                                                     const void *const *dev_samples, const size_t *counts, void *hip_stream) {
  return xl_rs_feed_device(xl_rs_q(b), true, n, ids, dev_samples, counts, hip_stream);
}

extern "C" int xlating_resample_q15_bank_output_device(xlating_resample_q15_bank *b, int stream_id, const void **d_out,
                                                       size_t *n_complex) {
  return xl_rs_output_device(xl_rs_q(b), true, stream_id, d_out, n_complex);
}

extern "C" int xlating_resample_q15_bank_fetch(xlating_resample_q15_bank *b) { return xl_rs_fetch(xl_rs_q(b), true); }

extern "C" int xlating_resample_q15_bank_output_host(xlating_resample_q15_bank *b, int stream_id, const int16_t **out,
                                                     size_t *n_complex) {
  const void *p = nullptr;
  const int rc = xl_rs_output_host(xl_rs_q(b), true, stream_id, out ? &p : nullptr, n_complex);
  if (rc == 0) *out = static_cast<const int16_t *>(p);
  return rc;
}

extern "C" uint64_t xlating_resample_q15_bank_produced(const xlating_resample_q15_bank *b, int stream_id) {
  return xl_rs_produced(xl_rs_q(b), true, stream_id);
}

extern "C" int xlating_resample_q15_bank_last_feed_ops(const xlating_resample_q15_bank *b, unsigned *launches, unsigned *copies) {
  return xl_rs_last_feed_ops(xl_rs_q(b), true, launches, copies);
}

extern "C" int xlating_resample_q15_bank_stats(const xlating_resample_q15_bank *b, unsigned *streams, unsigned *tables,
                                               size_t *table_bytes) {
  return xl_rs_stats(xl_rs_q(b), true, streams, tables, table_bytes);
}

extern "C" void xlating_resample_q15_bank_destroy(xlating_resample_q15_bank *b) {
  if (xl_rs_is(xl_rs_q(b), true)) xl_rs_destroy(xl_rs_q(b));
}
