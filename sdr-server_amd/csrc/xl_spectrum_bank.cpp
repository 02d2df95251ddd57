// xl_spectrum_bank.cpp -- the spectrum bank (include/xlating_spectrum.h, xlating_spectrum_bank_*): many independent streams of one
// width and format, advanced by one feed whose launches and copies do not depend on how many streams it carries.  Kernels:
// xl_spectrum_bank.hip; the cutting of a stream's samples into transforms: xl_spectrum_cut.h.
//
// Device state, per stream id: W samples of carry (the transform that straddles two feeds) and `slots` row slots of W maxima
// (row % slots; float bits, zero between rows).  Both arrays grow as streams are added.  A stream between feeds has at most one row in
// progress; a feed that would run a stream through more rows than it has slots is cut into ROUNDS (xl_spec_round_limit).
// One round = one table (runs of the ragged launch, carry operations, the list of completed rows) written into pinned memory and
// uploaded by one copy, then: the carry appends, the ragged transform launch, the carry saves, and -- when the round completes rows --
// the finishing launch and one pair of copies (dB, pixels) into a pinned batch.  Launches that have nothing to do are left out.
// The ring of pinned tables, the single device table and the growth of the per-stream arrays, with the rules of their lifetimes, are
// xl_bank_host.h's (shared with the resampler banks); a feed does not wait for the previous one.
// A bank of xlating_spectrum_bank_create_wide with a width above 8192 differs in four places: the ragged transform launch becomes the
// two-level transform's passes (xl_spectrum_bank_wide.hip), a chunk of the round's transform list at a time through one scratch buffer
// (stream order keeps one chunk's passes and the next chunk's apart); the carries are copied on a grid over pieces; the finishing launch
// is that file's; and the staging and the pinned batches are bounded in BYTES, which is one more reason for a round to end
// (xl_spectrum_bank_plan.h: a round's row budget).  The cut, the runs, the tables and the row stores are the same.
// Rows: a batch's rows are moved into their streams' host stores once its event has completed (looked at, without waiting, at the
// start of every feed; waited for by take_rows of a stream that has rows in flight).  The stores grow; rows are never lost.
#include "../../include/xlating_spectrum.h"

#include <errno.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <deque>
#include <new>
#include <utility>
#include <vector>

#include "xl_bank_host.h"
#include "xl_common.h"
#include "xl_device.h"
#include "xl_spectrum.h"
#include "xl_spectrum_bank.h"
#include "xl_spectrum_bank_plan.h"
#include "xl_spectrum_cut.h"
#include "xl_spectrum_wide_plan.h"

#define XL_BANK_MAX_STREAMS 65536

namespace {

struct XlBankStream {
  bool live = false;
  uint32_t gen = 0;  // counts the uses of this id: rows in flight of an earlier use are dropped
  uint32_t sr = 0, F = 0;
  int64_t P = 0, rows_done = 0;
  int pending = 0;    // rows queued and not taken
  int in_flight = 0;  // of those, rows still in a batch
  uint64_t mark = 0;  // the feed that named this stream last (duplicate check)
  std::vector<float> db;  // the un-taken rows that have arrived, from row `head`
  std::vector<uint8_t> px;
  size_t head = 0;
};

struct XlBankBatch {
  float *h_db = nullptr;
  uint8_t *h_px = nullptr;
  size_t cap = 0;  // rows
  hipEvent_t ev = nullptr;
  std::vector<std::pair<uint32_t, uint32_t>> rows;  // (stream id, gen) of row i
};

}  // namespace

struct xlating_spectrum_bank : XlSpecSetup {
  uint32_t slots = 0;
  hipStream_t own = nullptr;  // growth and clearing of the per-stream state
  hipEvent_t last = nullptr;  // behind the latest feed's work
  bool fed = false, broken = false;
  uint32_t cap_streams = 0;
  void *d_carry = nullptr;  // [cap_streams][W] samples
  void *d_max = nullptr;    // [cap_streams * slots][W] uint32_t
  std::vector<XlBankStream> streams;
  std::vector<int> free_ids;
  uint64_t feed_no = 0;
  XlTableRing ring;  // the rounds' tables
  float *d_db = nullptr;  // staging of one round's rows
  uint8_t *d_px = nullptr;
  size_t d_rows_cap = 0;
  std::deque<XlBankBatch *> flying;
  std::vector<XlBankBatch *> idle;
  unsigned launches = 0, copies = 0;
  // one round's tables and the feed's remaining work (members: no allocation per feed once grown)
  std::vector<XlBankRun> runs;
  std::vector<XlBankCarry> ops;
  std::vector<uint32_t> list;
  std::vector<size_t> rem;
  std::vector<const uint8_t *> ptr;
  // a width above XL_SPEC_MAX_W: the two-level transform's scratch ([transform][k1][j2]), how many transforms it holds, and how many rows
  // the staging (and a pinned batch) may hold
  bool wide = false;
  float2 *d_scratch = nullptr;
  uint32_t scratch_T = 0;
  size_t stage_rows = 0;
};

static bool xl_bank_live(const xlating_spectrum_bank *b, int id) {
  return b != nullptr && id >= 0 && (size_t)id < b->streams.size() && b->streams[(size_t)id].live;
}

static void xl_bank_batch_free(XlBankBatch *t) {
  if (t == nullptr) return;
  if (t->h_db) (void)hipHostFree(t->h_db);
  if (t->h_px) (void)hipHostFree(t->h_px);
  if (t->ev) (void)hipEventDestroy(t->ev);
  delete t;
}

// move the rows of completed batches into their streams' stores; wait: of every batch in flight
static int xl_bank_drain(xlating_spectrum_bank *b, bool wait) {
  const size_t W = b->W;
  while (!b->flying.empty()) {
    XlBankBatch *t = b->flying.front();
    if (wait) {
      XL_TRY_RET(hipEventSynchronize(t->ev));
    } else {
      const hipError_t e = hipEventQuery(t->ev);
      if (e == hipErrorNotReady) {
        (void)hipGetLastError();  // (not an error: keep it out of the next launch's hipGetLastError)
        break;
      }
      XL_TRY_RET(e);
    }
    for (size_t i = 0; i < t->rows.size(); ++i) {
      const uint32_t id = t->rows[i].first;
      if (id >= b->streams.size()) continue;
      XlBankStream &s = b->streams[id];
      if (!s.live || s.gen != t->rows[i].second) continue;
      s.db.insert(s.db.end(), t->h_db + i * W, t->h_db + (i + 1) * W);
      s.px.insert(s.px.end(), t->h_px + i * W, t->h_px + (i + 1) * W);
      s.in_flight--;
    }
    t->rows.clear();
    b->flying.pop_front();
    b->idle.push_back(t);
  }
  return 0;
}

// device state for `need` streams: the arrays are replaced by larger ones and the present streams' state moves over
static int xl_bank_reserve_streams(xlating_spectrum_bank *b, uint32_t need) {
  if (need <= b->cap_streams) return 0;
  if (b->fed) XL_TRY_RET(hipEventSynchronize(b->last));
  const XlStreamArray a[] = {{&b->d_carry, (size_t)b->W * b->ssz, false},  // (a carry is appended to from `have` on, saved from 0 on)
                             {&b->d_max, (size_t)b->slots * b->W * sizeof(uint32_t), true}};
  const uint32_t first = b->wide ? xl_bankw_first_streams(a[0].stride + a[1].stride) : 64u;
  return xl_streams_grow(&b->cap_streams, need, a, b->own, "spectrum bank: state", first);
}

// rows to allocate for a staging or a batch that must hold `rows`: twice that and 64 at least; a wide bank's are bounded in bytes
// (stage_rows >= rows: the round's budget)
static size_t xl_bank_rows_cap(const xlating_spectrum_bank *b, size_t rows) {
  const size_t cap = std::max<size_t>(rows * 2, 64);
  return b->wide ? std::max(rows, std::min(cap, b->stage_rows)) : cap;
}

static int xl_bank_batch(xlating_spectrum_bank *b, size_t rows, XlBankBatch **out) {
  XlBankBatch *t = nullptr;
  for (size_t i = 0; i < b->idle.size(); ++i)
    if (b->idle[i]->cap >= rows) {
      t = b->idle[i];
      b->idle.erase(b->idle.begin() + (long)i);
      break;
    }
  if (t == nullptr) {
    if (!b->idle.empty()) {  // (too small: replaced, so that the pool does not grow without bound)
      xl_bank_batch_free(b->idle.back());
      b->idle.pop_back();
    }
    t = new XlBankBatch();
    const size_t cap = xl_bank_rows_cap(b, rows);
    hipError_t e = hipEventCreateWithFlags(&t->ev, hipEventDisableTiming);
    if (e == hipSuccess) e = hipHostMalloc(&t->h_db, cap * b->W * sizeof(float), hipHostMallocDefault);
    if (e == hipSuccess) e = hipHostMalloc(&t->h_px, cap * b->W, hipHostMallocDefault);
    if (e != hipSuccess) {
      xl_bank_batch_free(t);
      XL_TRY_RET(e);
    }
    t->cap = cap;
  }
  *out = t;
  return 0;
}

static size_t xl_bank_align(size_t v) { return (v + 15u) & ~(size_t)15u; }

// one round: every stream with samples left consumes up to its round limit
static int xl_bank_round(xlating_spectrum_bank *b, size_t n, const int *ids, hipStream_t st) {
  const int64_t W = b->W;
  b->runs.clear(), b->ops.clear(), b->list.clear();
  XlBankBatch *batch = nullptr;
  std::vector<std::pair<uint32_t, uint32_t>> owners;
  uint32_t T = 0;
  bool any_app = false, any_save = false;
  int64_t budget = (int64_t)b->stage_rows;  // (wide) rows this round may still complete
  for (size_t i = 0; i < n; ++i) {
    if (b->rem[i] == 0) continue;
    const uint32_t id = (uint32_t)ids[i];
    XlBankStream &s = b->streams[id];
    const int64_t lim = b->wide ? xl_bankw_round_limit(s.sr, W, s.P, b->slots, budget) : xl_spec_round_limit(s.sr, s.P, b->slots);
    if (lim == 0) continue;  // (wide: the staging is full; the stream goes on in the next round)
    const int64_t c = std::min<int64_t>((int64_t)b->rem[i], lim);
    const XlSpecCut cut = xl_spec_cut(s.sr, W, s.P, c);
    if (cut.carry_app > 0 || cut.save_n > 0) {
      XlBankCarry op;
      op.src = b->ptr[i], op.stream = id, op.have = (uint32_t)cut.carry_have, op.app = (uint32_t)cut.carry_app;
      op.save_off = (uint32_t)cut.save_off, op.save_n = (uint32_t)cut.save_n, op.pad = 0;
      b->ops.push_back(op);
      any_app |= cut.carry_app > 0, any_save |= cut.save_n > 0;
    }
    XlBankRun r;
    r.F = s.F, r.sr = s.sr, r.slot0 = id * b->slots;
    if (cut.carry_done) {  // the completed straddling transform: one more run, read from the carry
      r.src = static_cast<const uint8_t *>(b->d_carry) + (size_t)id * W * b->ssz, r.base = cut.carry_t0, r.g0 = cut.carry_g, r.tsum = T;
      b->runs.push_back(r);
      T += 1u;
    }
    if (cut.T > 0) {
      r.src = b->ptr[i], r.base = s.P, r.g0 = cut.g_first, r.tsum = T;
      b->runs.push_back(r);
      T += (uint32_t)cut.T;
    }
    for (int64_t row = s.rows_done; row < cut.rows_done; ++row) {
      b->list.push_back(id * b->slots + (uint32_t)(row % b->slots));
      owners.emplace_back(id, s.gen);
    }
    const int done = (int)std::max<int64_t>(cut.rows_done - s.rows_done, 0);
    budget -= done;
    s.pending += done, s.in_flight += done;
    s.rows_done = std::max(s.rows_done, cut.rows_done);
    s.P += c;
    b->ptr[i] += (size_t)c * b->ssz;
    b->rem[i] -= (size_t)c;
  }
  // the table: runs, carry operations, row list
  const size_t o_ops = xl_bank_align(b->runs.size() * sizeof(XlBankRun));
  const size_t o_list = o_ops + xl_bank_align(b->ops.size() * sizeof(XlBankCarry));
  const size_t bytes = o_list + xl_bank_align(b->list.size() * sizeof(uint32_t));
  if (bytes == 0) return 0;
  XlRingTable *t = nullptr;
  XL_TRY_RET(xl_ring_acquire(&b->ring, bytes, &t));
  if (b->ring.d_cap < bytes) {
    XL_TRY_RET(hipStreamSynchronize(st));  // (this feed's earlier rounds read the table that is replaced)
    XL_TRY_RET(xl_ring_dev_grow(&b->ring, bytes));
  }
  uint8_t *h = static_cast<uint8_t *>(t->h);
  if (!b->runs.empty()) memcpy(h, b->runs.data(), b->runs.size() * sizeof(XlBankRun));
  if (!b->ops.empty()) memcpy(h + o_ops, b->ops.data(), b->ops.size() * sizeof(XlBankCarry));
  if (!b->list.empty()) memcpy(h + o_list, b->list.data(), b->list.size() * sizeof(uint32_t));
  XL_TRY_RET(xl_ring_upload(&b->ring, t, bytes, st));
  b->copies += 1;
  uint8_t *d = static_cast<uint8_t *>(b->ring.d_tab);
  const XlBankCarry *d_ops = reinterpret_cast<const XlBankCarry *>(d + o_ops);
  uint32_t *const d_max = static_cast<uint32_t *>(b->d_max);
  const auto carry = b->wide ? xl_bankw_carry : xl_bank_carry;
  if (any_app) {
    XL_TRY_RET(carry(d_ops, (uint32_t)b->ops.size(), b->d_carry, b->W, b->ssz, false, st));
    b->launches += 1;
  }
  if (T > 0) {
    XlBankArgs a;
    a.runs = reinterpret_cast<const XlBankRun *>(d), a.nruns = (uint32_t)b->runs.size(), a.T = T, a.W = b->W, a.slots = b->slots;
    a.rowmax = d_max, a.tw = b->d_tw, a.chirp = b->d_chirp, a.bspec = b->d_bspec, a.norm = 1.0f / (float)b->W;
    if (!b->wide) {
      XL_TRY_RET(xl_bank_launch(a, b->N, b->blue, b->fmt, st));
      b->launches += 1;
    } else {
      XlBankWideArgs w;
      w.a = a, w.scratch = b->d_scratch, w.tw1 = b->d_tw1, w.tw2 = b->d_tw2, w.N = b->N, w.N1 = b->N1, w.N2 = b->N2;
      const uint64_t chunks = xl_bankw_chunks(T, b->scratch_T);
      for (uint64_t i = 0; i < chunks; ++i) {
        w.t0 = (uint32_t)(i * b->scratch_T), w.Tc = (uint32_t)xl_bankw_chunk_len(T, b->scratch_T, i);
        XL_TRY_RET(xl_bankw_launch(w, b->blue, b->fmt, st));
        b->launches += xl_bankw_passes(b->blue);
      }
    }
  }
  if (any_save) {
    XL_TRY_RET(carry(d_ops, (uint32_t)b->ops.size(), b->d_carry, b->W, b->ssz, true, st));
    b->launches += 1;
  }
  const size_t nrows = b->list.size();
  if (nrows > 0) {
    if (b->d_rows_cap < nrows) {
      XL_TRY_RET(hipStreamSynchronize(st));  // (earlier rounds' copies read the staging that is replaced)
      if (b->d_db) (void)hipFree(b->d_db);
      if (b->d_px) (void)hipFree(b->d_px);
      b->d_db = nullptr, b->d_px = nullptr, b->d_rows_cap = 0;
      const size_t cap = xl_bank_rows_cap(b, nrows);
      XL_TRY_RET(hipMalloc(&b->d_db, cap * b->W * sizeof(float)));
      XL_TRY_RET(hipMalloc(&b->d_px, cap * b->W));
      b->d_rows_cap = cap;
    }
    const int rc = xl_bank_batch(b, nrows, &batch);
    if (rc != 0) return rc;
    batch->rows.swap(owners);
    b->flying.push_back(batch);
    const uint32_t *d_list = reinterpret_cast<const uint32_t *>(d + o_list);
    if (b->wide)
      XL_TRY_RET(xl_bankw_finish(d_list, (uint32_t)nrows, d_max, b->d_db, b->d_px, b->W, b->N1, b->N2, !b->blue, st));
    else
      XL_TRY_RET(xl_bank_finish(d_list, (uint32_t)nrows, d_max, b->d_db, b->d_px, b->W, st));
    XL_TRY_RET(hipMemcpyAsync(batch->h_db, b->d_db, nrows * b->W * sizeof(float), hipMemcpyDeviceToHost, st));
    XL_TRY_RET(hipMemcpyAsync(batch->h_px, b->d_px, nrows * b->W, hipMemcpyDeviceToHost, st));
    XL_TRY_RET(hipEventRecord(batch->ev, st));
    b->launches += 1;
    b->copies += 2;
  }
  return 0;
}

static int xl_bank_feed(xlating_spectrum_bank *b, size_t n, const int *ids, const void *const *dev_samples, const size_t *counts,
                        hipStream_t st) {
  b->feed_no++;
  uint64_t total_t = 0;
  for (size_t i = 0; i < n; ++i) {
    if (!xl_bank_live(b, ids[i]) || counts[i] > XL_SPEC_SPAN_MAX || (counts[i] > 0 && dev_samples[i] == nullptr)) return -EINVAL;
    XlBankStream &s = b->streams[(size_t)ids[i]];
    if (s.mark == b->feed_no) return -EINVAL;  // named twice
    s.mark = b->feed_no;
    total_t += counts[i] / b->W + 2u;
  }
  if (total_t > ((uint64_t)1 << 31)) return -EINVAL;  // (the ragged launch counts its transforms in 32 bits)
  b->launches = b->copies = 0;
  XL_TRY_RET(hipSetDevice(b->device));
  int rc = xl_bank_drain(b, false);
  if (rc != 0) return rc;
  b->rem.assign(counts, counts + n);
  b->ptr.resize(n);
  bool any = false;
  for (size_t i = 0; i < n; ++i) b->ptr[i] = static_cast<const uint8_t *>(dev_samples[i]), any |= counts[i] > 0;
  if (!any) return 0;
  if (b->fed) XL_TRY_RET(hipStreamWaitEvent(st, b->last, 0));
  while (any) {
    if ((rc = xl_bank_round(b, n, ids, st)) != 0) return rc;
    any = false;
    for (size_t i = 0; i < n; ++i) any |= b->rem[i] > 0;
  }
  XL_TRY_RET(hipEventRecord(b->last, st));
  b->fed = true;
  return 0;
}

// ---------------------------------------------------------------------------------------------------------- C API
static int xl_bank_create_cap(int width, int max_width, int format, xlating_spectrum_bank **out, const char *who) {
  if (out == nullptr) return -EINVAL;
  XlSpecSetup u;
  int rc = xl_spec_setup_init(&u, width, max_width, format, who);
  if (rc == -EINVAL) return rc;  // (as the refusal above: *out is left alone)
  *out = nullptr;
  if (rc != 0) return rc;
  xlating_spectrum_bank *b = new (std::nothrow) xlating_spectrum_bank();
  if (b == nullptr) {
    xl_spec_setup_free(&u);
    return -ENOMEM;
  }
  static_cast<XlSpecSetup &>(*b) = u;
  b->slots = std::min(16u, std::max(2u, 16384u / b->W));  // 64 KiB of maxima per stream at most
  if (const char *e = xl_exp_getenv("XL_EXP_SPEC_BANK_SLOTS")) {  // test knob: row slots per stream (rounds per feed)
    const long v = strtol(e, nullptr, 10);
    if (v > 0 && v <= 1024) b->slots = (uint32_t)v;
  }
  hipError_t e = hipStreamCreateWithFlags(&b->own, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&b->last, hipEventDisableTiming);
  if (e == hipSuccess) e = xl_ring_init(&b->ring);
  if (e == hipSuccess && b->W > XL_SPEC_MAX_W) {
    uint64_t stage = XL_BANKW_STAGE_DEFAULT;
    if (const char *v = xl_exp_getenv("XL_EXP_SPEC_BANK_STAGE")) {  // test knob: the staging's size in bytes (rows per round)
      const long long sb = strtoll(v, nullptr, 10);
      if (sb > 0) stage = (uint64_t)std::min<long long>(sb, 1ll << 30);
    }
    b->wide = true;
    b->stage_rows = (size_t)xl_bankw_stage_rows(stage, b->W);
    b->scratch_T = (uint32_t)xl_specw_chunk(xl_specw_scratch_bytes(), b->N);
    e = hipMalloc(&b->d_scratch, sizeof(float2) * (size_t)b->N * b->scratch_T);
  }
  if (e != hipSuccess) {
    xl_last_hip_error = e;
    XL_LOG_ERR("%s: %s", who, hipGetErrorString(e));
    rc = xl_errno_of_last_hip_error();
    xlating_spectrum_bank_destroy(b);
    return rc;
  }
  *out = b;
  return 0;
}

extern "C" int xlating_spectrum_bank_create(int width, int format, xlating_spectrum_bank **out) {
  return xl_bank_create_cap(width, XLATING_SPECTRUM_MAX_WIDTH, format, out, "xlating_spectrum_bank_create");
}

extern "C" int xlating_spectrum_bank_create_wide(int width, int format, xlating_spectrum_bank **out) {
  return xl_bank_create_cap(width, XLATING_SPECTRUM_MAX_WIDE_WIDTH, format, out, "xlating_spectrum_bank_create_wide");
}

extern "C" int xlating_spectrum_bank_add(xlating_spectrum_bank *b, uint32_t sampling_rate) {
  if (b == nullptr || sampling_rate == 0 || sampling_rate < b->W) return -EINVAL;
  if (b->broken) return -EIO;
  try {
    const bool reuse = !b->free_ids.empty();
    const size_t id = reuse ? (size_t)b->free_ids.back() : b->streams.size();
    if (id >= XL_BANK_MAX_STREAMS) return -ENOMEM;
    XL_TRY_RET(hipSetDevice(b->device));
    const int rc = xl_bank_reserve_streams(b, (uint32_t)id + 1u);
    if (rc != 0) return rc;
    if (reuse)
      b->free_ids.pop_back();
    else
      b->streams.emplace_back();
    XlBankStream &s = b->streams[id];
    s.live = true, s.sr = sampling_rate, s.F = sampling_rate / b->W, s.P = 0, s.rows_done = 0, s.pending = 0, s.in_flight = 0, s.head = 0;
    s.db.clear(), s.px.clear();
    return (int)id;
  } catch (const std::bad_alloc &) {
    return -ENOMEM;
  }
}

extern "C" int xlating_spectrum_bank_remove(xlating_spectrum_bank *b, int stream_id) {
  if (!xl_bank_live(b, stream_id)) return -EINVAL;
  XlBankStream &s = b->streams[(size_t)stream_id];
  if (s.P > 0 && !b->broken) {  // a row in progress leaves maxima behind: clear the id's slots for its next use
    XL_TRY_RET(hipSetDevice(b->device));
    if (b->fed) XL_TRY_RET(hipEventSynchronize(b->last));
    const size_t mbytes = (size_t)b->slots * b->W * sizeof(uint32_t);
    XL_TRY_RET(hipMemsetAsync(static_cast<uint8_t *>(b->d_max) + (size_t)stream_id * mbytes, 0, mbytes, b->own));
    XL_TRY_RET(hipStreamSynchronize(b->own));
  }
  s.live = false;
  s.gen++;
  s.pending = s.in_flight = 0;
  std::vector<float>().swap(s.db);
  std::vector<uint8_t>().swap(s.px);
  s.head = 0;
  try {
    b->free_ids.push_back(stream_id);
  } catch (const std::bad_alloc &) {  // (the id is then not reused)
  }
  return 0;
}

extern "C" int xlating_spectrum_bank_feed_device(xlating_spectrum_bank *b, size_t n, const int *ids, const void *const *dev_samples,
                                                 const size_t *counts, void *hip_stream) {
  if (b == nullptr || (n > 0 && (ids == nullptr || dev_samples == nullptr || counts == nullptr))) return -EINVAL;
  if (b->broken) return -EIO;
  if (n == 0) {
    b->launches = b->copies = 0;
    return 0;
  }
  int rc;
  try {
    rc = xl_bank_feed(b, n, ids, dev_samples, counts, static_cast<hipStream_t>(hip_stream));
  } catch (const std::bad_alloc &) {
    rc = -ENOMEM;
  }
  if (rc != 0 && rc != -EINVAL) b->broken = true;  // (-EINVAL is decided before anything is consumed)
  return rc;
}

extern "C" int xlating_spectrum_bank_take_rows(xlating_spectrum_bank *b, int stream_id, float *db, uint8_t *pixels, size_t max_rows) {
  if (!xl_bank_live(b, stream_id)) return -EINVAL;
  if (b->broken) return -EIO;
  XlBankStream &s = b->streams[(size_t)stream_id];
  if (s.in_flight > 0) {
    XL_TRY_RET(hipSetDevice(b->device));
    int rc;
    try {
      rc = xl_bank_drain(b, true);
    } catch (const std::bad_alloc &) {
      rc = -ENOMEM;
    }
    if (rc != 0) {
      b->broken = true;
      return rc;
    }
  }
  const size_t W = b->W, have = s.px.size() / W - s.head;
  const size_t n = std::min(std::min<size_t>(max_rows, 1u << 30), have);
  if (db != nullptr && n > 0) memcpy(db, s.db.data() + s.head * W, n * W * sizeof(float));
  if (pixels != nullptr && n > 0) memcpy(pixels, s.px.data() + s.head * W, n * W);
  s.head += n;
  s.pending -= (int)n;
  if (s.head * W == s.px.size()) s.db.clear(), s.px.clear(), s.head = 0;
  return (int)n;
}

extern "C" int xlating_spectrum_bank_rows_pending(const xlating_spectrum_bank *b, int stream_id) {
  if (!xl_bank_live(b, stream_id)) return -EINVAL;
  return b->streams[(size_t)stream_id].pending;
}

extern "C" int xlating_spectrum_bank_last_feed_ops(const xlating_spectrum_bank *b, unsigned *launches, unsigned *copies) {
  if (b == nullptr) return -EINVAL;
  if (launches) *launches = b->launches;
  if (copies) *copies = b->copies;
  return 0;
}

extern "C" void xlating_spectrum_bank_destroy(xlating_spectrum_bank *b) {
  if (b == nullptr) return;
  (void)hipSetDevice(b->device);
  if (b->fed) (void)hipEventSynchronize(b->last);
  if (b->own) (void)hipStreamSynchronize(b->own);
  for (XlBankBatch *t : b->flying) xl_bank_batch_free(t);
  for (XlBankBatch *t : b->idle) xl_bank_batch_free(t);
  xl_ring_destroy(&b->ring);
  if (b->d_db) (void)hipFree(b->d_db);
  if (b->d_px) (void)hipFree(b->d_px);
  if (b->d_carry) (void)hipFree(b->d_carry);
  if (b->d_max) (void)hipFree(b->d_max);
  if (b->d_scratch) (void)hipFree(b->d_scratch);
  xl_spec_setup_free(b);
  if (b->last) (void)hipEventDestroy(b->last);
  if (b->own) (void)hipStreamDestroy(b->own);
  delete b;
}
