// xl_serve.cpp -- the serve object (include/xlating_serve.h): one band on one GPU, from the wire request to the sink.  It owns an
// engine, at most one resampler bank of its family, at most one tuner bank, at most one power meter, a delivery object and the sinks, and
// calls nothing but their public functions; the ordering rule between them is stated in the header and kept in xl_serve_run below.  No arithmetic on samples
// happens here.
#include "../../include/xlating_serve.h"

#include <errno.h>
#include <stdlib.h>

#include <algorithm>
#include <map>
#include <new>
#include <string>
#include <vector>

#include "../../include/xlating_batch.h"
#include "../../include/xlating_delivery.h"
#include "../../include/xlating_meter.h"
#include "../../include/xlating_resample.h"
#include "../../include/xlating_resample_q15.h"
#include "../../include/xlating_sinks.h"
#include "../../include/xlating_tune.h"
#include "../../include/xlating_wire.h"
#include "xl_common.h"
#include "xl_serve_gain.h"
#include "xl_serve_squelch.h"

namespace {

// the latest XL_SERVE_TUNE_LOG changes of a client's rotation, oldest first (xlating_serve_tune_log)
#define XL_SERVE_TUNE_LOG 64
struct XlServeTuneLog {
  uint64_t first_sample[XL_SERVE_TUNE_LOG];
  int64_t F[XL_SERVE_TUNE_LOG], R[XL_SERVE_TUNE_LOG];
  uint32_t n = 0, head = 0;
};

struct XlServeClient {
  int rs = -1;           // its stream of the resampler bank, or -1: the rate divides the band rate
  uint32_t band_freq = 0;
  // xlating_serve_set_tune: the client's stream of the tuner bank (-1 until its first call), its final rate, the log of its changes
  int tn = -1;
  bool tn_fed = false;   // the latest blocks call rotated its row
  double rate = 0.0;
  XlServeTuneLog tune_log;
  // XL_SERVE_CF32_AS_CS16: the client's gain and meter (xl_serve_gain.h holds the policy and the log)
  int8_t gain = 0;       // from the next call that is packed
  bool agc = false;      // xlating_serve_set_auto_gain
  XlServeGainState agc_state = {0};
  XlServeGainLog log = {};
  uint64_t packed = 0;   // samples of its delivered stream packed so far: where a new gain or a new rotation begins
  uint64_t clipped_total = 0;
  uint32_t peak_bits = 0, clipped = 0, nans = 0;  // of the latest call queued to its sink
  int8_t level_gain = 0;                          // the gain that call was packed with
  // xlating_serve_set_squelch (xl_serve_squelch.h holds the policy and the log)
  bool sq_on = false;
  XlServeSquelch sq = {};
  XlServeSquelchLog sq_log = {};
  uint64_t produced = 0;   // samples of its final rows so far, delivered or withheld
  uint64_t withheld = 0;   // of those, the samples of the calls its gate was closed in
  double sq_power = 0.0;   // the latest call's mean power (0 while the client has no squelch) ...
  bool sq_open = true;     // ... and gate
};

}  // namespace

struct xlating_serve_t {
  xlating_serve_config cfg;
  std::string base_path;
  int device = 0, mode = XL_MODE_OPTIMIZED;
  size_t esz = 8;  // bytes per delivered sample
  bool narrow = false;  // XL_SERVE_CF32_AS_CS16: the cf32 family's rows, narrowed by the pack launch
  xlating_batch *eng = nullptr;
  xlating_sinks *sinks = nullptr;
  xlating_delivery *dlv = nullptr;
  xlating_resample_bank *rb = nullptr;       // cf32 family, created with the first fractional client
  xlating_resample_q15_bank *rq = nullptr;   // cs16 family
  xlating_tune_bank *tb = nullptr;           // created with the first xlating_serve_set_tune
  xlating_meter *mt = nullptr;               // created with the first xlating_serve_set_squelch
  hipStream_t st = nullptr;                  // the feed and the pack launch
  hipEvent_t ev_call = nullptr, ev_pack = nullptr;  // behind the engine call; behind the pack launch
  bool packed = false;                       // ev_pack has been recorded
  std::map<int, XlServeClient> clients;
  int pending = -1;                          // the ticket not handed to the sinks yet
  std::vector<int> pending_ids;              // its keys that are still owed their row (a client that is forgotten leaves the list)
  std::vector<int> handing;                  // (scratch of a hand-over)
  std::vector<int> pending_withheld, handing_withheld;  // the ticket's keys whose gate was closed (ascending): rows of length 0
  bool levels_on = false;                    // xlating_serve_enable_levels
  bool pending_gained = false, handing_gained = false;  // the ticket is one of pack_device_cs16_gain ...
  std::map<int, int8_t> pending_gain, handing_gain;     // ... packed with these gains, by client id
  std::vector<int8_t> gains;                 // (scratch of a call)
  std::vector<int> dropped;
  unsigned launches = 0, copies = 0;
  uint64_t d2h_bytes = 0;
  // (scratch of a call)
  std::vector<int> ids, rs_ids, tn_ids;
  std::vector<const void *> rows, rs_rows, tn_rows;
  std::vector<size_t> lens, rs_lens, tn_lens, bytes;
  std::vector<const void *> sq_rows;
  std::vector<size_t> sq_lens, sq_at;
};

// the bank's functions for either family
static int xl_serve_bank_add(xlating_serve *s, uint32_t L, uint32_t M, const float *taps, size_t len) {
  if (s->cfg.family == XL_SERVE_CS16) {
    if (s->rq == nullptr) {
      const int rc = xlating_resample_q15_bank_create(&s->rq);
      if (rc != 0) return rc;
    }
    return xlating_resample_q15_bank_add(s->rq, L, M, taps, len);
  }
  if (s->rb == nullptr) {
    const int rc = xlating_resample_bank_create(&s->rb);
    if (rc != 0) return rc;
  }
  return xlating_resample_bank_add(s->rb, L, M, taps, len);
}

static int xl_serve_bank_remove(xlating_serve *s, int rs) {
  return s->cfg.family == XL_SERVE_CS16 ? xlating_resample_q15_bank_remove(s->rq, rs) : xlating_resample_bank_remove(s->rb, rs);
}

static int xl_serve_bank_feed(xlating_serve *s, size_t n, const int *ids, const void *const *rows, const size_t *counts) {
  return s->cfg.family == XL_SERVE_CS16 ? xlating_resample_q15_bank_feed_device(s->rq, n, ids, rows, counts, s->st)
                                        : xlating_resample_bank_feed_device(s->rb, n, ids, rows, counts, s->st);
}

static int xl_serve_bank_output(xlating_serve *s, int rs, const void **row, size_t *n) {
  return s->cfg.family == XL_SERVE_CS16 ? xlating_resample_q15_bank_output_device(s->rq, rs, row, n)
                                        : xlating_resample_bank_output_device(s->rb, rs, row, n);
}

static void xl_serve_bank_ops(xlating_serve *s, unsigned *launches, unsigned *copies) {
  if (s->cfg.family == XL_SERVE_CS16) (void)xlating_resample_q15_bank_last_feed_ops(s->rq, launches, copies);
  else (void)xlating_resample_bank_last_feed_ops(s->rb, launches, copies);
}

// the client leaves the engine, the banks and the sinks
static void xl_serve_forget(xlating_serve *s, int id) {
  const auto it = s->clients.find(id);
  if (it == s->clients.end()) return;
  (void)xlating_sinks_detach(s->sinks, id);
  (void)xlating_batch_remove_client(s->eng, id);
  if (it->second.rs >= 0) (void)xl_serve_bank_remove(s, it->second.rs);
  if (it->second.tn >= 0) (void)xlating_tune_bank_remove(s->tb, it->second.tn);
  s->clients.erase(it);
  // the row the pending ticket holds under this id is nobody's now: the engine gives the id to the next client that joins, and that
  // client's stream starts with its own first block
  s->pending_ids.erase(std::remove(s->pending_ids.begin(), s->pending_ids.end(), id), s->pending_ids.end());
}

// sinks that failed since the last look: their clients are removed and reported
static void xl_serve_reap(xlating_serve *s) {
  int ids[64];
  for (;;) {
    const size_t n = xlating_sinks_failed(s->sinks, ids, 64);
    for (size_t i = 0; i < n; ++i) {
      if (s->clients.count(ids[i]) == 0) continue;
      xl_serve_forget(s, ids[i]);
      s->dropped.push_back(ids[i]);
    }
    if (n < 64) break;
  }
}

// ticket t's rows go to the sinks of the clients of s->handing (its keys still owed their row) that are still here; the ticket is
// released.  xl_serve_forget edits pending_ids, never handing: a sink that fails here takes its client out of the NEXT ticket's list.
static int xl_serve_deliver(xlating_serve *s, int t) {
  int rc = xlating_delivery_wait(s->dlv, t);
  for (size_t i = 0; rc == 0 && i < s->handing.size(); ++i) {
    const int id = s->handing[i];
    if (s->clients.count(id) == 0) continue;  // (dropped earlier in this loop's reap: cannot be a newcomer, nobody joins in here)
    const void *p = nullptr;
    size_t n = 0;
    if ((rc = xlating_delivery_row(s->dlv, t, id, &p, &n)) != 0) break;
    if (n > 0) (void)xlating_sinks_write_bytes(s->sinks, id, p, n);  // (-EPIPE: reported by xlating_sinks_failed below)
    // a row the squelch withheld: to the levels, the gain policy and the gain log this call did not happen
    if (std::binary_search(s->handing_withheld.begin(), s->handing_withheld.end(), id)) continue;
    if (!s->handing_gained) continue;
    // the row's level, and what the client's policy makes of it: a new gain holds from the next call that is packed
    XlServeClient &c = s->clients[id];
    if ((rc = xlating_delivery_row_level(s->dlv, t, id, &c.peak_bits, &c.clipped, &c.nans)) != 0) break;
    c.level_gain = s->handing_gain[id];
    c.clipped_total += c.clipped;
    if (!c.agc) continue;
    const int32_t g = xl_serve_gain_step(&c.agc_state, c.peak_bits, c.clipped, c.level_gain, c.gain);
    if (g != c.gain) xl_serve_gain_log_add(&c.log, c.packed, g);
    c.gain = (int8_t)g;
  }
  s->handing.clear(), s->handing_withheld.clear();
  const int rr = xlating_delivery_release(s->dlv, t);
  xl_serve_reap(s);
  return rc != 0 ? rc : rr;
}

// the pending ticket, if there is one
static int xl_serve_hand_over(xlating_serve *s) {
  if (s->pending < 0) return 0;
  const int t = s->pending;
  s->pending = -1;
  s->handing.swap(s->pending_ids);
  s->pending_ids.clear();
  s->handing_withheld.swap(s->pending_withheld);
  s->pending_withheld.clear();
  s->handing_gain.swap(s->pending_gain), s->handing_gained = s->pending_gained;
  s->pending_gain.clear(), s->pending_gained = false;
  return xl_serve_deliver(s, t);
}

extern "C" int xlating_serve_create(const xlating_serve_config *cfg, xlating_serve **out) {
  if (out == nullptr) return -EINVAL;
  *out = nullptr;
  if (cfg == nullptr || cfg->band_sampling_rate == 0 || cfg->base_path == nullptr ||
      (cfg->family != XL_SERVE_CF32 && cfg->family != XL_SERVE_CS16 && cfg->family != XL_SERVE_CF32_AS_CS16) ||
      (cfg->family == XL_SERVE_CS16 && cfg->input_format == XL_FMT_CF32))
    return -EINVAL;
  xlating_serve *s = new (std::nothrow) xlating_serve_t();
  if (s == nullptr) return -ENOMEM;
  int rc = 0;
  try {
    s->cfg = *cfg;
    s->base_path = cfg->base_path;
    s->cfg.base_path = s->base_path.c_str();
    if (s->cfg.group_blocks == 0) s->cfg.group_blocks = 1;
    if (s->cfg.lpf_cutoff_rate == 0) s->cfg.lpf_cutoff_rate = 5;
    if (s->cfg.writer_threads == 0) s->cfg.writer_threads = 2;
    if (s->cfg.delivery_slots == 0) s->cfg.delivery_slots = 2;
    // (8 calls of a client at a quarter of the band rate, 8 bytes a sample; allocated per client when its sink is attached)
    // (the narrowing family's at its 4 bytes a sample)
    s->narrow = cfg->family == XL_SERVE_CF32_AS_CS16;
    if (s->cfg.queue_bytes == 0)
      s->cfg.queue_bytes = (size_t)8 * s->cfg.group_blocks * ((size_t)s->cfg.buffer_size / 2 / 4 + 64) * (s->narrow ? 4 : 8);
    s->mode = cfg->family == XL_SERVE_CS16 ? XL_MODE_Q15 : (cfg->native ? XL_MODE_NATIVE : XL_MODE_OPTIMIZED);
    s->esz = cfg->family == XL_SERVE_CF32 ? 8 : 4;
    s->device = xl_hip_select_device(cfg->device);
    if (s->device < 0) {
      XL_LOG_ERR("xlating_serve_create: no usable HIP device (%s); there is no CPU path", xlating_hip_device_info());
      rc = -ENODEV;
    }
    if (rc == 0 && hipSetDevice(s->device) != hipSuccess) rc = -EIO;  // (the bank and the delivery belong to the current device)
    if (rc == 0)
      rc = xlating_batch_create_grouped(cfg->band_sampling_rate, cfg->input_format, cfg->buffer_size, s->cfg.group_blocks, s->device, &s->eng);
    if (rc == 0) rc = xlating_sinks_create(s->cfg.writer_threads, s->cfg.queue_bytes, &s->sinks);
    if (rc == 0) rc = xlating_delivery_create(s->cfg.delivery_slots, &s->dlv);
    if (rc == 0) {
      hipError_t e = hipStreamCreateWithFlags(&s->st, hipStreamNonBlocking);
      if (e == hipSuccess) e = hipEventCreateWithFlags(&s->ev_call, hipEventDisableTiming);
      if (e == hipSuccess) e = hipEventCreateWithFlags(&s->ev_pack, hipEventDisableTiming);
      if (e != hipSuccess) {
        xl_last_hip_error = e;
        XL_LOG_ERR("xlating_serve_create: %s", hipGetErrorString(e));
        rc = xl_errno_of_last_hip_error();
      }
    }
  } catch (const std::bad_alloc &) {
    rc = -ENOMEM;
  }
  if (rc != 0) {
    xlating_serve_destroy(s);
    return rc;
  }
  *out = s;
  return 0;
}

static int xl_serve_refuse(uint32_t details, uint8_t response[7], size_t *response_len) {
  *response_len = xlating_wire_build_response(XL_WIRE_STATUS_FAILURE, details, response);
  return 1;
}

extern "C" int xlating_serve_request(xlating_serve *s, const uint8_t *msg, size_t len, int socket_fd, uint8_t response[7],
                                     size_t *response_len, int *client_id) {
  if (s == nullptr || msg == nullptr || response == nullptr || response_len == nullptr || client_id == nullptr) return -EINVAL;
  uint8_t type = 0;
  int rc = xlating_wire_parse_header(msg, len, &type);
  if (rc != 0) return rc;
  if (type != XL_WIRE_TYPE_REQUEST) return -EPROTO;
  xlating_wire_request req;
  if ((rc = xlating_wire_parse_request(msg + XL_WIRE_HEADER_BYTES, len - XL_WIRE_HEADER_BYTES, &req)) != 0) return rc;
  const uint32_t band = s->clients.empty() ? 0u : s->clients.begin()->second.band_freq;
  xlating_wire_admission adm;
  xlating_wire_resample rs = {1u, 1u, 0u};
  uint32_t why = 0;
  rc = s->cfg.any_rate ? xlating_wire_admit_any_rate(&req, s->cfg.band_sampling_rate, band, s->cfg.lpf_cutoff_rate, &adm, &rs, &why)
                       : xlating_wire_admit(&req, s->cfg.band_sampling_rate, band, s->cfg.lpf_cutoff_rate, &adm, &why);
  if (rc != 0) return xl_serve_refuse(why, response, response_len);
  if (req.destination == XL_WIRE_DESTINATION_SOCKET && socket_fd < 0) return xl_serve_refuse(XL_WIRE_DETAILS_INTERNAL_ERROR, response, response_len);
  const bool second = rs.L != 1u || rs.M != 1u;
  float *rtaps = nullptr;
  size_t rlen = 0;
  if (second && xlating_wire_resample_taps(&req, &rs, s->cfg.lpf_cutoff_rate, &rtaps, &rlen) != 0)
    return xl_serve_refuse(XL_WIRE_DETAILS_INTERNAL_ERROR, response, response_len);
  // what is added from here on is undone on failure
  (void)hipSetDevice(s->device);
  const int id = xlating_wire_add_client(s->eng, &adm, s->cfg.band_sampling_rate);
  int rsid = -1;
  bool ok = id >= 0;
  if (ok && second) ok = (rsid = xl_serve_bank_add(s, rs.L, rs.M, rtaps, rlen)) >= 0;
  free(rtaps);
  bool sink = false;
  if (ok) {
    const char *ext = s->cfg.family == XL_SERVE_CF32 ? "cf32" : "cs16";
    rc = req.destination == XL_WIRE_DESTINATION_FILE ? xlating_sinks_attach_file_as(s->sinks, id, s->base_path.c_str(), ext, s->cfg.use_gzip)
                                                      : xlating_sinks_attach_fd(s->sinks, id, socket_fd, 0);
    ok = sink = rc == 0;
  }
  if (ok) {
    try {
      XlServeClient c;
      c.rs = rsid, c.band_freq = req.band_freq;
      c.rate = (double)s->cfg.band_sampling_rate * rs.L / ((double)adm.decimation * rs.M);
      s->clients[id] = c;
    } catch (const std::bad_alloc &) {
      ok = false;
    }
  }
  if (!ok) {
    if (sink) (void)xlating_sinks_detach(s->sinks, id);
    if (rsid >= 0) (void)xl_serve_bank_remove(s, rsid);
    if (id >= 0) (void)xlating_batch_remove_client(s->eng, id);
    return xl_serve_refuse(XL_WIRE_DETAILS_INTERNAL_ERROR, response, response_len);
  }
  *client_id = id;
  *response_len = xlating_wire_build_response(XL_WIRE_STATUS_SUCCESS, (uint32_t)id, response);
  return 0;
}

extern "C" int xlating_serve_remove(xlating_serve *s, int client_id) {
  if (s == nullptr || s->clients.count(client_id) == 0) return -EINVAL;
  (void)hipSetDevice(s->device);
  (void)xl_serve_hand_over(s);  // (overlap: the leaver's last rows)
  xl_serve_forget(s, client_id);  // (nothing left to do if its sink failed just now: it is then reported as dropped)
  return 0;
}

// the final rows of ids[0 .. n): rows / lens from the engine, replaced by the bank's for the fractional clients
static int xl_serve_final_rows(xlating_serve *s, size_t n, const int *ids, const void **rows, size_t *lens, bool engine_rows_given) {
  int rc = engine_rows_given ? 0 : xlating_batch_outputs_device(s->eng, n, ids, rows, lens);
  for (size_t i = 0; rc == 0 && i < n; ++i) {
    const int rs = s->clients[ids[i]].rs;
    if (rs >= 0) rc = xl_serve_bank_output(s, rs, &rows[i], &lens[i]);
  }
  return rc;
}

// ... replaced once more by the tuner bank's for the clients the latest call rotated
static int xl_serve_tuned_rows(xlating_serve *s, size_t n, const int *ids, const void **rows, size_t *lens) {
  int rc = 0;
  for (size_t i = 0; rc == 0 && i < n; ++i) {
    const XlServeClient &c = s->clients[ids[i]];
    if (c.tn >= 0 && c.tn_fed) rc = xlating_tune_bank_output_device(s->tb, c.tn, &rows[i], &lens[i]);
  }
  return rc;
}

// everything behind the engine call: feed, pack, hand-over
static int xl_serve_run(xlating_serve *s) {
  int rc = 0;
  s->launches = s->copies = 0, s->d2h_bytes = 0;
  const size_t n = s->clients.size();
  s->ids.clear(), s->rs_ids.clear(), s->rs_rows.clear(), s->rs_lens.clear();
  for (const auto &kv : s->clients) s->ids.push_back(kv.first);
  s->rows.assign(n, nullptr), s->lens.assign(n, 0), s->bytes.assign(n, 0);
  if ((rc = xlating_batch_outputs_device(s->eng, n, s->ids.data(), s->rows.data(), s->lens.data())) != 0) return rc;
  // the object's stream behind the call that wrote the rows
  if ((rc = xlating_batch_record_event(s->eng, s->ev_call)) != 0) return rc;
  XL_TRY_RET(hipStreamWaitEvent(s->st, s->ev_call, 0));
  for (size_t i = 0; i < n; ++i) {
    const int rs = s->clients[s->ids[i]].rs;
    if (rs < 0) continue;
    s->rs_ids.push_back(rs), s->rs_rows.push_back(s->rows[i]), s->rs_lens.push_back(s->lens[i]);
  }
  if (!s->rs_ids.empty()) {  // (on s->st, behind the previous pack launch that read the bank's rows)
    if ((rc = xl_serve_bank_feed(s, s->rs_ids.size(), s->rs_ids.data(), s->rs_rows.data(), s->rs_lens.data())) != 0) return rc;
    unsigned l = 0, c = 0;
    xl_serve_bank_ops(s, &l, &c);
    s->launches += l, s->copies += c;
    if ((rc = xl_serve_final_rows(s, n, s->ids.data(), s->rows.data(), s->lens.data(), true)) != 0) return rc;
  }
  // the tuned clients' final rows through one tuner feed, behind the resampler bank's on the same stream
  s->tn_ids.clear(), s->tn_rows.clear(), s->tn_lens.clear();
  for (size_t i = 0; i < n; ++i) {
    XlServeClient &c = s->clients[s->ids[i]];
    c.tn_fed = c.tn >= 0;
    if (c.tn_fed) s->tn_ids.push_back(c.tn), s->tn_rows.push_back(s->rows[i]), s->tn_lens.push_back(s->lens[i]);
  }
  if (!s->tn_ids.empty()) {
    if ((rc = xlating_tune_bank_feed_device(s->tb, s->tn_ids.size(), s->tn_ids.data(), s->tn_rows.data(), s->tn_lens.data(), s->st)) != 0)
      return rc;
    unsigned l = 0, c = 0;
    (void)xlating_tune_bank_last_feed_ops(s->tb, &l, &c);
    s->launches += l, s->copies += c;
    if ((rc = xl_serve_tuned_rows(s, n, s->ids.data(), s->rows.data(), s->lens.data())) != 0) return rc;
  }
  // the squelch: the squelched clients' final rows through one meter launch; the host waits for its figures (in both overlap modes:
  // the decision is made on THIS call's power, before the pack), steps each policy, and a closed row is packed with length 0
  bool squelched = false;
  for (const auto &kv : s->clients) squelched = squelched || kv.second.sq_on;
  s->handing_withheld.clear();  // (scratch until the tickets change hands below: this call's withheld keys)
  if (squelched) {
    s->sq_rows.clear(), s->sq_lens.clear(), s->sq_at.clear();
    for (size_t i = 0; i < n; ++i)
      if (s->clients[s->ids[i]].sq_on) s->sq_at.push_back(i), s->sq_rows.push_back(s->rows[i]), s->sq_lens.push_back(s->lens[i]);
    if ((rc = xlating_meter_measure_device(s->mt, s->cfg.family == XL_SERVE_CS16 ? XL_METER_CS16 : XL_METER_CF32, s->sq_at.size(),
                                           s->sq_rows.data(), s->sq_lens.data(), s->st)) != 0)
      return rc;
    unsigned l = 0, c = 0;
    (void)xlating_meter_last_ops(s->mt, &l, &c);
    s->launches += l, s->copies += c;
    if ((rc = xlating_meter_wait(s->mt)) != 0) return rc;
    for (size_t k = 0; k < s->sq_at.size(); ++k) {
      const size_t i = s->sq_at[k];
      XlServeClient &cl = s->clients[s->ids[i]];
      if ((rc = xlating_meter_power(s->mt, k, &cl.sq_power, nullptr)) != 0) return rc;
      cl.sq_open = xl_serve_squelch_step(&cl.sq, cl.sq_power) != 0;
      xl_serve_squelch_log_note(&cl.sq_log, cl.produced, cl.packed, cl.sq_open);
      if (cl.sq_open) continue;
      cl.withheld += s->lens[i];
      cl.produced += s->lens[i];  // (the open rows' below, with `packed`)
      s->lens[i] = 0;
      s->handing_withheld.push_back(s->ids[i]);  // (ascending: ids is)
    }
  }
  for (size_t i = 0; i < n; ++i) s->bytes[i] = s->lens[i] * s->esz;
  // the pack with gains and levels exactly when somebody asked for either; otherwise the call is what it always was
  bool gained = s->narrow && s->levels_on;
  for (const auto &kv : s->clients) gained = gained || (s->narrow && (kv.second.gain != 0 || kv.second.agc));
  s->gains.clear();
  if (gained)
    for (size_t i = 0; i < n; ++i) s->gains.push_back(s->clients[s->ids[i]].gain);
  const int t = gained ? xlating_delivery_pack_device_cs16_gain(s->dlv, n, s->ids.data(), s->rows.data(), s->lens.data(), s->gains.data(), s->st)
                : s->narrow ? xlating_delivery_pack_device_cs16(s->dlv, n, s->ids.data(), s->rows.data(), s->lens.data(), s->st)
                            : xlating_delivery_pack_device(s->dlv, n, s->ids.data(), s->rows.data(), s->bytes.data(), s->st);
  if (t < 0) return t;
  for (size_t i = 0; i < n; ++i) s->clients[s->ids[i]].packed += s->lens[i], s->clients[s->ids[i]].produced += s->lens[i];
  unsigned l = 0, c = 0;
  (void)xlating_delivery_last_ops(s->dlv, &l, &c, &s->d2h_bytes);
  s->launches += l, s->copies += c;
  // the next engine call behind the pack launch
  XL_TRY_RET(hipEventRecord(s->ev_pack, s->st));
  s->packed = true;
  // this call's ticket becomes the pending one BEFORE the previous one is handed over: a client whose sink fails in that hand-over
  // is forgotten, and with it its id in this ticket's list
  const int prev = s->pending;
  s->handing.swap(s->pending_ids);
  s->handing_withheld.swap(s->pending_withheld);  // (this call's list becomes the pending ticket's, the previous ticket's is handed over)
  s->handing_gain.swap(s->pending_gain), s->handing_gained = s->pending_gained;
  s->pending = t;
  s->pending_ids = s->ids;
  s->pending_gain.clear(), s->pending_gained = gained;
  for (size_t i = 0; gained && i < n; ++i) s->pending_gain[s->ids[i]] = s->gains[i];
  if (prev >= 0) rc = xl_serve_deliver(s, prev);  // (overlap: the previous call's rows, whose copy ran beside this call's launches)
  if (!s->cfg.overlap) {
    const int rh = xl_serve_hand_over(s);
    rc = rc != 0 ? rc : rh;
  }
  return rc;
}

extern "C" int xlating_serve_blocks_host(xlating_serve *s, const void *input, size_t input_len, unsigned nblocks) {
  if (s == nullptr) return -EINVAL;
  if (s->clients.empty()) {  // (a client's stream starts with the block after its request)
    s->launches = s->copies = 0, s->d2h_bytes = 0;
    return 0;
  }
  XL_TRY_RET(hipSetDevice(s->device));
  // (a host call waits for the previous call before it reuses the engine's input buffers; here also for the pack launch behind it)
  if (s->packed) XL_TRY_RET(hipEventSynchronize(s->ev_pack));
  try {
    const int rc = xlating_batch_process_host_group(s->eng, input, input_len, nblocks, s->mode);
    return rc != 0 ? rc : xl_serve_run(s);
  } catch (const std::bad_alloc &) {
    return -ENOMEM;
  }
}

extern "C" int xlating_serve_blocks_device(xlating_serve *s, const void *d_input, size_t input_len, unsigned nblocks, void *hip_stream) {
  if (s == nullptr) return -EINVAL;
  if (s->clients.empty()) {
    s->launches = s->copies = 0, s->d2h_bytes = 0;
    return 0;
  }
  XL_TRY_RET(hipSetDevice(s->device));
  try {
    const int rc = xlating_batch_process_device_group_ev(s->eng, d_input, input_len, nblocks, s->mode, hip_stream,
                                                         s->packed ? s->ev_pack : nullptr, nullptr);
    return rc != 0 ? rc : xl_serve_run(s);
  } catch (const std::bad_alloc &) {
    return -ENOMEM;
  }
}

extern "C" int xlating_serve_flush(xlating_serve *s) {
  if (s == nullptr) return -EINVAL;
  (void)hipSetDevice(s->device);
  const int rc = xl_serve_hand_over(s);
  const int rf = xlating_sinks_flush(s->sinks);
  xl_serve_reap(s);
  return rc != 0 ? rc : rf;
}

extern "C" int xlating_serve_outputs_device(xlating_serve *s, size_t n, const int *client_ids, const void **d_rows, size_t *n_complex) {
  if (s == nullptr || (n > 0 && (client_ids == nullptr || d_rows == nullptr || n_complex == nullptr))) return -EINVAL;
  for (size_t i = 0; i < n; ++i)
    if (s->clients.count(client_ids[i]) == 0) return -EINVAL;
  const int rc = xl_serve_final_rows(s, n, client_ids, d_rows, n_complex, false);
  return rc != 0 ? rc : xl_serve_tuned_rows(s, n, client_ids, d_rows, n_complex);
}

extern "C" size_t xlating_serve_dropped(xlating_serve *s, int *client_ids, size_t cap) {
  if (s == nullptr || (client_ids == nullptr && cap > 0)) return 0;
  xl_serve_reap(s);
  const size_t n = std::min(cap, s->dropped.size());
  std::copy(s->dropped.begin(), s->dropped.begin() + (ptrdiff_t)n, client_ids);
  s->dropped.erase(s->dropped.begin(), s->dropped.begin() + (ptrdiff_t)n);
  return n;
}

extern "C" int xlating_serve_sink_stats(xlating_serve *s, uint64_t *bytes_written, uint64_t *blocks_dropped) {
  if (s == nullptr) return -EINVAL;
  xlating_sinks_stats(s->sinks, bytes_written, blocks_dropped);
  return 0;
}

// the client of a call that XL_SERVE_CF32_AS_CS16 alone answers, or nullptr
static XlServeClient *xl_serve_gain_client(xlating_serve *s, int client_id) {
  if (s == nullptr || !s->narrow) return nullptr;
  const auto it = s->clients.find(client_id);
  return it == s->clients.end() ? nullptr : &it->second;
}

extern "C" int xlating_serve_set_gain(xlating_serve *s, int client_id, int gain_log2) {
  XlServeClient *c = xl_serve_gain_client(s, client_id);
  if (c == nullptr || gain_log2 < XL_SERVE_GAIN_MIN || gain_log2 > XL_SERVE_GAIN_MAX) return -EINVAL;
  if (gain_log2 != c->gain) xl_serve_gain_log_add(&c->log, c->packed, gain_log2);
  c->gain = (int8_t)gain_log2, c->agc = false;
  return 0;
}

extern "C" int xlating_serve_set_auto_gain(xlating_serve *s, int client_id, int on) {
  XlServeClient *c = xl_serve_gain_client(s, client_id);
  if (c == nullptr) return -EINVAL;
  if ((on != 0) != c->agc) c->agc_state.quiet = 0;
  c->agc = on != 0;
  return 0;
}

extern "C" int xlating_serve_enable_levels(xlating_serve *s, int on) {
  if (s == nullptr || !s->narrow) return -EINVAL;
  s->levels_on = on != 0;
  return 0;
}

extern "C" int xlating_serve_levels(xlating_serve *s, size_t n, const int *client_ids, uint32_t *peak_bits, uint32_t *clipped, uint32_t *nans,
                                    int8_t *gain_log2, uint64_t *clipped_total) {
  if (s == nullptr || !s->narrow || (n > 0 && client_ids == nullptr)) return -EINVAL;
  for (size_t i = 0; i < n; ++i)
    if (s->clients.count(client_ids[i]) == 0) return -EINVAL;
  for (size_t i = 0; i < n; ++i) {
    const XlServeClient &c = s->clients[client_ids[i]];
    if (peak_bits) peak_bits[i] = c.peak_bits;
    if (clipped) clipped[i] = c.clipped;
    if (nans) nans[i] = c.nans;
    if (gain_log2) gain_log2[i] = c.level_gain;
    if (clipped_total) clipped_total[i] = c.clipped_total;
  }
  return 0;
}

extern "C" int xlating_serve_gain_log(xlating_serve *s, int client_id, size_t cap, uint64_t *first_sample, int8_t *gain_log2) {
  XlServeClient *c = xl_serve_gain_client(s, client_id);
  if (c == nullptr || (cap > 0 && (first_sample == nullptr || gain_log2 == nullptr))) return -EINVAL;
  return (int)xl_serve_gain_log_read(&c->log, cap > XL_SERVE_GAIN_LOG ? XL_SERVE_GAIN_LOG : (uint32_t)cap, first_sample, gain_log2);
}

static void xl_serve_tune_log_add(XlServeTuneLog *l, uint64_t first_sample, int64_t F, int64_t R) {
  // two changes before any sample was packed between them: the later one stands
  if (l->n > 0u && l->first_sample[(l->head + l->n - 1u) % XL_SERVE_TUNE_LOG] == first_sample) {
    const uint32_t at = (l->head + l->n - 1u) % XL_SERVE_TUNE_LOG;
    l->F[at] = F, l->R[at] = R;
    return;
  }
  if (l->n == XL_SERVE_TUNE_LOG) l->head = (l->head + 1u) % XL_SERVE_TUNE_LOG, --l->n;
  const uint32_t at = (l->head + l->n) % XL_SERVE_TUNE_LOG;
  l->first_sample[at] = first_sample, l->F[at] = F, l->R[at] = R;
  ++l->n;
}

extern "C" int xlating_serve_set_tune(xlating_serve *s, int client_id, double shift_hz, double ramp_hz_per_s) {
  if (s == nullptr || s->cfg.family == XL_SERVE_CS16) return -EINVAL;
  const auto it = s->clients.find(client_id);
  if (it == s->clients.end()) return -EINVAL;
  XlServeClient &c = it->second;
  int64_t F = 0, R = 0;
  int rc = xlating_tune_from_hz(shift_hz, ramp_hz_per_s, c.rate, &F, &R);
  if (rc != 0) return rc;
  if (c.tn < 0) {  // from here on the client stays in the bank, at (0, 0) too: its phase is continuous
    (void)hipSetDevice(s->device);
    if (s->tb == nullptr && (rc = xlating_tune_bank_create(&s->tb)) != 0) return rc;
    if ((rc = xlating_tune_bank_add(s->tb, 0u, F, R)) < 0) return rc;
    c.tn = rc;
  } else if ((rc = xlating_tune_bank_set(s->tb, c.tn, F, R)) != 0) {
    return rc;
  }
  xl_serve_tune_log_add(&c.tune_log, c.packed, F, R);
  return 0;
}

extern "C" int xlating_serve_tune_log(xlating_serve *s, int client_id, size_t cap, uint64_t *first_sample, int64_t *F, int64_t *R) {
  if (s == nullptr || s->cfg.family == XL_SERVE_CS16 || (cap > 0 && (first_sample == nullptr || F == nullptr || R == nullptr))) return -EINVAL;
  const auto it = s->clients.find(client_id);
  if (it == s->clients.end()) return -EINVAL;
  const XlServeTuneLog &l = it->second.tune_log;
  const uint32_t n = l.n < cap ? l.n : (uint32_t)cap;
  for (uint32_t i = 0; i < n; ++i) {
    const uint32_t at = (l.head + (l.n - n) + i) % XL_SERVE_TUNE_LOG;
    first_sample[i] = l.first_sample[at], F[i] = l.F[at], R[i] = l.R[at];
  }
  return (int)n;
}

extern "C" int xlating_serve_set_squelch(xlating_serve *s, int client_id, double open_power, double close_power, unsigned hang_calls) {
  if (s == nullptr || !xl_serve_squelch_valid(open_power, close_power)) return -EINVAL;
  const auto it = s->clients.find(client_id);
  if (it == s->clients.end()) return -EINVAL;
  if (s->mt == nullptr) {
    (void)hipSetDevice(s->device);
    const int rc = xlating_meter_create(&s->mt);
    if (rc != 0) return rc;
  }
  XlServeClient &c = it->second;
  if (c.sq_on) {  // new marks: the gate stays where it is
    c.sq.open_power = open_power, c.sq.close_power = close_power, c.sq.hang_calls = hang_calls, c.sq.below = 0u;
  } else {
    xl_serve_squelch_init(&c.sq, open_power, close_power, hang_calls);
    c.sq_on = true;
  }
  return 0;
}

extern "C" int xlating_serve_clear_squelch(xlating_serve *s, int client_id) {
  if (s == nullptr) return -EINVAL;
  const auto it = s->clients.find(client_id);
  if (it == s->clients.end()) return -EINVAL;
  XlServeClient &c = it->second;
  if (!c.sq_on) return 0;
  c.sq_on = false, c.sq_open = true, c.sq_power = 0.0;
  xl_serve_squelch_log_note(&c.sq_log, c.produced, c.packed, 1);
  return 0;
}

extern "C" int xlating_serve_squelch_state(xlating_serve *s, size_t n, const int *client_ids, double *power, uint8_t *open,
                                           uint64_t *withheld_samples) {
  if (s == nullptr || (n > 0 && client_ids == nullptr)) return -EINVAL;
  for (size_t i = 0; i < n; ++i)
    if (s->clients.count(client_ids[i]) == 0) return -EINVAL;
  for (size_t i = 0; i < n; ++i) {
    const XlServeClient &c = s->clients[client_ids[i]];
    if (power) power[i] = c.sq_power;
    if (open) open[i] = c.sq_open ? 1u : 0u;
    if (withheld_samples) withheld_samples[i] = c.withheld;
  }
  return 0;
}

extern "C" int xlating_serve_squelch_log(xlating_serve *s, int client_id, size_t cap, uint64_t *stream_sample, uint64_t *delivered_sample,
                                         uint8_t *open) {
  if (s == nullptr || (cap > 0 && (stream_sample == nullptr || delivered_sample == nullptr || open == nullptr))) return -EINVAL;
  const auto it = s->clients.find(client_id);
  if (it == s->clients.end()) return -EINVAL;
  return (int)xl_serve_squelch_log_read(&it->second.sq_log, cap > XL_SERVE_SQUELCH_LOG ? XL_SERVE_SQUELCH_LOG : (uint32_t)cap, stream_sample,
                                        delivered_sample, open);
}

extern "C" struct xlating_batch_t *xlating_serve_engine(xlating_serve *s) { return s ? s->eng : nullptr; }

extern "C" int xlating_serve_last_ops(const xlating_serve *s, unsigned *launches_after_engine, unsigned *copies_after_engine,
                                      uint64_t *d2h_bytes) {
  if (s == nullptr) return -EINVAL;
  if (launches_after_engine) *launches_after_engine = s->launches;
  if (copies_after_engine) *copies_after_engine = s->copies;
  if (d2h_bytes) *d2h_bytes = s->d2h_bytes;
  return 0;
}

extern "C" void xlating_serve_destroy(xlating_serve *s) {
  if (s == nullptr) return;
  (void)hipSetDevice(s->device >= 0 ? s->device : 0);
  if (s->dlv && s->sinks) (void)xl_serve_hand_over(s);
  if (s->st) (void)hipStreamSynchronize(s->st);
  if (s->eng) (void)xlating_batch_sync(s->eng);
  if (s->sinks) xlating_sinks_destroy(s->sinks);  // (flushes and closes every file)
  if (s->dlv) xlating_delivery_destroy(s->dlv);
  if (s->rb) xlating_resample_bank_destroy(s->rb);
  if (s->rq) xlating_resample_q15_bank_destroy(s->rq);
  if (s->tb) xlating_tune_bank_destroy(s->tb);
  if (s->mt) xlating_meter_destroy(s->mt);
  if (s->eng) xlating_batch_destroy(s->eng);
  if (s->ev_call) (void)hipEventDestroy(s->ev_call);
  if (s->ev_pack) (void)hipEventDestroy(s->ev_pack);
  if (s->st) (void)hipStreamDestroy(s->st);
  delete s;
}
