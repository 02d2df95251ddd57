// xl_batch.cpp -- batched fan-out engine behind include/xlating_batch.h.
//
// What the reference does per IQ block with N clients (src/tcp_server.c:257-271 -> src/dsp_worker.c:202-204 ->
// src/queue.c:87-119 -> dsp_worker.c:57-65): N memcpy's of the block and N process_* calls on N threads.
// Here: the block lives ONCE in HBM, one to three launches serve every client of this GPU, outputs stay in HBM until
// fetched.  A CALL covers G >= 1 consecutive blocks ("group"): the results are those of G successive reference calls
// (the NCO phase is renormalised at every block end, xlating.c:73) from one set of launches -- the branch spectra of
// the polyphase path are streamed once per call instead of once per block, the launches are G times bigger, and the
// NCO recurrence (a dependent chain of ~23 us per block whatever the client count) has G times more work to hide in.
//
// HBM layout (all resident across calls; a call's only per-call data is XlPos, 16 bytes of kernel arguments):
//   hist[2]      raw history (ping-pong): the last XL_HCAP samples of the stream in the INPUT format
//   block        engine-owned copy of the current blocks (host path) -- or the caller's device buffer, in place
//   taps         [tile][Tpad][ct] float2, tap i of the ct clients of a tile contiguous (one s_load_dwordx16)
//   groups[ct]   XlGroup descriptors (<= 4 tiles of one class each) incl. the class's plan-time stream record
//   nco          XlNcoClient per client; phase[XL_NTAB][slot] running NCO phases (a ring: committed, then the calls tabulated ahead)
//   phtab[XL_NTAB] [client][K_cap / 16] float2 phase tables (a ring: xl_ahead.h), out[2] outputs (ping-pong), same indexing
//
// Streaming rule (xl_grid.h): a client's outputs lie on the global grid n = k*D of ITS stream; output
// k's newest sample is stream sample k*D.  Samples older than the client (it joined mid-stream) must read as zero.
// Classes: clients sharing (D, T, stream offset mod D, valid history) share tiles of the direct kernel; their number is
// unlimited (the per-call numbers of a class are computed on the device from its record and XlPos).  In optimized mode
// all "mature" clients (every window inside their own stream) of one (D, T) form ONE polyphase class whatever their
// grid offsets (xl_polyphase.h).
//
// Streams.  A call's outputs depend on (raw history, blocks, phase table) only.  The phase table is data independent
// (float32 recurrence p <- p * incr, xlating.c:70-73), so call c+1's table is tabulated inside call c's launches (the
// "NCO role") or, up to four calls ahead, by a chain launch on a side stream, guessing that the next calls have the same shape; the
// running phases live in a ring beside the tables (committed, then ahead), so that a wrong guess is simply redone by a small launch
// of its own.  The call's own launches run on the caller's stream in stream order; the look-ahead's rules are xl_ahead.h's.
#include <errno.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <map>
#include <new>
#include <string>
#include <vector>

#include "../../include/xlating_batch.h"
#include "xl_ahead.h"
#include "xl_common.h"
#include "xl_device.h"
#include "xl_mixf_layout.h"
#include "xl_plan.h"
#include "xl_polyphase.h"
#include "xl_q15_ahead.h"
#include "xl_taps.h"
#include "xl_wide.h"
#include "xl_xop_layout.h"

#define XL_GROUP_MAX 64u  // most blocks per call

static_assert(XL_AHEAD_MAXCALLS == XL_CHAIN_MAXCALLS, "xl_ahead.h plans the chain launches of xl_device.h");

struct xlating_batch_t {
  uint32_t fs = 0;
  int fmt = 0;
  uint32_t bps = 2;
  uint32_t max_samples = 0;  // per block
  uint32_t gcap = 1;         // most blocks per call
  int device = -1;
  hipStream_t own_stream = nullptr;   // used when the caller passes no stream / host path
  hipStream_t last_stream = nullptr;  // caller stream of the latest call
  hipEvent_t dep_ev = nullptr;        // orders a call on a new stream behind the previous call's stream
  // Side-stream NCO chain (calls of several blocks): the next call's phase table is tabulated by xl_nco_chain_kernel on
  // nco_stream while this call's launches run on the caller's stream (the look-ahead state below).
  hipStream_t nco_stream = nullptr;
  // CU reservation: the chain kernel needs whole CUs (one wave per SIMD) and finds them only if nothing else is resident
  // there -- behind a launch that fills the chip its workgroups waited for the next kernel boundary (measured: chain
  // kernel 215 us alone, 262-293 us launched next to the forward / mix launches).  So nco_stream is created with a CU
  // mask of `reserve_r` CUs per XCD (mask bit b = XCD b % 8, CU b / 8 of it; tools/ubench_cumask.hip) and the engine's
  // own compute stream for side-stream calls, cs_masked, with the complement.  Callers that pass XL_STREAM_ENGINE get it.
  hipStream_t cs_masked = nullptr;
  unsigned long long *d_chain_stats = nullptr;  // tuning (XL_EXP_CHAIN_STATS): per chain workgroup cycles / ticks of the latest launch
  hipStream_t nco_masked = nullptr;  // the side stream that goes with cs_masked; nco_stream (unmasked) serves callers' own streams
  uint32_t reserve_r = 0;
  int reserve_band = -1;  // band of the reservation rule the latest plan was in (xl_chain_band; -1: none yet): hysteresis at the band edges
  uint32_t expected_clients = 0;  // option "expected_clients": the CUs are reserved for this many clients from the first plan on
  double macs_all = 0.0, macs_rest = 0.0;  // complex MACs per sample of a block: all clients' direct launches / those outside `poly`
  int nco_side = -1;          // option "nco_side_stream": 1 always, 0 never (NCO role inside the launches), -1: calls of >= 2 blocks
  bool poisoned = false;              // a launch failed mid-call: device state is undefined, every later call fails

  std::vector<Client> clients;
  int nalive = 0;
  bool dirty = true;
  // Plan buffers are recycled across re-plans (a client joining or leaving rebuilds the plan; hipMalloc / hipFree of a few
  // hundred MB took 30-90 ms per re-plan at 1024-4096 clients): live allocations with their capacities, and the ones the
  // previous plan released, waiting to be taken again.
  std::map<void *, size_t> plan_caps;
  std::vector<void *> plan_spare;
  bool want_q15 = false;  // the Q15 tap image is built from the first XL_MODE_Q15 call on
  // option "q15_kernel": 0 (default) = XL_MODE_Q15 calls run every non-wide client on the float64 launches (launches[], d_qtaps);
  // 1 = the clients the host proves eligible (xl_q15_digits.h) on one matrix-core launch (qmm), the others on float64 launches of their
  // own (launches_q15; d_qtaps is then THEIR image).  Built with the all-clients set (xl_batch_build_all_set).
  uint32_t q15_kernel = 0;
  XlQmmPlan qmm;
  XlQmmTile *d_qmm_tiles = nullptr;
  int8_t *d_qmm_image = nullptr;
  Launch launches_q15[XL_NLAUNCH];
  int planned_immature = 0;  // clients that were not mature when the plan was built (they merge once they are)
  uint32_t trel = 0;         // samples consumed since the plan was built (XlPos::trel)
  uint64_t calls_since_plan = 0;  // calls run with the current plan (their outputs live in its rows)
  uint32_t plan_maxD = 1;
  std::vector<DirectClass> classes;       // direct classes over ALL clients (native mode)
  std::vector<DirectClass> classes_rest;  // direct classes over the clients outside `poly` (optimized mode)
  Launch launches[XL_NLAUNCH];       // one per register-tile height 12, 10, 9, 8, 4, 2, 1: ALL clients (native mode).  Built on
                                     // demand (xl_batch_build_all_set): an engine that only ever runs optimized calls on the polyphase
                                     // path never pays for the all-clients tap image (4 MB and 1.4 ms per re-plan at 1024 clients)
  bool all_built = false;            // launches[] / d_taps / d_qtaps match the current plan
  int big_h = 8;                     // register-tile height of the large direct classes (chosen per plan)
  uint64_t next_uid = 1;
  std::map<uint32_t, uint32_t> free_rows;  // output rows: free extents (offset -> length) below rows_end
  uint32_t rows_end = 0;
  Launch launches_rest[XL_NLAUNCH];  // same, over classes_rest (optimized mode)
  std::vector<PolyClass> poly;       // classes on the polyphase overlap-save path in optimized mode
  float2 *d_W = nullptr;             // e^{-2 pi j n/256}
  float2 *d_phase_run = nullptr;     // running phases between the NCO slices of a call
  size_t phase_run_cap = 0;
  int poly_mode = -1;        // option "polyphase": 0 never, 1 whenever the shape allows, -1 (default) by the size rule
  bool poly_min_set = false;        // "polyphase_min_clients" was given: it holds for every class (else 32 where the mix runs on the matrix cores)
  uint32_t poly_min_clients = 32;   // XL_EXP_POLY_MIN (tuning): smallest class that takes the polyphase path under the size rule
  uint32_t poly_m = 0;        // option "polyphase_m": force the transform length (64 / 128 / 256); 0 = by the size rule
  uint32_t inv_reg = 0;       // option "inverse_kernel", M = 128 classes: 0 (default) = by the launch's size (xlp_inverse_pick: the 8-lane kernel
                              // for launches of up to 2048 tiles, the LDS transform up to 8192, the 32 x 4 cut beyond), 5 = always eight lanes per column, 16- and
                              // 8-point transforms in registers (xl_inv8.hip), 6 = always the 32 x 4 cut (xl_inv32.hip: 32-point transforms
                              // in registers, whole-line loads, 256-byte store runs), 3 = always staged in LDS on dense rows with an XOR swizzle
  uint32_t mix_kernel = 1;    // option "mix_kernel": 1 (default) = two-half float16 operands on the matrix cores where the class allows them
                              // (integer input format, D <= 112), float32 operands on the matrix cores everywhere else (cf32 input,
                              // D > 112); 3 = float32 operands for every class (the all-float32 arithmetic of the path)
  int mix_img = -1;           // option "mix_operand_image": classes on the two-half kernel of up to 8 k-blocks with an integer input format
                              // (xlp_ximg_eligible) get their shared spectra from the forward launch in the mix's operand form -- -1
                              // (default) by the size rule (xlp_ximg_pays), 1 wherever the form exists; 0 = float32 spectra, converted
                              // by every column group's staging
  uint32_t mix_pp = 0;        // XL_EXP_MIX_PP (tuning): passes per workgroup of the mix launch; 0 = the launcher's default
  uint32_t inv_skip_at = 256;  // inverse launch (4-wave workgroups, dealt per CU): one workgroup slot kept empty on the chain CUs
  uint32_t poly_exp = 0;     // XL_TUNING builds: tuning switches of the mix kernel
  uint32_t poly_slice_fi = 20000;  // NCO role inside the launches: TWO slices, forward | inverse, boundary in 1/65536 of the call (no launch
                                   // that issues matrix instructions hosts the role; the inverse launch is the longer one: 31 % | 69 %
                                   // keeps both slices inside their launches at 4096 clients with the scalar role step)
  std::vector<XlNcoClient> nco;
  // Wide clients (xl_wide.hip): outside the classes and launch sets above, one launch of their own per call, after the others.
  std::vector<XlWideClient> wide;
  XlWideClient *d_wide = nullptr;
  float2 *d_wtaps = nullptr;    // [client][Tpad] reversed taps
  double *d_wqtaps = nullptr;   // [client][T] Q15 taps as (re, im) doubles (integer input formats)
  uint32_t wide_tpad_max = 0;
  bool exp_wide = false;        // XL_EXP_WIDE (tests): every client joins as a wide client
  // option "max_window": 0 = wide clients read the XL_HCAP ring d_hist; else the largest T - 1 + D admitted, and every wide client reads
  // d_whist, a second ring of max_window raw samples rolled each call (allocated when the option is set, without clients)
  uint32_t max_window = 0;
  void *d_whist[2] = {nullptr, nullptr};
  size_t out_total = 0;
  uint64_t ncalls = 0;  // calls processed

  void *d_hist[2] = {nullptr, nullptr};
  int hcur = 0;  // d_hist[hcur] = history in front of the next call
  void *d_block = nullptr;
  void *h_block = nullptr;  // pinned staging
  float2 *d_taps = nullptr;       // tap image of the all-clients launch set
  float2 *d_taps_rest = nullptr;  // tap image of the optimized-mode launch set (the clients outside the polyphase classes)
  double *d_qtaps = nullptr;   // Q15 taps as doubles, same indexing as d_taps (XL_MODE_Q15)
  uint32_t *d_qinc = nullptr;  // per nco entry: packed Q15 phase increment
  // The Q15 family's phases and its phase look-ahead (xl_q15_ahead.h: the invariants are stated there): per slot the running Q15 phase
  // in two buffers, two phase tables, the events "the look-ahead is complete" / "the call's table is written" (created when the option
  // is first set to 1); `qahead` holds the indices into them and makes every decision.
  short2 *d_qphase[2] = {nullptr, nullptr};
  short2 *d_qphtab[2] = {nullptr, nullptr};
  hipEvent_t ev_qchain = nullptr, ev_qready = nullptr;
  XlQ15Ahead qahead = xl_q15_ahead_init();
  // option "q15_nco": 0 (default) = xl_nco_q15_batch_kernel in front of every Q15 call's launches, in place; 1 = every tabulation
  // by xl_nco_q15_ahead_kernel, and behind a Q15 call the NEXT call's table (same shape assumed: xl_grid_next) on nco_stream while
  // the call's launches run.
  uint32_t q15_nco = 0;
  bool last_q15 = false;       // the latest call produced cs16 outputs
  XlNcoClient *d_nco = nullptr;
  float2 *d_out[2] = {nullptr, nullptr};
  int ocur = 0;  // d_out[ocur] holds the latest call's outputs
  size_t out_alloc = 0;
  float2 *h_out = nullptr;
  size_t h_out_alloc = 0;
  bool fetched = false;

  // The float families' phase look-ahead (xl_ahead.h: the ring's invariants are stated there): rings of phase buffers and phase tables,
  // per table the events "its tabulation on a side stream is complete" / "its readers have been passed"; `ahead` holds the indices
  // into them and makes every decision.
  float2 *d_phase[XL_NTAB] = {};
  size_t phase_cap = 0;
  float2 *d_phtab[XL_NTAB] = {};
  hipEvent_t ev_chain[XL_NTAB] = {}, ev_done[XL_NTAB] = {};
  XlAhead ahead = xl_ahead_init();
  hipStream_t last_nco = nullptr;  // the side stream of the latest chain launch (nullptr: none since the masked pair was last re-created)
  bool exp_nofuse = false;  // XL_TUNING: keep the NCO tabulation a launch of its own

  uint32_t exp_flags = 0;  // tuning knobs
  // Wave priority of the NCO role / NCO launch (3: a pure dependent chain must not queue behind the FIR waves;
  // 1..3 measured equal for 505 taps, 3 best for short filters).
  uint32_t nco_prio = 3;
  uint32_t nco_wpw = 1;   // waves per NCO-role workgroup that carry clients
  bool riders = true;     // NCO role rides in spare waves of the FIR workgroups when the plan has some
  int riders_min_wgs = 512;
  int exp_h = 0;   // forces the tile height of the large classes (8 | 9 | 10 | 12)
#ifdef XL_TUNING
  const char *poly_trace = nullptr;  // XL_EXP_POLY_TRACE=<file>: timeline of the latest mix launch
  unsigned long long *d_ptrace = nullptr;
  const char *exp_trace = nullptr;  // XL_EXP_TRACE=<file>: dump per-wave timestamps of the latest FIR launch
  unsigned long long *d_trace = nullptr;
  size_t trace_cap = 0;
#endif
  uint32_t timing_every = 1;  // xlating_batch_timing_stride: bracket only every n-th call (an event pair costs a few us of stream time)
  int timing = 0;  // 1: bracket every call's launches; 2: also time the three polyphase launches separately
  std::vector<hipEvent_t> ev;       // pairs: start, stop of a call's launches (on the launch stream)
  std::vector<hipEvent_t> ev_ncot;  // pairs: start, stop of stand-alone NCO launches (rare)
  std::vector<hipEvent_t> ev_poly;  // quadruples: before forward, after forward, after mix, after inverse (timing == 2)
  double poly_ms[3] = {0.0, 0.0, 0.0};
  int timed_poly = 0;
  std::vector<hipEvent_t> ev_pool;  // recycled timing events (hipEventCreate per call would bound the host)
  double fir_ms = 0.0, nco_ms = 0.0;
  int timed_launches = 0, timed_nco = 0;
};

static hipError_t xl_batch_timing_event(xlating_batch *b, hipEvent_t *out) {
  if (!b->ev_pool.empty()) {
    *out = b->ev_pool.back();
    b->ev_pool.pop_back();
    return hipSuccess;
  }
  return hipEventCreate(out);
}

static void xl_batch_sync_all(xlating_batch *b) {
  (void)hipStreamSynchronize(b->last_stream);  // may be the NULL (legacy default) stream: still a real stream
  if (b->own_stream) (void)hipStreamSynchronize(b->own_stream);
  if (b->nco_stream) (void)hipStreamSynchronize(b->nco_stream);
  if (b->cs_masked) (void)hipStreamSynchronize(b->cs_masked);
  if (b->nco_masked) (void)hipStreamSynchronize(b->nco_masked);
}

// A plan buffer of at least `bytes`: the smallest spare one that fits (and is not more than twice too big), else a fresh
// allocation with 1/8 of headroom, so that the next few joins find room in place.
static hipError_t xl_plan_alloc(xlating_batch *b, void **out, size_t bytes) {
  int best = -1;
  for (size_t i = 0; i < b->plan_spare.size(); ++i) {
    const size_t cap = b->plan_caps[b->plan_spare[i]];
    if (cap >= bytes && cap <= 2 * bytes + 4096 && (best < 0 || cap < b->plan_caps[b->plan_spare[best]])) best = (int)i;
  }
  if (best >= 0) {
    *out = b->plan_spare[best];
    b->plan_spare.erase(b->plan_spare.begin() + best);
    return hipSuccess;
  }
  const size_t cap = bytes + bytes / 8 + 256;
  void *p = nullptr;
  hipError_t e = hipMalloc(&p, cap);
  if (e != hipSuccess) return e;
  b->plan_caps[p] = cap;
  *out = p;
  return hipSuccess;
}

static void xl_plan_release(xlating_batch *b, void *p) {
  if (p) b->plan_spare.push_back(p);
}

// what the finished plan did not take again goes back to the device
static void xl_plan_trim(xlating_batch *b) {
  for (void *p : b->plan_spare) {
    (void)hipFree(p);
    b->plan_caps.erase(p);
  }
  b->plan_spare.clear();
}

static void xl_poly_release(xlating_batch *b, PolyClass &pc) {
  void *dev[] = {pc.d_X, pc.d_Y, pc.d_cols, pc.d_Rh, pc.d_cscale, pc.d_segmax};
  for (void *q : dev) xl_plan_release(b, q);
  pc.d_X = pc.d_Y = nullptr;
  pc.d_segmax = nullptr;
  pc.d_cols = nullptr;
  pc.d_Rh = nullptr;
  pc.d_cscale = nullptr;
}

static void xl_release_launch_set(xlating_batch *b, Launch *set) {
  for (int i = 0; i < XL_NLAUNCH; ++i) {
    Launch &l = set[i];
    xl_plan_release(b, l.d_groups);
    l.d_groups = nullptr;
    l.groups.clear();
  }
}

// the matrix-core Q15 launch and the float64 launch set beside it (option "q15_kernel")
static void xl_release_q15_matrix(xlating_batch *b) {
  xl_release_launch_set(b, b->launches_q15);
  xl_plan_release(b, b->d_qmm_tiles);
  xl_plan_release(b, b->d_qmm_image);
  b->d_qmm_tiles = nullptr;
  b->d_qmm_image = nullptr;
  b->qmm = XlQmmPlan();
}

// Drops what a plan builds from scratch every time (launch sets, tap images, NCO records).  The polyphase classes
// survive re-plans (xl_batch_plan takes over the ones that still fit); `all` releases them too.
static void xl_batch_free_plan(xlating_batch *b, bool all) {
  xl_release_launch_set(b, b->launches);
  xl_release_launch_set(b, b->launches_rest);
  xl_release_q15_matrix(b);
  b->all_built = false;
  if (all) {
    for (PolyClass &pc : b->poly) xl_poly_release(b, pc);
    b->poly.clear();
  }
  xl_plan_release(b, b->d_taps);
  xl_plan_release(b, b->d_taps_rest);
  xl_plan_release(b, b->d_qtaps);
  xl_plan_release(b, b->d_qinc);
  xl_plan_release(b, b->d_nco);
  xl_plan_release(b, b->d_wide);
  xl_plan_release(b, b->d_wtaps);
  xl_plan_release(b, b->d_wqtaps);
  b->d_wide = nullptr;
  b->d_wtaps = nullptr;
  b->d_wqtaps = nullptr;
  b->d_taps = b->d_taps_rest = nullptr;
  b->d_qtaps = nullptr;
  b->d_qinc = nullptr;
  b->d_nco = nullptr;
}

extern "C" void xlating_batch_destroy(xlating_batch *b) {
  if (b == nullptr) return;
  if (b->device >= 0) (void)hipSetDevice(b->device);
  xl_batch_sync_all(b);
  xl_batch_free_plan(b, true);
  xl_plan_trim(b);
  void *dev[] = {b->d_hist[0], b->d_hist[1], b->d_whist[0], b->d_whist[1], b->d_block, b->d_out[0], b->d_out[1], b->d_W, b->d_phase_run, b->d_qphase[0], b->d_qphase[1], b->d_qphtab[0], b->d_qphtab[1]};
  for (void *p : dev)
    if (p) (void)hipFree(p);
  for (int i = 0; i < XL_NTAB; ++i) {
    if (b->d_phase[i]) (void)hipFree(b->d_phase[i]);
    if (b->d_phtab[i]) (void)hipFree(b->d_phtab[i]);
  }
  if (b->d_chain_stats) (void)hipFree(b->d_chain_stats);
#ifdef XL_TUNING
  if (b->d_trace) (void)hipFree(b->d_trace);
  if (b->d_ptrace) (void)hipFree(b->d_ptrace);
#endif
  if (b->h_block) (void)hipHostFree(b->h_block);
  if (b->h_out) (void)hipHostFree(b->h_out);
  for (hipEvent_t e : b->ev) (void)hipEventDestroy(e);
  for (hipEvent_t e : b->ev_ncot) (void)hipEventDestroy(e);
  for (hipEvent_t e : b->ev_poly) (void)hipEventDestroy(e);
  for (hipEvent_t e : b->ev_pool) (void)hipEventDestroy(e);
  if (b->dep_ev) (void)hipEventDestroy(b->dep_ev);
  for (hipEvent_t e : b->ev_chain)
    if (e) (void)hipEventDestroy(e);
  for (hipEvent_t e : b->ev_done)
    if (e) (void)hipEventDestroy(e);
  if (b->ev_qchain) (void)hipEventDestroy(b->ev_qchain);
  if (b->ev_qready) (void)hipEventDestroy(b->ev_qready);
  if (b->nco_stream) (void)hipStreamDestroy(b->nco_stream);
  if (b->cs_masked) (void)hipStreamDestroy(b->cs_masked);
  if (b->nco_masked) (void)hipStreamDestroy(b->nco_masked);
  if (b->own_stream) (void)hipStreamDestroy(b->own_stream);
  delete b;
}

// Tuning knobs that are not part of the documented option set: reachable through XL_EXP_* environment variables read at create
// (tests and tools force a path this way; all of them are result-neutral within the parity bars)
static int xl_batch_set_tuning(xlating_batch *b, const std::string &n, long value) {
  if (n == "polyphase_min_clients") {
    if (value < 1) return -EINVAL;
    b->poly_min_clients = (uint32_t)value;
    b->poly_min_set = true;
  } else if (n == "mix_passes_per_workgroup") {
    if (value < 0 || value > 64) return -EINVAL;
    b->mix_pp = (uint32_t)value;
  } else if (n == "riders") {
    b->riders = value != 0;
  } else if (n == "riders_min_workgroups") {
    b->riders_min_wgs = (int)value;
  } else if (n == "tile_height") {
    if (value != 0 && value != 8 && value != 9 && value != 10 && value != 12) return -EINVAL;
    b->exp_h = (int)value;
  } else if (n == "nco_calls_per_launch") {
    if (value < 1 || value > (long)XL_CHAIN_MAXCALLS) return -EINVAL;
    b->ahead.chain_calls = (int)value;
  } else if (n == "nco_slice") {  // forward | inverse boundary of the in-launch NCO role, in 1/65536 of a call
    if (value < 0 || value > 65536) return -EINVAL;
    b->poly_slice_fi = (uint32_t)value;
  } else {
    return -ENOENT;
  }
  b->dirty = true;
  return 0;
}

extern "C" int xlating_batch_set_option(xlating_batch *b, const char *name, long value) {
  if (b == nullptr || name == nullptr) return -EINVAL;
  const std::string n(name);
  if (n == "polyphase") {
    if (value < -1 || value > 1) return -EINVAL;
    b->poly_mode = (int)value;
  } else if (n == "polyphase_m") {
    if (value != 0 && value != 64 && value != 128 && value != 256) return -EINVAL;
    b->poly_m = (uint32_t)value;
  } else if (n == "inverse_kernel") {
    if (value != 0 && value != 3 && value != 5 && value != 6) return -EINVAL;
    b->inv_reg = (uint32_t)value;
  } else if (n == "mix_kernel") {
    if (value != 1 && value != 3) return -EINVAL;
    b->mix_kernel = (uint32_t)value;
  } else if (n == "mix_operand_image") {
    if (value < -1 || value > 1) return -EINVAL;
    b->mix_img = (int)value;
  } else if (n == "expected_clients") {
    if (value < 0 || value > 8192) return -EINVAL;
    b->expected_clients = (uint32_t)value;
  } else if (n == "nco_side_stream") {
    if (value < -1 || value > 1) return -EINVAL;
    b->nco_side = (int)value;
  } else if (n == "q15_kernel") {
    if (value != 0 && value != 1) return -EINVAL;
    b->q15_kernel = (uint32_t)value;
  } else if (n == "q15_nco") {
    if (value != 0 && value != 1) return -EINVAL;
    if (hipSetDevice(b->device) != hipSuccess) return -EIO;
    xl_batch_sync_all(b);  // (a look-ahead in flight writes the buffers the next tabulation writes, whatever the option then says)
    xl_q15_ahead_option_set(&b->qahead);
    if (value == 1 && b->ev_qchain == nullptr) {
      if (hipEventCreateWithFlags(&b->ev_qchain, hipEventDisableTiming) != hipSuccess ||
          hipEventCreateWithFlags(&b->ev_qready, hipEventDisableTiming) != hipSuccess) {
        (void)hipGetLastError();
        if (b->ev_qchain) (void)hipEventDestroy(b->ev_qchain);
        b->ev_qchain = b->ev_qready = nullptr;
        return -ENOMEM;
      }
    }
    b->q15_nco = (uint32_t)value;
  } else if (n == "max_window") {  // an admission setting: the ring's size is fixed while clients read it
    if (value != 0 && (value <= (long)XL_HCAP || value > (1l << 20))) return -EINVAL;
    if (b->nalive > 0) return -EBUSY;
    if (hipSetDevice(b->device) != hipSuccess) return -EIO;
    xl_batch_sync_all(b);
    for (int i = 0; i < 2; ++i) {
      if (b->d_whist[i]) (void)hipFree(b->d_whist[i]);
      b->d_whist[i] = nullptr;
    }
    b->max_window = 0;
    if (value != 0) {
      const size_t bytes = (size_t)value * b->bps;
      for (int i = 0; i < 2; ++i) {
        if (hipMalloc(&b->d_whist[i], bytes) != hipSuccess || hipMemset(b->d_whist[i], 0, bytes) != hipSuccess) {
          (void)hipGetLastError();
          for (int j = 0; j < 2; ++j) {
            if (b->d_whist[j]) (void)hipFree(b->d_whist[j]);
            b->d_whist[j] = nullptr;
          }
          return -ENOMEM;
        }
      }
      b->max_window = (uint32_t)value;
    }
  } else {
    return -ENOENT;
  }
  b->dirty = true;
  return 0;
}

extern "C" int xlating_batch_create_grouped(uint32_t sampling_freq, int input_format, uint32_t max_input_buffer_length,
                                            unsigned max_group_blocks, int device, xlating_batch **batch) {
  if (batch == nullptr || input_format < XL_FMT_CU8 || input_format > XL_FMT_CF32 || sampling_freq == 0 ||
      max_input_buffer_length < 2 || max_group_blocks < 1 || max_group_blocks > XL_GROUP_MAX ||
      (uint64_t)(max_input_buffer_length / 2) * max_group_blocks > (1u << 28))
    return -EINVAL;
  const int dev = xl_hip_select_device(device);
  if (dev < 0) {
    XL_LOG_ERR("no usable HIP device (%s); this build has no CPU arithmetic path", xlating_hip_device_info());
    return -ENODEV;
  }
  xlating_batch *b = new (std::nothrow) xlating_batch_t();
  if (b == nullptr) return -ENOMEM;
  b->fs = sampling_freq;
  b->fmt = input_format;
  b->bps = xl_bytes_per_sample(input_format);
  b->max_samples = max_input_buffer_length / 2;
  b->gcap = max_group_blocks;
  b->device = dev;
  {
    const size_t hbytes = (size_t)XL_HCAP * b->bps;
    const size_t bbytes = (size_t)b->max_samples * b->gcap * b->bps + 16;
    XL_TRY(hipSetDevice(dev));
    XL_TRY(hipStreamCreateWithFlags(&b->own_stream, hipStreamNonBlocking));
    int cus = 0;  // (nothing reads the count at present; the query stays among the runtime calls that create makes)
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    XL_TRY(hipEventCreateWithFlags(&b->dep_ev, hipEventDisableTiming));
    XL_TRY(hipStreamCreateWithFlags(&b->nco_stream, hipStreamNonBlocking));
    for (int i = 0; i < XL_NTAB; ++i) {
      XL_TRY(hipEventCreateWithFlags(&b->ev_chain[i], hipEventDisableTiming));
      XL_TRY(hipEventCreateWithFlags(&b->ev_done[i], hipEventDisableTiming));
    }
    for (int i = 0; i < 2; ++i) {
      XL_TRY(hipMalloc(&b->d_hist[i], hbytes));
      XL_TRY(hipMemsetAsync(b->d_hist[i], 0, hbytes, b->own_stream));
    }
    XL_TRY(hipMalloc(&b->d_block, bbytes));
    XL_TRY(hipHostMalloc(&b->h_block, bbytes, hipHostMallocDefault));
    XL_TRY(hipStreamSynchronize(b->own_stream));
  }
  // Result-neutral plan options may also come from the environment (tests and tools force a path this way); the
  // switches that trace launches or break results exist in -DXL_TUNING builds only (tools/experiments/).
  {
    static const struct {
      const char *env, *opt;
      bool documented;
    } knobs[] = {{"XL_EXP_POLY", "polyphase", true},          {"XL_EXP_POLY_M", "polyphase_m", true},
                 {"XL_EXP_INV", "inverse_kernel", true},      {"XL_EXP_MIX", "mix_kernel", true},
                 {"XL_EXP_MIX_IMG", "mix_operand_image", true},
                 {"XL_EXP_NCO_SIDE", "nco_side_stream", true}, {"XL_EXP_EXPECTED", "expected_clients", true},
                 {"XL_EXP_POLY_MIN", "polyphase_min_clients", false}, {"XL_EXP_MIX_PP", "mix_passes_per_workgroup", false},
                 {"XL_EXP_H", "tile_height", false},          {"XL_EXP_RIDERS", "riders", false},
                 {"XL_EXP_RIDERS_MIN", "riders_min_workgroups", false}, {"XL_EXP_CHAIN_CALLS", "nco_calls_per_launch", false},
                 {"XL_EXP_NCO_SLICE", "nco_slice", false}};
    for (const auto &k : knobs)
      if (const char *v = xl_exp_getenv(k.env)) {
        const int rc = k.documented ? xlating_batch_set_option(b, k.opt, atol(v)) : xl_batch_set_tuning(b, k.opt, atol(v));
        if (rc != 0) XL_LOG_ERR("%s=%s is not a value of \"%s\" (ignored)", k.env, v, k.opt);
      }
  }
  if (xl_exp_getenv("XL_EXP_CHAIN_STATS")) (void)hipMalloc((void **)&b->d_chain_stats, 4096 * 4 * sizeof(unsigned long long));
  if (xl_exp_getenv("XL_EXP_INVSKIP")) b->inv_skip_at = (uint32_t)atoi(xl_exp_getenv("XL_EXP_INVSKIP"));
  if (xl_exp_getenv("XL_EXP_NCOPRIO")) b->nco_prio = (uint32_t)atoi(xl_exp_getenv("XL_EXP_NCOPRIO")) & 3u;
  if (xl_exp_getenv("XL_EXP_FLATPRIO")) b->exp_flags |= 2u;
  b->exp_wide = xl_exp_getenv("XL_EXP_WIDE") != nullptr;
#ifdef XL_TUNING
  b->exp_trace = xl_exp_getenv("XL_EXP_TRACE");
  b->exp_nofuse = xl_exp_getenv("XL_EXP_NOFUSE") != nullptr;
  b->poly_trace = xl_exp_getenv("XL_EXP_POLY_TRACE");
  if (xl_exp_getenv("XL_EXP_POLY_EXP")) b->poly_exp = (uint32_t)atoi(xl_exp_getenv("XL_EXP_POLY_EXP"));
#endif
  b->last_stream = b->own_stream;
  b->dirty = true;
  *batch = b;
  return 0;
fail:
  xlating_batch_destroy(b);
  return xl_errno_of_last_hip_error();
}

extern "C" int xlating_batch_create(uint32_t sampling_freq, int input_format, uint32_t max_input_buffer_length,
                                    int device, xlating_batch **batch) {
  return xlating_batch_create_grouped(sampling_freq, input_format, max_input_buffer_length, 1, device, batch);
}

// Would the matrix-core Q15 launch (option "q15_kernel") carry this client?  The host code the plan runs, no device.
extern "C" int xlating_batch_q15_matrix_admits(uint32_t decimation, const float *taps, size_t taps_len, int32_t center_freq,
                                               uint32_t sampling_freq) {
  if (taps == nullptr || taps_len == 0 || decimation == 0 || sampling_freq == 0 || taps_len - 1 + decimation > XL_HCAP) return 0;
  if (xl_fir_needs_wide(decimation, (uint32_t)taps_len, 12u)) return 0;  // (a wide client: its own launch)
  const uint32_t T = (uint32_t)taps_len, ksteps = xl_q15mm_ksteps(T);
  if (xl_q15mm_pick_nc(decimation, ksteps) == 0u || !xl_q15mm_acc_bounded(ksteps)) return 0;
  std::vector<float> rt(2 * (size_t)xl_roundup(T, XL_TAP_UNROLL), 0.0f);
  std::vector<int16_t> rtq(2 * taps_len, 0);
  float incr[2];
  int16_t qincr[2];
  xl_prepare_taps(taps, taps_len, center_freq, sampling_freq, decimation, rt.data(), rtq.data(), incr, qincr);
  return xl_q15mm_admits_taps(rtq.data(), T);
}

extern "C" int xlating_batch_num_clients(const xlating_batch *b) { return b ? b->nalive : 0; }

extern "C" int xlating_batch_add_client(xlating_batch *b, uint32_t decimation, const float *taps, size_t taps_len,
                                        int32_t center_freq) {
  if (taps_len == 0) return -1;  // like create_frequency_xlating_filter (xlating.c:496-498)
  if (b == nullptr || taps == nullptr || decimation == 0) return -EINVAL;
  const uint32_t wcap = b->max_window ? b->max_window : XL_HCAP;  // option "max_window"
  if (taps_len - 1 + decimation > wcap) {
    XL_LOG_ERR("%zu taps at decimation %u exceed the engine's history capacity (%u samples; option \"max_window\")", taps_len, decimation, wcap);
    return -EINVAL;
  }
  const uint32_t Tpad = xl_roundup((uint32_t)taps_len, XL_TAP_UNROLL);
  // no LDS tile of the direct kernel fits (xl_wide.h; checked at the largest tap step of its tile heights), or the window reaches
  // past XL_HCAP: the wide kernel
  const bool wide = xl_fir_needs_wide(decimation, (uint32_t)taps_len, 12u) || taps_len - 1 + decimation > XL_HCAP || b->exp_wide;
  int id = -1;
  for (size_t i = 0; i < b->clients.size(); ++i)
    if (!b->clients[i].alive) {
      id = (int)i;
      break;
    }
  if (id < 0) {
    b->clients.emplace_back();
    id = (int)b->clients.size() - 1;
  }
  Client &c = b->clients[id];
  c = Client();
  c.alive = true;
  c.uid = b->next_uid++;
  c.D = decimation;
  c.T = (uint32_t)taps_len;
  c.Tpad = Tpad;
  c.wide = wide;
  c.rt.assign(2 * (size_t)Tpad, 0.0f);
  c.rtq.assign(2 * taps_len, 0);
  xl_prepare_taps(taps, taps_len, center_freq, b->fs, decimation, c.rt.data(), c.rtq.data(), c.incr, c.qincr);
  c.qmm_digits = xl_q15mm_admits_taps(c.rtq.data(), c.T) != 0;
  c.out_cap = b->gcap * (b->max_samples / decimation + 1);  // xlating.c:568 per block
  c.row_len = xl_roundup(c.out_cap, 2 * XL_PH_STRIDE);  // rows start at multiples of 2 strides: the NCO role stores pairs of
                                                        // table entries as 16 bytes
  c.out_off = xl_row_alloc(b->free_rows, b->rows_end, c.row_len);
  b->nalive++;
  b->dirty = true;
  // The running phase of a new client starts at 1 + 0j (xlating.c:543); slot = client id.  Any phase table
  // tabulated ahead is for the old client set: drop it (the committed phases are untouched by it).
  (void)hipSetDevice(b->device);
  xl_batch_sync_all(b);
  xl_ahead_drop(&b->ahead);
  xl_q15_ahead_drop(&b->qahead);
  // Every failure from here on rolls the client back (a phantom client with an undefined phase would otherwise be
  // planned and filtered on every later call, with no id in the caller's hands to remove it).
  auto rollback = [&](int code) {
    c.alive = false;
    c.rt.clear();
    xl_row_free(b->free_rows, b->rows_end, c.out_off, c.row_len);
    c.row_len = 0;
    b->nalive--;
    return code;
  };
  if ((size_t)id >= b->phase_cap) {
    // grow all running-phase buffers or none: allocate the whole new set first, swap it in only when complete
    const size_t ncap = std::max<size_t>(1024, 2 * b->clients.size());
    float2 *np[XL_NTAB] = {};
    short2 *nq[2] = {nullptr, nullptr};
    bool ok = true;
    for (int i = 0; ok && i < 2; ++i) ok = hipMalloc((void **)&nq[i], ncap * sizeof(short2)) == hipSuccess;
    for (int i = 0; ok && i < XL_NTAB; ++i) ok = hipMalloc((void **)&np[i], ncap * sizeof(float2)) == hipSuccess;
    for (int i = 0; ok && i < XL_NTAB; ++i)
      if (b->d_phase[i]) ok = hipMemcpy(np[i], b->d_phase[i], b->phase_cap * sizeof(float2), hipMemcpyDeviceToDevice) == hipSuccess;
    for (int i = 0; ok && i < 2; ++i)
      if (b->d_qphase[i]) ok = hipMemcpy(nq[i], b->d_qphase[i], b->phase_cap * sizeof(short2), hipMemcpyDeviceToDevice) == hipSuccess;
    if (!ok) {
      (void)hipGetLastError();
      for (int i = 0; i < XL_NTAB; ++i)
        if (np[i]) (void)hipFree(np[i]);
      for (int i = 0; i < 2; ++i)
        if (nq[i]) (void)hipFree(nq[i]);
      return rollback(-ENOMEM);
    }
    for (int i = 0; i < XL_NTAB; ++i) {
      if (b->d_phase[i]) (void)hipFree(b->d_phase[i]);
      b->d_phase[i] = np[i];
    }
    for (int i = 0; i < 2; ++i) {
      if (b->d_qphase[i]) (void)hipFree(b->d_qphase[i]);
      b->d_qphase[i] = nq[i];
    }
    b->phase_cap = ncap;
  }
  {
    const float2 one = make_float2(1.0f, 0.0f);
    const short2 qone = make_short2(INT16_MAX, 0);  // xlating.c:546-547
    if (hipMemcpy(b->d_phase[b->ahead.pcur] + id, &one, sizeof(one), hipMemcpyHostToDevice) != hipSuccess) return rollback(-EIO);
    if (hipMemcpy(b->d_qphase[b->qahead.cur] + id, &qone, sizeof(qone), hipMemcpyHostToDevice) != hipSuccess) return rollback(-EIO);
  }
  return id;
}

extern "C" int xlating_batch_remove_client(xlating_batch *b, int id) {
  if (b == nullptr || id < 0 || (size_t)id >= b->clients.size() || !b->clients[id].alive) return -EINVAL;
  b->clients[id].alive = false;
  b->clients[id].rt.clear();
  xl_row_free(b->free_rows, b->rows_end, b->clients[id].out_off, b->clients[id].row_len);
  b->clients[id].row_len = 0;
  b->nalive--;
  b->dirty = true;
  return 0;
}

// The settings the plan's host logic reads (xl_plan.h).
static XlPlanOpts xl_plan_opts(const xlating_batch *b) {
  XlPlanOpts o;
  o.fmt = b->fmt, o.max_samples = b->max_samples, o.gcap = b->gcap;
  o.poly_mode = b->poly_mode, o.poly_min_set = b->poly_min_set, o.poly_min_clients = b->poly_min_clients, o.poly_m = b->poly_m;
  o.mix_kernel = b->mix_kernel, o.mix_img = b->mix_img, o.riders = b->riders, o.riders_min_wgs = b->riders_min_wgs;
  o.exp_h = b->exp_h, o.nco_side = b->nco_side, o.expected_clients = b->expected_clients;
  o.q15_kernel = b->q15_kernel;
  return o;
}

// Uploads one launch set: its tap image (+ the Q15 image) and its group descriptors.
static int xl_upload_launch_set(xlating_batch *b, Launch *set, const std::vector<float> &image, float2 **d_image,
                                const std::vector<double> *imageq) {
  if (!image.empty()) {
    XL_TRY(xl_plan_alloc(b, (void **)d_image, image.size() * sizeof(float) + 256));
    XL_TRY(hipMemcpy(*d_image, image.data(), image.size() * sizeof(float), hipMemcpyHostToDevice));
  }
  if (imageq && !imageq->empty()) {
    XL_TRY(xl_plan_alloc(b, (void **)&b->d_qtaps, imageq->size() * sizeof(double) + 256));
    XL_TRY(hipMemcpy(b->d_qtaps, imageq->data(), imageq->size() * sizeof(double), hipMemcpyHostToDevice));
  }
  for (int i = 0; i < XL_NLAUNCH; ++i) {
    Launch &L = set[i];
    if (L.groups.empty()) continue;
    XL_TRY(xl_plan_alloc(b, (void **)&L.d_groups, L.groups.size() * sizeof(XlGroup)));
    XL_TRY(hipMemcpy(L.d_groups, L.groups.data(), L.groups.size() * sizeof(XlGroup), hipMemcpyHostToDevice));
  }
  return 0;
fail:
  return xl_errno_of_last_hip_error();
}

// The all-clients launch set (native and Q15 calls, optimized calls too small for the polyphase path): built when a call
// first needs it after the client set changed.  Its tap image is the one thing of a plan whose cost grows with every
// client (T x 8 bytes each, gathered tap-major on the host and uploaded).
static int xl_batch_build_all_set(xlating_batch *b) {
  if (b->all_built) return 0;
  xl_batch_sync_all(b);  // (launches in flight may still read the previous image)
  xl_q15_ahead_drop(&b->qahead);  // (... and a Q15 look-ahead the increments released below)
  xl_release_launch_set(b, b->launches);
  xl_plan_release(b, b->d_taps);
  xl_plan_release(b, b->d_qtaps);
  xl_plan_release(b, b->d_qinc);
  xl_release_q15_matrix(b);
  b->d_taps = nullptr;
  b->d_qtaps = nullptr;
  b->d_qinc = nullptr;
  std::vector<float> image;
  std::vector<double> imageq;
  const bool has_q15 = b->fmt != XL_FMT_CF32 && b->want_q15;
  const bool matrix = has_q15 && b->q15_kernel == 1u;  // (the all-clients set then carries no Q15 image: d_qtaps is launches_q15's)
  const bool all_q = has_q15 && !matrix;
  int rc = xl_build_launches(xl_plan_opts(b), b->clients, b->launches, b->classes, b->big_h, &image, all_q ? &imageq : nullptr);
  if (rc != 0) return rc;
  rc = xl_upload_launch_set(b, b->launches, image, &b->d_taps, all_q ? &imageq : nullptr);
  if (rc != 0) return rc;
  if (matrix) {
    std::vector<bool> rest_use(b->clients.size(), true);
    for (size_t i = 0; i < b->clients.size(); ++i)
      if (b->clients[i].wide) rest_use[i] = false;
    xl_build_q15mm(xl_plan_opts(b), b->clients, b->classes, &b->qmm, &rest_use);
    std::vector<DirectClass> classes_q;
    xl_direct_classes(b->clients, rest_use, &classes_q);
    std::vector<float> image_q;  // (the float taps of the set: not uploaded, Q15 calls read d_qtaps only)
    rc = xl_build_launches(xl_plan_opts(b), b->clients, b->launches_q15, classes_q, b->big_h, &image_q, &imageq);
    if (rc != 0) return rc;
    rc = xl_upload_launch_set(b, b->launches_q15, std::vector<float>(), &b->d_taps, &imageq);
    if (rc != 0) return rc;
    if (!b->qmm.tiles.empty()) {
      XL_TRY(xl_plan_alloc(b, (void **)&b->d_qmm_tiles, b->qmm.tiles.size() * sizeof(XlQmmTile)));
      XL_TRY(hipMemcpy(b->d_qmm_tiles, b->qmm.tiles.data(), b->qmm.tiles.size() * sizeof(XlQmmTile), hipMemcpyHostToDevice));
      XL_TRY(xl_plan_alloc(b, (void **)&b->d_qmm_image, b->qmm.image.size()));
      XL_TRY(hipMemcpy(b->d_qmm_image, b->qmm.image.data(), b->qmm.image.size(), hipMemcpyHostToDevice));
      std::vector<int8_t>().swap(b->qmm.image);  // (the host copy has served)
    }
  }
  if (has_q15) {
    std::vector<uint32_t> qinc;
    for (const XlNcoClient &nc : b->nco) {
      const Client &c = b->clients[nc.slot];
      qinc.push_back((uint32_t)(uint16_t)c.qincr[0] | ((uint32_t)(uint16_t)c.qincr[1] << 16));
    }
    XL_TRY(xl_plan_alloc(b, (void **)&b->d_qinc, qinc.size() * sizeof(uint32_t)));
    XL_TRY(hipMemcpy(b->d_qinc, qinc.data(), qinc.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
  }
  xl_plan_trim(b);
  b->all_built = true;
  return 0;
fail:
  return xl_errno_of_last_hip_error();
}

// Brings the device images of a polyphase class in line with its member list: columns, branch spectra of the NEW columns.
static int xl_poly_sync_device(xlating_batch *b, PolyClass &pc, const std::vector<uint32_t> &new_cols, bool fresh, uint32_t cap_samples) {
  // the images a growing class moves into: owned by nobody until they are handed to `pc` below -- a failure in between gives
  // them back (fail:)
  float2 *nY = nullptr;
  void *nRh = nullptr;
  float *ncs = nullptr;
  XlpCol *ncols = nullptr;
  // ---- capacity: column groups (Rh, Y, cols) and segments (Y, X)
  const uint32_t need_cg = ((uint32_t)pc.col_client.size() + XLP_COLS - 1) / XLP_COLS;
  const uint32_t nseg_cap = (cap_samples / pc.D + 2 + pc.V - 1) / pc.V + 1;
  const uint32_t passes = (nseg_cap + XLP_SEG - 1) / XLP_SEG;
  if (fresh || need_cg > pc.ncg_cap || nseg_cap != pc.nseg_cap) {
    // grow by an eighth (at least one group) so that the next joins find room; the old spectra move over on the device
    const uint32_t cap = fresh ? need_cg : std::max(need_cg, pc.ncg_cap + std::max(1u, pc.ncg_cap / 8u));
    // operand-form image, a group's part contiguous: the old groups are one copy, the new ones start as zeros (empty columns are
    // multiplied into sums that are never stored, but must be finite)
    const size_t per_cg = pc.mix_kind == 3u ? xlmf_rf_bytes_per_group(pc.M, pc.nkb) : xlp_rh_bytes_per_group(pc.M, pc.nkb);
    XL_TRY(xl_plan_alloc(b, &nRh, (size_t)cap * per_cg));
    const size_t old_bytes = fresh ? 0 : (size_t)pc.ncg_cap * per_cg;
    if (old_bytes) XL_TRY(hipMemcpyAsync(nRh, pc.d_Rh, old_bytes, hipMemcpyDeviceToDevice, b->own_stream));
    XL_TRY(hipMemsetAsync((char *)nRh + old_bytes, 0, (size_t)cap * per_cg - old_bytes, b->own_stream));
    XL_TRY(xl_plan_alloc(b, (void **)&ncs, (size_t)cap * XLP_COLS * sizeof(float)));
    XL_TRY(xl_plan_alloc(b, (void **)&nY, xly_bytes(cap, nseg_cap, pc.M)));
    XL_TRY(xl_plan_alloc(b, (void **)&ncols, (size_t)cap * XLP_COLS * sizeof(XlpCol)));
    XL_TRY(hipStreamSynchronize(b->own_stream));
    xl_plan_release(b, pc.d_Rh);
    xl_plan_release(b, pc.d_cscale);
    xl_plan_release(b, pc.d_Y);
    xl_plan_release(b, pc.d_cols);
    pc.d_Rh = nRh, pc.d_cscale = ncs, pc.d_Y = nY, pc.d_cols = ncols;
    nY = nullptr, nRh = nullptr, ncs = nullptr, ncols = nullptr;
    pc.ncg_cap = cap;
    if (fresh || nseg_cap != pc.nseg_cap || pc.d_X == nullptr) {
      xl_plan_release(b, pc.d_X);
      pc.d_X = nullptr;
      // (X: the padding branches and the unused segment slots of the last pass must be finite: cleared once)
      // (the operand form: groups of four branches beyond the last one the forward launch writes likewise)
      const size_t xbytes = pc.ximg ? xop_bytes(passes, pc.M, pc.nkb) : (size_t)passes * pc.Dpad * pc.M * XLP_XS * sizeof(float2);
      XL_TRY(xl_plan_alloc(b, (void **)&pc.d_X, xbytes));
      XL_TRY(hipMemsetAsync(pc.d_X, 0, xbytes, b->own_stream));
      xl_plan_release(b, pc.d_segmax);
      pc.d_segmax = nullptr;
      pc.seg_cap = passes * XLP_SEG, pc.seg_par = 0;
      if (pc.mix_kind == 1u && b->fmt == XL_FMT_CF32) {
        const size_t sbytes = 2u * (size_t)pc.seg_cap * XLP_SEGMAX_STRIDE * sizeof(uint32_t);
        XL_TRY(xl_plan_alloc(b, (void **)&pc.d_segmax, sbytes));
        XL_TRY(hipMemsetAsync(pc.d_segmax, 0, sbytes, b->own_stream));
      }
    }
    pc.nseg_cap = nseg_cap;
  }
  pc.ncg = need_cg;
  // ---- per-column records (16 bytes each: all of them, every plan)
  {
    std::vector<XlpCol> cols((size_t)pc.ncg_cap * XLP_COLS);
    for (XlpCol &cc : cols) {
      cc.out_off = 0xFFFFFFFFu;
      cc.delta = 0;
      cc.incr = make_float2(0.0f, 0.0f);
    }
    for (size_t j = 0; j < pc.col_client.size(); ++j) {
      if (pc.col_client[j] < 0) continue;
      const Client &c = b->clients[pc.col_client[j]];
      cols[j].out_off = c.out_off;
      cols[j].delta = pc.col_delta[j];
      cols[j].incr = make_float2(c.incr[0], c.incr[1]);
    }
    XL_TRY(hipMemcpy(pc.d_cols, cols.data(), cols.size() * sizeof(XlpCol), hipMemcpyHostToDevice));
    // what the two-half mix multiplies a column's sums by: 1 / (its scale * the spectra's).  (float32 operands are neither scaled nor
    // split: the table stays at 1 and nobody reads it)
    std::vector<float> cs((size_t)pc.ncg_cap * XLP_COLS, 1.0f);
    pc.col_scale.resize(pc.col_client.size(), 1.0f);
    if (pc.mix_kind == 1u) {
      for (uint32_t j : new_cols) pc.col_scale[j] = xl_poly_col_scale(b->clients[pc.col_client[j]], pc.D, pc.T);
      for (size_t j = 0; j < pc.col_client.size(); ++j) {
        if (pc.col_client[j] < 0) continue;
        cs[j] = b->fmt == XL_FMT_CF32 ? 1.0f / pc.col_scale[j] : 1.0f / (pc.col_scale[j] * XLP_H_XSCALE);  // (cf32: the segments' own scales, in the kernel)
      }
    }
    XL_TRY(hipMemcpy(pc.d_cscale, cs.data(), cs.size() * sizeof(float), hipMemcpyHostToDevice));
  }
  // ---- branch spectra of the new columns (device kernel, double arithmetic)
  if (!new_cols.empty()) {
    const size_t nn = new_cols.size();
    std::vector<float> rt(nn * pc.T * 2);  // [tap][new column]
    std::vector<uint32_t> meta(3 * nn);    // [new column]: delay, then column index, then (two-half mix) the column scale's bits
    for (size_t j = 0; j < nn; ++j) {
      const Client &c = b->clients[pc.col_client[new_cols[j]]];
      meta[j] = pc.col_delta[new_cols[j]];
      meta[nn + j] = new_cols[j];
      const float sc = pc.col_scale[new_cols[j]];
      memcpy(&meta[2 * nn + j], &sc, sizeof(float));
      for (uint32_t i = 0; i < pc.T; ++i) {
        rt[((size_t)i * nn + j) * 2] = c.rt[2 * i];
        rt[((size_t)i * nn + j) * 2 + 1] = c.rt[2 * i + 1];
      }
    }
    float2 *d_rt = nullptr;
    uint32_t *d_meta = nullptr;
    XL_TRY(xl_plan_alloc(b, (void **)&d_rt, rt.size() * sizeof(float)));
    hipError_t e = xl_plan_alloc(b, (void **)&d_meta, meta.size() * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMemcpy(d_rt, rt.data(), rt.size() * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_meta, meta.data(), meta.size() * sizeof(uint32_t), hipMemcpyHostToDevice);
    if (e == hipSuccess)
      e = pc.mix_kind == 3u
              ? xlp_launch_tables_f(d_rt, d_meta, d_meta + nn, (uint32_t)nn, pc.T, pc.D, pc.A, pc.M, pc.nkb, pc.d_Rh, b->own_stream)
              : xlp_launch_tables_h(d_rt, d_meta, d_meta + nn, reinterpret_cast<const float *>(d_meta + 2 * nn), (uint32_t)nn, pc.T,
                                    pc.D, pc.A, pc.M, pc.nkb, pc.d_Rh, b->own_stream);
    if (e == hipSuccess) e = hipStreamSynchronize(b->own_stream);
    xl_plan_release(b, d_rt);  // (scratch: spare again at once)
    xl_plan_release(b, d_meta);
    if (e != hipSuccess) {
      xl_last_hip_error = e;
      goto fail;
    }
  }
  return 0;
fail : {
  void *unowned[] = {nRh, ncs, nY, ncols};
  for (void *q : unowned) xl_plan_release(b, q);
}
  return xl_errno_of_last_hip_error();
}

// Re-creates the CU-masked stream pair for `want` reserved CUs per XCD (0: none), with every stream of the engine synchronised.
static void xl_batch_reserve_cus(xlating_batch *b, uint32_t want) {
  if (b->cs_masked) (void)hipStreamDestroy(b->cs_masked);
  if (b->nco_masked) (void)hipStreamDestroy(b->nco_masked);
  b->cs_masked = b->nco_masked = nullptr;
  b->last_nco = nullptr;
  b->reserve_r = 0;
  b->last_stream = b->own_stream;  // (everything was synchronised at the top of the plan)
  xl_ahead_reset(&b->ahead);
  if (want > 0u) {
    uint32_t chain_mask[8], main_mask[8];
    for (uint32_t wd = 0; wd < 8; ++wd) {
      chain_mask[wd] = 0u;
      for (uint32_t bit = 0; bit < 32; ++bit)
        if (wd * 32u + bit < 8u * want) chain_mask[wd] |= 1u << bit;
      main_mask[wd] = ~chain_mask[wd];
    }
    if (hipExtStreamCreateWithCUMask(&b->nco_masked, 8, chain_mask) == hipSuccess &&
        hipExtStreamCreateWithCUMask(&b->cs_masked, 8, main_mask) == hipSuccess) {
      b->reserve_r = want;
    } else {
      XL_LOG_ERR("CU-masked streams are not available (%s): the NCO chain kernel shares the chip", hipGetErrorString(hipGetLastError()));
      if (b->cs_masked) (void)hipStreamDestroy(b->cs_masked);
      if (b->nco_masked) (void)hipStreamDestroy(b->nco_masked);
      b->cs_masked = b->nco_masked = nullptr;
    }
  }
}

// Uploads the wide clients' descriptors and tap images.
static int xl_upload_wide(xlating_batch *b) {
  std::vector<float> wt;
  std::vector<double> wq;
  size_t k = 0;
  for (size_t i = 0; i < b->clients.size(); ++i) {
    const Client &c = b->clients[i];
    if (!c.alive || !c.wide) continue;
    XlWideClient &w = b->wide[k++];
    w.tap_off = (uint32_t)(wt.size() / 2);
    wt.insert(wt.end(), c.rt.begin(), c.rt.end());
    w.qtap_off = (uint32_t)(wq.size() / 2);
    if (b->fmt != XL_FMT_CF32)
      for (int16_t q : c.rtq) wq.push_back((double)q);
  }
  XL_TRY(xl_plan_alloc(b, (void **)&b->d_wide, b->wide.size() * sizeof(XlWideClient)));
  XL_TRY(hipMemcpy(b->d_wide, b->wide.data(), b->wide.size() * sizeof(XlWideClient), hipMemcpyHostToDevice));
  XL_TRY(xl_plan_alloc(b, (void **)&b->d_wtaps, wt.size() * sizeof(float)));
  XL_TRY(hipMemcpy(b->d_wtaps, wt.data(), wt.size() * sizeof(float), hipMemcpyHostToDevice));
  if (!wq.empty()) {
    XL_TRY(xl_plan_alloc(b, (void **)&b->d_wqtaps, wq.size() * sizeof(double)));
    XL_TRY(hipMemcpy(b->d_wqtaps, wq.data(), wq.size() * sizeof(double), hipMemcpyHostToDevice));
  }
  return 0;
fail:
  return xl_errno_of_last_hip_error();
}

// (Re)build the resident plan.  INCREMENTAL where it matters: clients keep their output rows, polyphase classes keep their
// columns and branch spectra (a join computes one column), the all-clients launch set is built only when a call needs it;
// rebuilt every time: the class lists, the optimized-mode direct set (the few clients outside the polyphase classes) and the
// small per-client records.
static int xl_batch_plan(xlating_batch *b) {
  // tuning: XL_EXP_PLAN_TIMING=1 prints where a re-plan spends its time
  static const bool plan_timing = xl_exp_getenv("XL_EXP_PLAN_TIMING") != nullptr;
  auto t_prev = std::chrono::steady_clock::now();
  auto lap = [&](const char *what) {
    if (!plan_timing) return;
    const auto now = std::chrono::steady_clock::now();
    fprintf(stderr, "plan: %-28s %8.3f ms\n", what, std::chrono::duration<double, std::milli>(now - t_prev).count());
    t_prev = now;
  };
  xl_batch_sync_all(b);
  lap("sync");
  xl_ahead_drop(&b->ahead);
  xl_q15_ahead_drop(&b->qahead);
  const uint32_t advanced = b->trel;  // samples since the previous plan: every plan-time stream record moves by this much
  xl_batch_free_plan(b, false);
  b->classes.clear();
  b->classes_rest.clear();
  b->nco.clear();
  b->wide.clear();
  b->wide_tpad_max = 0;
  b->trel = 0;
  b->calls_since_plan = 0;
  b->planned_immature = 0;
  b->plan_maxD = 1;
  const uint32_t cap_samples = b->max_samples * b->gcap;
  const XlPlanOpts o = xl_plan_opts(b);
  for (size_t i = 0; i < b->clients.size(); ++i) {
    Client &c = b->clients[i];
    if (!c.alive) continue;
    c.planned_mature = xl_mature(c);
    if (!c.planned_mature) b->planned_immature++;
    b->plan_maxD = std::max(b->plan_maxD, c.D);
    XlNcoClient nc;
    memset(&nc, 0, sizeof(nc));
    nc.incr = make_float2(c.incr[0], c.incr[1]);
    nc.out_off = c.out_off;
    nc.slot = (uint32_t)i;
    nc.D = c.D;
    nc.rem0 = (uint32_t)(c.consumed % c.D);
    b->nco.push_back(nc);
    if (c.wide) {
      const uint32_t hcap = b->max_window ? b->max_window : XL_HCAP;
      XlWideClient w;
      memset(&w, 0, sizeof(w));
      w.D = c.D;
      w.T = c.T;
      w.Tpad = c.Tpad;
      w.out_off = c.out_off;
      w.rem0 = nc.rem0;
      w.hv0 = (uint32_t)std::min<uint64_t>(c.consumed, hcap);
      w.incr = nc.incr;
      w.qincr = (uint32_t)(uint16_t)c.qincr[0] | ((uint32_t)(uint16_t)c.qincr[1] << 16);
      b->wide.push_back(w);
      b->wide_tpad_max = std::max(b->wide_tpad_max, c.Tpad);
    }
  }
  b->out_total = b->rows_end;

  // ---- polyphase classes (optimized mode): the classes of the previous plan that still fit are taken over, the others released
  std::vector<bool> all_use(b->clients.size(), true);
  for (size_t i = 0; i < b->clients.size(); ++i)
    if (b->clients[i].wide) all_use[i] = false;
  std::vector<bool> rest_use(all_use);
  std::vector<PolyClass> next_poly;
  std::vector<XlPolyPending> pending;
  xl_poly_form_classes(o, b->clients, b->poly, advanced, &next_poly, &pending, &rest_use);
  for (PolyClass &oc : b->poly)
    if (!oc.keep) xl_poly_release(b, oc);
  b->poly = std::move(next_poly);
  xl_direct_classes(b->clients, all_use, &b->classes);
  if (!b->poly.empty()) xl_direct_classes(b->clients, rest_use, &b->classes_rest);
  lap("classes");

  b->big_h = xl_pick_tile_height(o, b->classes);
  std::vector<float> image_rest;  // tap image of the optimized-mode launch set
  if (!b->poly.empty()) {
    int rc = xl_build_launches(o, b->clients, b->launches_rest, b->classes_rest, b->big_h, &image_rest, nullptr);
    if (rc != 0) {
      // (b->poly already holds the updated classes whose new columns have no branch spectra yet: a plan that stops here must not
      // be reused -- drop it like every other failure does)
      xl_batch_free_plan(b, true);
      b->dirty = true;
      return rc;
    }
  }
  lap("tiles + tap images (host)");

  // ---- CU reservation for the side-stream chain kernel (64 clients per workgroup = per CU, dealt round-robin to the
  // 8 XCDs): recreate the two masked streams when the number of reserved CUs changes
  {
    b->macs_all = xl_direct_macs(b->classes);
    b->macs_rest = xl_direct_macs(b->classes_rest);
    const char *exp_reserve = xl_exp_getenv("XL_EXP_RESERVE");
    const XlReserve rv = xl_reserve_want(o, b->nco.size(), b->classes_rest, b->poly, b->macs_all, b->macs_rest, b->reserve_band,
                                         xl_exp_getenv("XL_EXP_NOMASK") != nullptr, xl_exp_getenv("XL_EXP_ROUNDS1") != nullptr,
                                         exp_reserve ? atoi(exp_reserve) : -1);
    b->reserve_band = rv.band;
    if (xl_reserve_recreate(rv.want, b->reserve_r)) xl_batch_reserve_cus(b, rv.want);
  }

  lap("masked streams");
  // upload
  if (b->nco.empty()) {
    xl_plan_trim(b);
    b->dirty = false;
    return 0;
  }
  XL_TRY(xl_plan_alloc(b, (void **)&b->d_nco, b->nco.size() * sizeof(XlNcoClient)));
  XL_TRY(hipMemcpy(b->d_nco, b->nco.data(), b->nco.size() * sizeof(XlNcoClient), hipMemcpyHostToDevice));
  if (!b->wide.empty() && xl_upload_wide(b) != 0) goto fail;
  if (!b->poly.empty()) {
    if (xl_upload_launch_set(b, b->launches_rest, image_rest, &b->d_taps_rest, nullptr) != 0) goto fail;
  }
  lap("uploads (taps, groups, nco)");
  // ---- polyphase classes: images and the branch spectra of the new columns
  if (!b->poly.empty()) {
    if (b->d_W == nullptr) {
      std::vector<float> w(2 * 256);
      for (uint32_t n = 0; n < 256; ++n) {
        const double ang = -2.0 * M_PI * (double)n / 256.0;
        w[2 * n] = (float)cos(ang);
        w[2 * n + 1] = (float)sin(ang);
      }
      w[0] = 1.0f, w[1] = 0.0f;
      w[2 * 64] = 0.0f, w[2 * 64 + 1] = -1.0f;
      w[2 * 128] = -1.0f, w[2 * 128 + 1] = 0.0f;
      w[2 * 192] = 0.0f, w[2 * 192 + 1] = 1.0f;
      XL_TRY(hipMalloc((void **)&b->d_W, 256 * sizeof(float2)));
      XL_TRY(hipMemcpy(b->d_W, w.data(), 256 * sizeof(float2), hipMemcpyHostToDevice));
    }
    if (b->phase_run_cap < b->phase_cap) {
      if (b->d_phase_run) (void)hipFree(b->d_phase_run);
      b->d_phase_run = nullptr;
      b->phase_run_cap = 0;
      XL_TRY(hipMalloc((void **)&b->d_phase_run, b->phase_cap * sizeof(float2)));
      b->phase_run_cap = b->phase_cap;
    }
    for (const XlPolyPending &pd : pending)
      if (xl_poly_sync_device(b, b->poly[pd.idx], pd.new_cols, pd.fresh, cap_samples) != 0) goto fail;
  }
  lap("polyphase images + R kernel");
  if (b->out_total > b->out_alloc) {
    const size_t want = b->out_total + b->out_total / 8 + 64;  // (headroom: the next joins do not reallocate the outputs)
    for (int i = 0; i < 2; ++i) {
      if (b->d_out[i]) (void)hipFree(b->d_out[i]);
      b->d_out[i] = nullptr;
    }
    for (int i = 0; i < XL_NTAB; ++i) {
      if (b->d_phtab[i]) (void)hipFree(b->d_phtab[i]);
      b->d_phtab[i] = nullptr;
    }
    b->out_alloc = 0;
    for (int i = 0; i < 2; ++i) {
      if (b->d_qphtab[i]) (void)hipFree(b->d_qphtab[i]);
      b->d_qphtab[i] = nullptr;
    }
    for (int i = 0; i < 2; ++i) XL_TRY(hipMalloc((void **)&b->d_qphtab[i], (want / XL_PH_STRIDE + 8) * sizeof(short2)));
    for (int i = 0; i < 2; ++i) XL_TRY(hipMalloc((void **)&b->d_out[i], want * sizeof(float2)));
    for (int i = 0; i < XL_NTAB; ++i)
      XL_TRY(hipMalloc((void **)&b->d_phtab[i], (want / XL_PH_STRIDE + 8) * sizeof(float2)));  // every XL_PH_STRIDE-th phase
    b->out_alloc = want;
  }
  lap("output buffers");
  xl_plan_trim(b);
  lap("trim");
  b->dirty = false;
  return 0;
fail:
  // a half-built plan must not be used: drop it and stay dirty, the next call plans again (or fails again)
  xl_batch_free_plan(b, true);
  b->dirty = true;
  return xl_errno_of_last_hip_error();
}

// Tabulate the phases of a call as a launch of its own on stream `st`: committed phases -> the call's table + next
// phases.  Only needed when no table was tabulated ahead (first call, changed call shape, changed client set).
static hipError_t xl_batch_nco(xlating_batch *b, const XlPos pos, const XlAheadBegin &ah, hipStream_t st) {
  hipError_t e;
  hipEvent_t n0 = nullptr, n1 = nullptr;
  if (b->timing) {
    for (int i = 0; i < 2; ++i) {
      hipEvent_t ev;
      e = xl_batch_timing_event(b, &ev);
      if (e != hipSuccess) return e;
      b->ev_ncot.push_back(ev);
    }
    n0 = b->ev_ncot[b->ev_ncot.size() - 2];
    n1 = b->ev_ncot[b->ev_ncot.size() - 1];
    e = hipEventRecord(n0, st);
    if (e != hipSuccess) return e;
  }
  e = xl_launch_nco_table(b->d_nco, (uint32_t)b->nco.size(), b->d_phase[ah.phase_in], b->d_phase[ah.pcur],
                          b->d_phtab[ah.tab], pos, 0xFFFFFFFFu, b->nco_prio, st);
  if (e != hipSuccess) return e;
  return n1 ? hipEventRecord(n1, st) : hipSuccess;
}

#ifdef XL_TUNING
static hipError_t xl_dump_trace(const char *path, const unsigned long long *d, size_t n, hipStream_t s) {
  std::vector<unsigned long long> h(n);
  hipError_t e = hipStreamSynchronize(s);
  if (e != hipSuccess) return e;
  e = hipMemcpy(h.data(), d, n * sizeof(unsigned long long), hipMemcpyDeviceToHost);
  if (e != hipSuccess) return e;
  if (FILE *f = fopen(path, "wb")) {
    fwrite(h.data(), sizeof(unsigned long long), n, f);
    fclose(f);
  }
  return hipSuccess;
}
#endif

// The wide clients' outputs of a call (the most any of them produces) and their launch, behind the call's other launches on the same
// stream: windows from [ring | blocks] (the XL_HCAP ring, or the max_window ring), phases from table `phtab` (Q15: d_qphtab).
static uint32_t xl_batch_wide_maxk(const xlating_batch *b, const XlPos &pos) {
  const uint32_t hcap = b->max_window ? b->max_window : XL_HCAP;
  uint32_t k = 0;
  for (const XlWideClient &w : b->wide) k = std::max(k, xl_grid_dyn_cap(w.D, w.T, w.rem0, w.hv0, pos, hcap).K);
  return k;
}

#define XL_STREAM_ENGINE_P (reinterpret_cast<hipStream_t>((intptr_t)-1))

// What one call is given, decides and carries from stage to stage (xl_batch_run).
struct XlCall {
  // inputs
  const void *d_blocks;
  size_t S;    // samples per block
  unsigned G;  // blocks
  uint32_t N;  // S * G
  int mode;    // normalised: the x86 variants are XL_MODE_OPTIMIZED with their flags in pos.pad
  XlPos pos;
  hipStream_t s;
  hipEvent_t wait_ev, record_ev;
  // decisions
  uint32_t maxK, maxKw;  // the most outputs any client / any wide client (a launch of their own) produces in this call
  bool use_poly, side;
  int p;  // parity of this call: output buffer
  int hb, hn;
  XlAheadBegin ah;     // the phase look-ahead's decisions (xl_ahead.h): this call's table and phases, ...
  XlAheadChain chain;  // ... its chain launch (n = 0: none), ...
  bool want_done;      // ... and whether it records ev_done[ah.tab]
  // running flags
  bool rolled, nco_fused;
  bool done_attached;    // ev_done[ah.tab] rides on the call's last launch
  bool record_attached;  // the caller's record_ev rides on the last launch instead (no ev_done wanted there)
  hipEvent_t f0, f1;  // timing: around the call's launches
  bool ended;         // xl_call_begin ended the call: it returns `ret`
  int ret;
};

#define XL_STAGE static inline __attribute__((always_inline))  // stages and their helpers: one caller's body, cut for reading only
// A stage returns 0, or nonzero after a failed HIP call (xl_batch_run maps it).  xl_call_begin may also end the call on its own:
// a refusal's errno, or 0 for an engine without clients.
XL_STAGE int xl_call_end(XlCall &c, int ret) {
  c.ended = true, c.ret = ret;
  return 0;
}

// Executes the synchronisation a look-ahead decision asks for: `s` the call's stream, `ns` its side stream.
XL_STAGE hipError_t xl_ahead_run(xlating_batch *b, const XlAheadOps &l, hipStream_t s, hipStream_t ns = nullptr) {
  for (int i = 0; i < l.n; ++i) {
    const XlAheadOp o = l.op[i];
    hipStream_t st = o.stream == XL_AHEAD_S_CALL ? s : (o.stream == XL_AHEAD_S_SIDE ? ns : b->last_nco);
    hipEvent_t ev = o.ev == XL_AHEAD_EV_DEP      ? b->dep_ev
                    : o.ev == XL_AHEAD_EV_CHAIN  ? b->ev_chain[o.idx]
                    : o.ev == XL_AHEAD_EV_DONE   ? b->ev_done[o.idx]
                    : o.ev == XL_AHEAD_EV_QCHAIN ? b->ev_qchain
                                                 : b->ev_qready;
    const hipError_t e = o.op == XL_AHEAD_WAIT ? hipStreamWaitEvent(st, ev, 0) : hipEventRecord(ev, st);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

// The first reader of a table that came from the side stream waits for its chain launch, once per stream and launch.
XL_STAGE hipError_t xl_call_chain_wait(xlating_batch *b, XlCall &c) {
  if (!c.ah.chain_wait) return hipSuccess;
  const hipError_t e = hipStreamWaitEvent(c.s, b->ev_chain[c.ah.chain_ev], 0);
  if (e == hipSuccess) xl_ahead_chain_waited(&b->ahead, &c.ah, c.s);
  return e;
}

// The first launch of a call also rolls the raw history into d_hist[hn] (XlFirArgs, XlpArgs).
template <class Args>
XL_STAGE void xl_call_roll_args(const xlating_batch *b, XlCall &c, Args &a) {
  a.hist_out = b->d_hist[c.hn], a.hist_units = XL_HCAP * (b->bps / 2), a.block_units = c.N * (b->bps / 2);
  c.rolled = true;
}

// A direct launch's arguments, as far as the float and the Q15 family fill them alike.
XL_STAGE void xl_call_fir_args(const xlating_batch *b, const XlCall &c, const Launch &L, XlFirArgs &a) {
  memset(&a, 0, sizeof(a));
  a.in0 = b->d_hist[c.hb], a.n0 = XL_HCAP, a.in1 = c.d_blocks, a.n1 = c.N;
  a.fmt = b->fmt, a.pos = c.pos;
  a.groups = L.d_groups, a.ngroups = (uint32_t)L.groups.size(), a.ota = L.ota;
  const uint32_t Kl = (c.N + L.minD - 1) / L.minD;  // (an upper bound of the launch's largest output count)
  a.xtiles = (std::min(Kl, c.maxK) + L.ota - 1) / L.ota;
  a.out = b->d_out[c.p];
}

// The wide clients' launch (see xl_batch_wide_maxk); Q15 calls pass their own table and no float table.
static hipError_t xl_batch_wide_launch(xlating_batch *b, const XlCall &c, const float2 *phtab, const short2 *qphtab = nullptr) {
  XlWideArgs w;
  memset(&w, 0, sizeof(w));
  const bool big = b->max_window != 0;
  w.in0 = big ? b->d_whist[c.hb] : b->d_hist[c.hb];
  w.n0 = w.hcap = big ? b->max_window : XL_HCAP;
  w.in1 = c.d_blocks, w.n1 = c.N;
  w.fmt = b->fmt, w.pos = c.pos;
  w.clients = b->d_wide, w.nclients = (uint32_t)b->wide.size();
  w.xtiles = (c.maxKw + 63u) / 64u;
  w.parts = c.mode == XL_MODE_OPTIMIZED ? xl_wide_parts(b->wide_tpad_max) : 1u;
  w.taps = b->d_wtaps, w.phtab = phtab, w.out = b->d_out[c.p];
  w.qtaps = b->d_wqtaps, w.qphtab = qphtab;
  return xl_launch_wide(c.mode == XL_MODE_Q15 ? 2 : (c.mode == XL_MODE_OPTIMIZED ? 1 : 0), w, c.s);
}

// Everything is enqueued: commit the host-side state of the call (both families).
XL_STAGE void xl_call_commit(xlating_batch *b, const XlCall &c) {
  b->poisoned = false;
  xl_clients_commit(b->clients, (uint32_t)c.S, c.G);
  b->trel += c.N, b->ocur = c.p, b->hcur = c.hn;
  b->ncalls++, b->calls_since_plan++;
}

// XL_TUNING (XL_EXP_POLY_TRACE): arms the polyphase trace buffer in front of the one launch of a class that is traced, or
// dumps it behind that launch.  (Plain builds trace nothing and never get here.)
static hipError_t xl_ptrace(xlating_batch *b, XlpArgs &pa, hipStream_t s, bool arm) {
#ifdef XL_TUNING
  const size_t n = 32768;
  if (!arm) return pa.trace = nullptr, xl_dump_trace(b->poly_trace, b->d_ptrace, n, s);
  hipError_t e = b->d_ptrace ? hipSuccess : hipMalloc((void **)&b->d_ptrace, n * sizeof(unsigned long long));
  if (e == hipSuccess) e = hipMemsetAsync(b->d_ptrace, 0, n * sizeof(unsigned long long), s);
  if (e == hipSuccess) pa.trace = b->d_ptrace;
  return e;
#else
  return hipSuccess;
#endif
}

// Stage 1: checks, re-plan, what runs where, the stream.
XL_STAGE int xl_call_begin(xlating_batch *b, XlCall &c) {
  const size_t S = c.S;
  const unsigned G = c.G;
  if (S > b->max_samples || G < 1 || G > b->gcap ||
      (c.mode != XL_MODE_NATIVE && c.mode != XL_MODE_OPTIMIZED && c.mode != XL_MODE_Q15 && c.mode != XL_MODE_OPTIMIZED_X86 &&
       c.mode != XL_MODE_OPTIMIZED_X86_FMA) ||
      (c.mode == XL_MODE_Q15 && b->fmt == XL_FMT_CF32))
    return xl_call_end(c, -EINVAL);
  // the x86 AVX build's optimized variant = the optimized arithmetic with the phase never renormalised (xlating.c:338-339):
  // the stream position carries the flag to every kernel that walks phases (xl_grid.h: XL_POS_NORENORM)
  const uint32_t pos_flags = c.mode == XL_MODE_OPTIMIZED_X86 ? XL_POS_NORENORM
                             : (c.mode == XL_MODE_OPTIMIZED_X86_FMA ? (XL_POS_NORENORM | XL_POS_FMA_STEP) : 0u);
  if (c.mode == XL_MODE_OPTIMIZED_X86 || c.mode == XL_MODE_OPTIMIZED_X86_FMA) c.mode = XL_MODE_OPTIMIZED;
  if (c.mode == XL_MODE_Q15 && !b->want_q15) {  // (the Q15 tap image is built from the first Q15 call on)
    b->want_q15 = true;
    b->all_built = false;
  }
  if (b->poisoned) return xl_call_end(c, -EIO);
  // a client that was still inside its zero-history when the plan was built may be mature by now: it then joins
  // the class of its grid (direct kernel) / its (D, T) class (polyphase) -- re-plan
  if (!b->dirty && b->planned_immature > 0)
    for (const Client &cl : b->clients)
      if (cl.alive && !cl.planned_mature && xl_mature(cl)) {
        b->dirty = true;
        break;
      }
  if (!b->dirty && (uint64_t)b->trel + (uint64_t)S * G >= (1ull << 31)) b->dirty = true;  // re-base the classes' stream records
  if (b->dirty) {
    int rc = xl_batch_plan(b);
    if (rc != 0) return xl_call_end(c, rc);
  }
  if (G > 1 && S < b->plan_maxD && !b->nco.empty()) {
    XL_LOG_ERR("a call of %u blocks needs blocks of at least the largest decimation (%u samples); got %zu", G, b->plan_maxD, S);
    return xl_call_end(c, -EINVAL);
  }
  c.pos.trel = b->trel, c.pos.S = (uint32_t)S, c.pos.G = G, c.pos.pad = pos_flags;
  c.N = (uint32_t)(S * G);
  c.p = (int)(b->ncalls & 1), c.hb = b->hcur, c.hn = b->hcur ^ 1;
  // optimized mode: the polyphase classes leave the direct launches (tiny calls stay direct: a segment is 128 or 256
  // branch samples whatever the call holds)
  c.maxK = 0;
  for (const DirectClass &cs : b->classes) c.maxK = std::max(c.maxK, xl_grid_dyn(cs.D, cs.T, cs.rem0, cs.hv0, c.pos).K);
  c.maxKw = xl_batch_wide_maxk(b, c.pos);
  c.use_poly = c.mode == XL_MODE_OPTIMIZED && !b->poly.empty() && c.maxK >= 2 * XLP_M_MAX;
  if (!c.use_poly && !b->nco.empty()) {  // this call runs the all-clients launch set: build it if the plan has not yet
    int rc = xl_batch_build_all_set(b);
    if (rc != 0) return xl_call_end(c, rc);
  }
  c.side = xl_side_call(c.mode == XL_MODE_Q15, b->nco_side, G, c.use_poly, b->nco.size(),
                        xl_direct_is_light((c.use_poly ? b->macs_rest : b->macs_all) * (double)S), b->cs_masked != nullptr,
                        c.s == XL_STREAM_ENGINE_P);
  if (c.s == XL_STREAM_ENGINE_P) c.s = (c.side && b->cs_masked) ? b->cs_masked : b->own_stream;
  // Calls depend on each other through the engine's device state (history, phases, tables): a call on another stream than the
  // previous one is ordered behind it.  (Overlapping consecutive one-block calls through two compute streams -- round 4's
  // "pipeline_calls" -- cost this runtime more in cross-stream events than it gained: profiles/r04_one_block_pipelining.txt.)
  if (c.s != b->last_stream) {
    XL_TRY(hipEventRecord(b->dep_ev, b->last_stream));
    XL_TRY(hipStreamWaitEvent(c.s, b->dep_ev, 0));
  }
  b->last_stream = c.s;
  b->fetched = false;
  if (c.wait_ev) XL_TRY(hipStreamWaitEvent(c.s, c.wait_ev, 0));
  if (b->nco.empty()) {
    if (c.record_ev) XL_TRY(hipEventRecord(c.record_ev, c.s));
    return xl_call_end(c, 0);
  }
  return 0;
fail:
  return 1;
}

// Stage 2: the Q15 family (xlating.c:92-140, 416-447), a whole call: its own phase (never renormalised), the same raw
// history.  The float phases stay where they are; a float phase table tabulated ahead was for a call at this stream
// position and is dropped.
//
// The Q15 phase table: which buffers the call's tabulation reads and writes, whether an earlier call has made it already, which table
// the launches read, what is tabulated ahead behind the commit and every wait and record around the two are xl_q15_ahead.h's.
// The kernel that steps [phase_in] -> [phase_out] into table [tab] for a call at `pos`: this call's on its own stream after a wrong
// guess, the next call's on nco_stream.
XL_STAGE hipError_t xl_q15_tabulate(xlating_batch *b, int phase_in, int phase_out, int tab, XlPos pos, hipStream_t s) {
  return xl_launch_nco_q15_ahead(b->d_nco, b->d_qinc, (uint32_t)b->nco.size(), b->d_qphase[phase_in], b->d_qphase[phase_out], b->d_qphtab[tab],
                                 pos, b->nco_prio, s);
}

XL_STAGE int xl_call_q15(xlating_batch *b, XlCall &c) {
  hipStream_t s = c.s;
  const bool matrix = b->q15_kernel == 1u;  // the eligible clients on the matrix cores, the float64 launches over the others
  const bool ahead = b->q15_nco == 1u;
  const uint32_t ncl = (uint32_t)b->nco.size();
  XlQ15AheadBegin qa;    // the Q15 look-ahead's decisions for this call: its tabulation, its table ...
  const short2 *qphtab;  // ... which the launches below read
  XL_TRY(xl_ahead_run(b, xl_ahead_pending_wait(&b->ahead), s));
  xl_ahead_drop(&b->ahead);
  b->poisoned = true;
  qa = xl_q15_ahead_begin(&b->qahead, ahead, c.pos);
  qphtab = b->d_qphtab[qa.tab];
  XL_TRY(xl_ahead_run(b, qa.pre, s));
  if (qa.in_place)
    XL_TRY(xl_launch_nco_q15_batch(b->d_nco, b->d_qinc, ncl, b->d_qphase[qa.phase_in], b->d_qphtab[qa.tab], c.pos, s));
  else if (!qa.hit)
    XL_TRY(xl_q15_tabulate(b, qa.phase_in, qa.phase_out, qa.tab, c.pos, s));
  XL_TRY(xl_ahead_run(b, qa.post, s));
  if (matrix && !b->qmm.tiles.empty() && c.maxK > 0) {
    XlQmmArgs m;
    memset(&m, 0, sizeof(m));
    m.in0 = b->d_hist[c.hb], m.n0 = XL_HCAP, m.in1 = c.d_blocks, m.n1 = c.N;
    m.fmt = b->fmt, m.pos = c.pos;
    m.tiles = b->d_qmm_tiles, m.ntiles = (uint32_t)b->qmm.tiles.size();
    for (const XlQmmTile &t : b->qmm.tiles)
      m.xtiles = std::max(m.xtiles, (xl_grid_dyn(t.D, t.T, t.rem0, t.hv0, c.pos).K + XL_QMM_WAVES * t.nc - 1u) / (XL_QMM_WAVES * t.nc));
    m.image = b->d_qmm_image, m.qphtab = qphtab, m.out = b->d_out[c.p];
    if (m.xtiles > 0) {
      xl_call_roll_args(b, c, m);
      XL_TRY(xl_launch_q15_mm(m, b->qmm.lds, s));
    }
  }
  for (int lq = 0; lq < XL_NLAUNCH && c.maxK > 0; ++lq) {
    Launch &L = matrix ? b->launches_q15[lq] : b->launches[lq];
    if (L.groups.empty()) continue;
    XlFirArgs a;
    xl_call_fir_args(b, c, L, a);
    if (!c.rolled) xl_call_roll_args(b, c, a);
    XL_TRY(xl_launch_fir_q15_batch(L.ct, L.nw, a, b->d_qtaps, qphtab, L.lds, s));
  }
  if (!c.rolled) XL_TRY(xl_launch_update_history(b->d_hist[c.hb], c.d_blocks, XL_HCAP, c.N, b->bps, b->d_hist[c.hn], s));
  if (c.maxKw > 0) XL_TRY(xl_batch_wide_launch(b, c, nullptr, qphtab));
  if (b->d_whist[0]) XL_TRY(xl_launch_update_history(b->d_whist[c.hb], c.d_blocks, b->max_window, c.N, b->bps, b->d_whist[c.hn], s));
  if (c.record_ev) XL_TRY(hipEventRecord(c.record_ev, s));
  xl_call_commit(b, c);
  b->last_q15 = true;
  xl_q15_ahead_commit(&b->qahead, &qa);
  {
    const XlQ15AheadNext nx = xl_q15_ahead_next(&b->qahead, ahead, c.pos, b->planned_immature, ncl);
    if (nx.launch) {
      b->poisoned = true;  // (a failed look-ahead launch leaves the spare buffers and the side stream in an unknown state)
      XL_TRY(xl_ahead_run(b, nx.pre, s, b->nco_stream));
      XL_TRY(xl_q15_tabulate(b, nx.phase_in, nx.phase_out, nx.tab, nx.pos, b->nco_stream));
      XL_TRY(xl_ahead_run(b, nx.post, s, b->nco_stream));
      b->poisoned = false;
      xl_q15_ahead_launched(&b->qahead, &nx);
    }
  }
  return 0;
fail:
  return 1;
}

// Stage 3: this call's phase table: tabulated ahead by an earlier call's launches if the shape guess was right, else here.
XL_STAGE int xl_call_table(xlating_batch *b, XlCall &c) {
#ifdef XL_TUNING
  const bool nofuse = b->exp_nofuse;  // tuning: tabulate by a launch of its own before every call
#else
  const bool nofuse = false;
#endif
  c.ah = xl_ahead_begin(&b->ahead, (uint32_t)c.S, c.G, c.pos.pad, c.s, c.side, nofuse);
  if (!c.ah.hit) {
    XL_TRY(xl_ahead_run(b, c.ah.pre, c.s));
    XL_TRY(xl_batch_nco(b, c.pos, c.ah, c.s));
  }
  xl_ahead_drop(&b->ahead);  // (from here on a failure poisons the engine)
  b->poisoned = true;
  return 0;
fail:
  return 1;
}

// Stage 4 (side-stream calls without a look-ahead table left): the tables of the NEXT calls (same shape assumed), concurrently
// with the launches of the stages below, by one chain launch that starts from the phases this call commits.
XL_STAGE int xl_call_chain(xlating_batch *b, XlCall &c) {
  // (the CU-masked pair of streams goes together: a chain kernel confined to CUs that the caller's own, unmasked
  // stream keeps filling would wait for kernel boundaries)
  hipStream_t ns = (c.s == b->cs_masked && b->nco_masked) ? b->nco_masked : b->nco_stream;
  const XlAheadChain ch = xl_ahead_chain(&b->ahead, &c.ah, ns != b->last_nco);
  XlChainCalls cc;
  XL_TRY(xl_ahead_run(b, ch.pre, c.s, ns));
  b->last_nco = ns;
  memset(&cc, 0, sizeof(cc));
  cc.n = (uint32_t)ch.n;
  for (int i = 0; i < ch.n; ++i) cc.tab[i] = b->d_phtab[ch.tab[i]], cc.state_out[i] = b->d_phase[ch.phase[i]];
  XL_TRY(xl_launch_nco_chain(b->d_nco, (uint32_t)b->nco.size(), b->d_phase[ch.phase_in], cc, xl_grid_next(c.pos),
                             b->d_chain_stats, ns, b->ev_chain[ch.ev]));
  c.chain = ch;
  return 0;
fail:
  return 1;
}

// Stage 5: the launches on the caller's stream begin: window images from [d_hist[hb] | blocks], phases from the call's table ->
// d_out[p]; the first launch also rolls the raw history into d_hist[hn], and the launches of a call that fuses tabulate the ring's
// next table for the next call.  Here: the call's timing events, whether it records ev_done for its table, and the direct launches
// of its launch set.  Only the first launch of a call rolls the history and may carry the NCO role.
XL_STAGE int xl_call_direct(xlating_batch *b, XlCall &c) {
  hipStream_t s = c.s;
  Launch *const Ls = c.use_poly ? b->launches_rest : b->launches;
  if (b->timing && (c.maxK > 0 || c.maxKw > 0) && b->ncalls % b->timing_every == 0) {
    for (int i = 0; i < 2; ++i) {
      hipEvent_t ev;
      XL_TRY(xl_batch_timing_event(b, &ev));
      b->ev.push_back(ev);
    }
    c.f0 = b->ev[b->ev.size() - 2], c.f1 = b->ev[b->ev.size() - 1];
  }
  c.want_done = xl_ahead_want_done(&b->ahead, c.side, c.chain.n);
  if (c.f0) XL_TRY(hipEventRecord(c.f0, s));
  for (int lq = 0; lq < XL_NLAUNCH && c.maxK > 0; ++lq) {
    Launch &L = Ls[lq];
    if (L.groups.empty()) continue;
    XlFirArgs a;
    xl_call_fir_args(b, c, L, a);
    // wave-priority segments pay when the launch is about one round of workgroups, and cost when new
    // workgroups keep arriving (they would outrank nearly finished ones): enable up to two rounds
    const size_t wgs = (size_t)a.ngroups * a.xtiles;
    const size_t cap = 256 * std::max<size_t>(1, std::min<size_t>((160 * 1024) / std::max<size_t>(L.lds, 1), 7));
    const bool flat = (b->exp_flags & 2u) || wgs > 2 * cap;
    a.flags = (L.all_wide ? 1u : 0u) | (flat ? 2u : 0u) | 4u | ((b->nco_prio & 3u) << 4);
    a.taps = c.use_poly ? b->d_taps_rest : b->d_taps;
    a.phtab = b->d_phtab[c.ah.tab];
    if (!c.rolled) {
      xl_call_roll_args(b, c, a);
      if (c.ah.fuse) {
        a.nco_clients = b->d_nco;
        a.nco_nclients = (uint32_t)b->nco.size();
        const uint32_t slots = L.idle_waves * a.xtiles;
        const uint32_t want = (a.nco_nclients + XL_NCO_LANES - 1) / XL_NCO_LANES;
        if (b->riders && slots > 0 && (uint64_t)slots * 64u >= a.nco_nclients &&
            xl_riders_window(wgs, L.nw, L.groups[0].Tpad, L.ct, c.maxK, L.lds, b->riders_min_wgs)) {
          a.nco_slots = std::min(slots, want);
          a.nco_lanes = (a.nco_nclients + a.nco_slots - 1) / a.nco_slots;
        } else {
          a.nco_wpw = std::max<uint32_t>(1, std::min<uint32_t>(b->nco_wpw, (uint32_t)L.nw));
          a.nco_blocks = (a.nco_nclients + XL_NCO_LANES * a.nco_wpw - 1) / (XL_NCO_LANES * a.nco_wpw);
        }
        a.nco_state_in = b->d_phase[c.ah.pcur], a.nco_state_out = b->d_phase[xl_nx(c.ah.pcur)];
        a.nco_tab = b->d_phtab[xl_nx(c.ah.tab)];
        c.nco_fused = true;
      }
    }
#ifdef XL_TUNING
    size_t trace_n = 0;
    if (b->exp_trace) {
      trace_n = ((size_t)a.nco_blocks + (size_t)8 * ((a.ngroups * a.xtiles + 7) / 8)) * XL_NW_MAX * 6;
      if (trace_n > b->trace_cap) {
        if (b->d_trace) (void)hipFree(b->d_trace);
        b->d_trace = nullptr;
        XL_TRY(hipMalloc((void **)&b->d_trace, trace_n * sizeof(unsigned long long)));
        b->trace_cap = trace_n;
      }
      XL_TRY(hipMemsetAsync(b->d_trace, 0, trace_n * sizeof(unsigned long long), s));
      a.trace = b->d_trace;
    }
#endif
    XL_TRY(xl_call_chain_wait(b, c));
    XL_TRY(xl_launch_fir(L.ct, c.mode, L.nw, a, L.lds, s));
#ifdef XL_TUNING
    if (b->exp_trace) XL_TRY(xl_dump_trace(b->exp_trace, b->d_trace, trace_n, s));
#endif
  }
  return 0;
fail:
  return 1;
}

// Stage 6: one polyphase class: forward, mix and inverse launch, with the two slices of the NCO role.  `last`: the call's
// last class.
XL_STAGE int xl_call_poly_class(xlating_batch *b, XlCall &c, PolyClass &pc, bool last) {
  hipStream_t s = c.s;
  XlpArgs pa;
  memset(&pa, 0, sizeof(pa));
  if (!c.rolled) {  // the forward launch also rolls the raw history
    xl_call_roll_args(b, c, pa);
    pa.roll_blocks = 32;
  }
  pa.in0 = b->d_hist[c.hb], pa.n0 = XL_HCAP, pa.in1 = c.d_blocks, pa.n1 = c.N;
  pa.fmt = (uint32_t)b->fmt, pa.pos = c.pos;
  // the class's shared grid in this call (xl_grid.h): one D-step ahead of the reference client's output 0
  const XlDyn dref = xl_grid_dyn(pc.D, pc.T, pc.rem_ref0, pc.hv0, c.pos);
  pa.j0_ref = dref.j0;
  pa.base = dref.base - pc.D;
  pa.Kq = xl_merge_points(pc.D, c.pos);
  pa.zero_below = dref.zero_below;  // (0 for mature members: nothing below their join points is weighted)
  pa.D = pc.D, pa.Dpad = pc.Dpad, pa.T = pc.T, pa.A = pc.A, pa.V = pc.V, pa.M = pc.M;
  pa.nseg = (pa.Kq + pc.V - 1) / pc.V;
  pa.nseg_cap = pc.nseg_cap;
  if (pa.nseg > pa.nseg_cap) {
    XL_LOG_ERR("internal: %u segments exceed the plan's capacity %u", pa.nseg, pa.nseg_cap);
    return 1;  // (the engine is poisoned: -EIO)
  }
  pa.ncg = pc.ncg, pa.mix_kind = pc.mix_kind, pa.nkb = pc.nkb;
  pa.exp = b->poly_exp, pa.inv_reg = b->inv_reg, pa.mix_pp = b->mix_pp;
  pa.Rh = pc.d_Rh, pa.cscale = pc.d_cscale;
  pa.segmax = pc.d_segmax, pa.seg_par = pc.seg_par, pa.seg_cap = pc.seg_cap;
  pc.seg_par ^= 1u;  // (a failed call leaves stale maxima behind at worst: a smaller scale than necessary, never a wrong one)
  pa.W = b->d_W, pa.X = pc.d_X, pa.ximg = pc.ximg ? 1u : 0u, pa.Y = pc.d_Y, pa.cols = pc.d_cols;
  pa.phtab = b->d_phtab[c.ah.tab], pa.out = b->d_out[c.p];
  // the NEXT call's phase recurrence rides in these launches (a direct launch above carries all of it if there is
  // one): TWO slices, forward | inverse -- never the mix launch: no launch that issues matrix instructions hosts the role
  // 
  const bool carry = c.ah.fuse && !c.nco_fused;
  const uint32_t sl1 = std::min(b->poly_slice_fi, 60000u);
  if (carry) {
    pa.nco_clients = b->d_nco, pa.nco_nclients = (uint32_t)b->nco.size();
    pa.nco_blocks = (pa.nco_nclients + XL_NCO_LANES - 1) / XL_NCO_LANES;
    pa.nco_tab = b->d_phtab[xl_nx(c.ah.tab)], pa.nco_prio = b->nco_prio;
    pa.nco_k0 = 0, pa.nco_k1 = sl1;
    pa.nco_state_src = b->d_phase[c.ah.pcur], pa.nco_state_dst = b->d_phase_run;
  }
  // the call's last launch carries the "table has been read" event the side stream waits for
  const bool last_launch = c.side && c.rolled && last && c.maxKw == 0;  // (a wide launch follows: it reads the table too)
  // XL_EXP_POLY_TRACE: timeline of the mix launch (2: work waves' span + each NCO wave), of the forward launch instead (1:
  // XL_EXP_POLY_TRACE_FWD) or of the inverse launch instead (3: XL_EXP_POLY_TRACE_INV)
#ifdef XL_TUNING
  const int traced = !b->poly_trace ? 0 : (xl_exp_getenv("XL_EXP_POLY_TRACE_FWD") ? 1 : (xl_exp_getenv("XL_EXP_POLY_TRACE_INV") ? 3 : 2));
#else
  const int traced = 0;
#endif
  hipEvent_t pe[4] = {nullptr, nullptr, nullptr, nullptr};
  if (b->timing == 2) {
    for (int i = 0; i < 4; ++i) {
      XL_TRY(xl_batch_timing_event(b, &pe[i]));
      b->ev_poly.push_back(pe[i]);
    }
    XL_TRY(hipEventRecord(pe[0], s));
  }
  if (traced == 1) XL_TRY(xl_ptrace(b, pa, s, true));
  XL_TRY(xlp_launch_forward(pa, s));
  if (traced == 1) XL_TRY(xl_ptrace(b, pa, s, false));
  if (pe[1]) XL_TRY(hipEventRecord(pe[1], s));
  pa.roll_blocks = 0;
  pa.nco_blocks = 0;  // (no role in the mix launch)
  if (traced == 2) XL_TRY(xl_ptrace(b, pa, s, true));
  XL_TRY(xlp_launch_mix(pa, s));
  pa.nco_skip = 0;
  if (traced == 2) XL_TRY(xl_ptrace(b, pa, s, false));
  if (pe[2]) XL_TRY(hipEventRecord(pe[2], s));
  if (carry) {
    pa.nco_tab = b->d_phtab[xl_nx(c.ah.tab)];
    pa.nco_blocks = (pa.nco_nclients + XL_NCO_LANES - 1) / XL_NCO_LANES;
    pa.nco_k0 = sl1, pa.nco_k1 = 65536;
    pa.nco_state_src = b->d_phase_run, pa.nco_state_dst = b->d_phase[xl_nx(c.ah.pcur)];
    if (b->inv_skip_at > 0) pa.nco_skip_at = b->inv_skip_at, pa.nco_skip = pa.nco_blocks;
    c.nco_fused = true;
  }
  if (traced == 3) XL_TRY(xl_ptrace(b, pa, s, true));
  XL_TRY(xl_call_chain_wait(b, c));  // (the forward and mix launches do not read the table)
  {
    const bool attach = last_launch && traced != 3;  // (a traced inverse launch carries no event)
    XL_TRY(xlp_launch_inverse(pa, s, attach ? (c.want_done ? b->ev_done[c.ah.tab] : c.record_ev) : nullptr));
    pc.last_inv = (int)xlp_inverse_pick(pa.M, pa.inv_reg, pa.nseg * pa.ncg * 4u);
    c.done_attached = attach && c.want_done;
    c.record_attached = attach && !c.want_done && c.record_ev != nullptr;
  }
  if (traced == 3) XL_TRY(xl_ptrace(b, pa, s, false));
  if (pe[3]) XL_TRY(hipEventRecord(pe[3], s));
  ++pc.calls;
  return 0;
fail:
  return 1;
}

// Stage 7: the wide clients, behind the launches above on the same stream, and the history rolls that no launch carried.
XL_STAGE int xl_call_wide_and_rolls(xlating_batch *b, XlCall &c) {
  hipStream_t s = c.s;
  if (c.maxKw > 0) {
    XL_TRY(xl_call_chain_wait(b, c));
    XL_TRY(xl_batch_wide_launch(b, c, b->d_phtab[c.ah.tab]));
  }
  if (c.f1) XL_TRY(hipEventRecord(c.f1, s));
  if (!c.rolled)  // no client produced output in this call (tiny block): roll the history on its own
    XL_TRY(xl_launch_update_history(b->d_hist[c.hb], c.d_blocks, XL_HCAP, c.N, b->bps, b->d_hist[c.hn], s));
  if (b->d_whist[0]) XL_TRY(xl_launch_update_history(b->d_whist[c.hb], c.d_blocks, b->max_window, c.N, b->bps, b->d_whist[c.hn], s));
  return 0;
fail:
  return 1;
}

// Stage 8: the "table has been read" event, the caller's event, the host commit and the look-ahead handed to the next call.
XL_STAGE int xl_call_finish(xlating_batch *b, XlCall &c) {
  // the call's table has been read by everything enqueued so far
  if (c.want_done && !c.done_attached) XL_TRY(hipEventRecord(b->ev_done[c.ah.tab], c.s));
  if (c.record_ev && !c.record_attached) XL_TRY(hipEventRecord(c.record_ev, c.s));
  xl_ahead_finish(&b->ahead, &c.ah, b->ncalls + 1, c.side, c.want_done, c.chain.n, c.nco_fused, (uint32_t)c.S, c.G, c.pos.pad);
  xl_call_commit(b, c);
  return 0;
fail:
  return 1;
}

// One call: G blocks of S samples each, contiguous at d_blocks.  s_in: the caller's stream, or XL_STREAM_ENGINE_P = the
// engine's own compute stream (the CU-masked one for calls whose NCO chain runs on the side stream).  wait_ev / record_ev:
// optional events of the caller, waited for before / recorded after the call's work on that stream.
static int xl_batch_run(xlating_batch *b, const void *d_blocks, size_t input_len, unsigned G, int mode, hipStream_t s_in,
                        hipEvent_t wait_ev = nullptr, hipEvent_t record_ev = nullptr) {
  XlCall c;
  memset(&c, 0, sizeof(c));
  c.d_blocks = d_blocks, c.S = input_len / 2, c.G = G, c.mode = mode;
  c.s = s_in, c.wait_ev = wait_ev, c.record_ev = record_ev;
  if (xl_call_begin(b, c)) goto fail;
  if (c.ended) return c.ret;
  if (c.mode == XL_MODE_Q15) {
    if (xl_call_q15(b, c)) goto fail;
    return 0;
  }
  b->last_q15 = false;
  if (xl_call_table(b, c)) goto fail;
  if (c.side && c.ah.spec_left == 0 && xl_call_chain(b, c)) goto fail;
  if (xl_call_direct(b, c)) goto fail;
  if (c.maxK > 0 && c.use_poly)
    for (PolyClass &pc : b->poly)
      if (xl_call_poly_class(b, c, pc, &pc == &b->poly.back())) goto fail;
  if (xl_call_wide_and_rolls(b, c)) goto fail;
  if (xl_call_finish(b, c)) goto fail;
  return 0;
fail:
  return b->poisoned ? -EIO : xl_errno_of_last_hip_error();
}

// one direct launch in describe: its tile height and groups; " lanes<ota>" when it runs fewer than 64 outputs per wave (a window image
// of 64 exceeds the LDS) and " reads8" when it reads single samples (a group of odd decimation: no 16-byte LDS reads)
static std::string xl_describe_launch(const Launch &L) {
  std::string d = " h" + std::to_string(L.ct) + " x " + std::to_string(L.groups.size()) + " groups";
  if (L.ota < 64u) d += " lanes" + std::to_string(L.ota);
  if (!L.all_wide) d += " reads8";
  return d;
}

extern "C" int xlating_batch_describe(xlating_batch *b, char *buf, size_t n) {
  if (b == nullptr || buf == nullptr || n == 0) return -EINVAL;
  if (hipSetDevice(b->device) != hipSuccess) return -EIO;
  // A re-plan reassigns every client's output row and may reallocate the output buffers, while the latest call's outputs
  // stay valid "until the next process call" (xlating_batch.h): with calls behind it a dirty engine reports the plan
  // those calls ran with and says that a new one is pending; before the first call after a plan nothing can be lost.
  const bool pending = b->dirty && b->calls_since_plan > 0;
  if (b->dirty && !pending) {
    int rc = xl_batch_plan(b);
    if (rc != 0) return rc;
  }
  std::string d = "clients " + std::to_string(b->nalive) + " classes " + std::to_string(b->classes.size()) + " | direct:";
  if (!b->all_built && !b->nco.empty()) d += " (built by the first call that runs all clients on the direct kernel)";
  for (const Launch &L : b->launches)
    if (!L.groups.empty()) d += xl_describe_launch(L);
  d += " | polyphase:";
  if (b->poly.empty()) d += " none";
  for (size_t k = 0; k < b->poly.size(); ++k) {
    const PolyClass &pc = b->poly[k];
    d += " cls" + std::to_string(k) + " D" + std::to_string(pc.D) + " T" + std::to_string(pc.T) + " cols" +
         std::to_string(pc.members.size()) + " V" + std::to_string(pc.V) + " M" + std::to_string(pc.M);
    if (pc.dmax) d += " offsets<=" + std::to_string(pc.dmax);
    d += pc.mix_kind == 3u ? " mix=mf32" : (pc.ximg ? " mix=mfma/img" : " mix=mfma");
    if (pc.M == 128u) {
      // (before the class's first launch: what the size rule picks for a call of the plan's full size -- gcap blocks of max_samples)
      const uint32_t kq_full = (uint32_t)(((uint64_t)b->max_samples * b->gcap + pc.D - 1u) / pc.D) + 1u;
      const int k = b->inv_reg ? (int)b->inv_reg
                               : (pc.last_inv >= 0 ? pc.last_inv : (int)xlp_inverse_pick(pc.M, 0u, ((kq_full + pc.V - 1u) / pc.V) * pc.ncg * 4u));
      d += k == 6 ? " inv=cut32" : (k == 5 ? " inv=lanes8" : (k == 3 ? " inv=lds" : " inv=auto"));
    }
    d += " calls=" + std::to_string(pc.calls);  // (calls that took the class's polyphase launches, not the direct fall-back)
  }
  if (!b->poly.empty()) {
    d += " | optimized-mode direct:";
    bool any = false;
    for (const Launch &L : b->launches_rest)
      if (!L.groups.empty()) {
        d += xl_describe_launch(L);
        any = true;
      }
    if (!any) d += " none";
  }
  if (!b->wide.empty()) {
    d += " | wide: " + std::to_string(b->wide.size()) + " clients";
    if (b->max_window) d += " window<=" + std::to_string(b->max_window);
  }
  if (b->q15_kernel == 1u && b->fmt != XL_FMT_CF32) {
    d += " | q15 matrix:";
    if (!b->all_built || !b->want_q15) {
      d += " (built by the first Q15 call)";
    } else {
      d += " " + std::to_string(b->qmm.nclients) + " clients x " + std::to_string(b->qmm.tiles.size()) + " tiles, float64: " +
           std::to_string(b->qmm.fb_digits + b->qmm.fb_window) + " clients (digits " + std::to_string(b->qmm.fb_digits) + ", window " +
           std::to_string(b->qmm.fb_window) + ")";
    }
  }
  if (b->q15_nco == 1u)
    d += " | q15 nco: ahead, " + std::to_string(b->qahead.used) + " used, " + std::to_string(b->qahead.dropped) + " dropped";
  if (b->exp_flags & 2u) d += " | tap loop: flat priority";  // (XL_EXP_FLATPRIO: every direct launch takes the one-piece tap loop)
  if (b->reserve_r) d += " | side kernel: " + std::to_string(8u * b->reserve_r) + " CUs reserved";
  if (pending) d += " | re-plan pending (client set or options changed: the next process call plans again)";
  const size_t len = std::min(d.size(), n - 1);
  memcpy(buf, d.data(), len);
  buf[len] = 0;
  return (int)len;
}

extern "C" int xlating_batch_process_device_group_ev(xlating_batch *b, const void *d_input, size_t input_len,
                                                     unsigned nblocks, int mode, void *hip_stream, void *wait_event,
                                                     void *record_event) {
  if (b == nullptr || (d_input == nullptr && input_len > 0)) return -EINVAL;
  if (hipSetDevice(b->device) != hipSuccess) return -EIO;
  // NULL is HIP's legacy default stream (what torch.cuda.current_stream().cuda_stream is by default): pass it through
  hipStream_t s = reinterpret_cast<hipStream_t>(hip_stream);
  return xl_batch_run(b, d_input, input_len, nblocks, mode, s, reinterpret_cast<hipEvent_t>(wait_event),
                      reinterpret_cast<hipEvent_t>(record_event));
}

extern "C" int xlating_batch_process_device_group(xlating_batch *b, const void *d_input, size_t input_len,
                                                  unsigned nblocks, int mode, void *hip_stream) {
  return xlating_batch_process_device_group_ev(b, d_input, input_len, nblocks, mode, hip_stream, nullptr, nullptr);
}

extern "C" int xlating_batch_process_device(xlating_batch *b, const void *d_input, size_t input_len, int mode,
                                            void *hip_stream) {
  return xlating_batch_process_device_group(b, d_input, input_len, 1, mode, hip_stream);
}

extern "C" int xlating_batch_process_host_group(xlating_batch *b, const void *input, size_t input_len, unsigned nblocks,
                                                int mode) {
  if (b == nullptr || (input == nullptr && input_len > 0)) return -EINVAL;
  const size_t S = input_len / 2;
  if (S > b->max_samples || nblocks < 1 || nblocks > b->gcap) return -EINVAL;
  if (hipSetDevice(b->device) != hipSuccess) return -EIO;
  hipStream_t s = b->own_stream;
  // the pinned staging buffer and the device block buffer are reused: wait until the previous call is consumed
  xl_batch_sync_all(b);
  const size_t bytes = S * nblocks * b->bps;
  if (bytes) {
    memcpy(b->h_block, input, bytes);
    if (hipMemcpyAsync(b->d_block, b->h_block, bytes, hipMemcpyHostToDevice, s) != hipSuccess) return -EIO;
  }
  return xl_batch_run(b, b->d_block, input_len, nblocks, mode, s);
}

extern "C" int xlating_batch_process_host(xlating_batch *b, const void *input, size_t input_len, int mode) {
  return xlating_batch_process_host_group(b, input, input_len, 1, mode);
}

extern "C" size_t xlating_batch_output_len(const xlating_batch *b, int id) {
  if (b == nullptr || id < 0 || (size_t)id >= b->clients.size() || !b->clients[id].alive) return 0;
  return b->clients[id].last_K;
}

extern "C" size_t xlating_batch_output_len_block(const xlating_batch *b, int id, unsigned block) {
  if (b == nullptr || id < 0 || (size_t)id >= b->clients.size() || !b->clients[id].alive ||
      block >= b->clients[id].last_Kg.size())
    return 0;
  return b->clients[id].last_Kg[block];
}

extern "C" int xlating_batch_sync(xlating_batch *b) {
  if (b == nullptr) return -EINVAL;
  if (hipSetDevice(b->device) != hipSuccess) return -EIO;
  if (hipStreamSynchronize(b->last_stream) != hipSuccess) return -EIO;
  // (a Q15 phase table being tabulated a call ahead, option "q15_nco": enqueued work of the engine like the call's own)
  if (xl_q15_ahead_pending(&b->qahead) && hipStreamSynchronize(b->nco_stream) != hipSuccess) return -EIO;
  return 0;
}

extern "C" int xlating_batch_query(xlating_batch *b) {
  if (b == nullptr) return -EINVAL;
  if (hipSetDevice(b->device) != hipSuccess) return -EIO;
  const hipError_t e = hipStreamQuery(b->last_stream);
  if (e == hipErrorNotReady) {
    (void)hipGetLastError();  // (not an error: clear the sticky code)
    return 0;
  }
  return e == hipSuccess ? 1 : -EIO;
}

extern "C" int xlating_batch_record_event(xlating_batch *b, void *hip_event) {
  if (b == nullptr || hip_event == nullptr) return -EINVAL;
  if (hipSetDevice(b->device) != hipSuccess) return -EIO;
  hipEvent_t ev = reinterpret_cast<hipEvent_t>(hip_event);
  return hipEventRecord(ev, b->last_stream) == hipSuccess ? 0 : -EIO;
}

extern "C" int xlating_batch_fetch(xlating_batch *b) {
  if (b == nullptr) return -EINVAL;
  int rc = xlating_batch_sync(b);
  if (rc != 0) return rc;
  if (b->out_total == 0 || b->d_out[b->ocur] == nullptr) {
    b->fetched = true;
    return 0;
  }
  // (clients that joined since the latest call have rows -- assigned at add_client -- that may lie beyond what the device images hold:
  // those grow with the next plan.  Only what exists is copied; such a client has no outputs yet.)
  const size_t n = std::min(b->out_total, b->out_alloc);
  if (n > b->h_out_alloc) {
    if (b->h_out) (void)hipHostFree(b->h_out);
    b->h_out = nullptr;
    b->h_out_alloc = 0;
    if (hipHostMalloc((void **)&b->h_out, n * sizeof(float2), hipHostMallocDefault) != hipSuccess)
      return -ENOMEM;
    b->h_out_alloc = n;
  }
  if (hipMemcpyAsync(b->h_out, b->d_out[b->ocur], n * sizeof(float2), hipMemcpyDeviceToHost, b->own_stream) != hipSuccess)
    return -EIO;
  if (hipStreamSynchronize(b->own_stream) != hipSuccess) return -EIO;
  b->fetched = true;
  return 0;
}

extern "C" int xlating_batch_output_host_cs16(xlating_batch *b, int id, const int16_t **output, size_t *output_len) {
  if (b == nullptr || id < 0 || (size_t)id >= b->clients.size() || !b->clients[id].alive || !b->fetched ||
      output == nullptr || output_len == nullptr || !b->last_q15)
    return -EINVAL;
  const Client &c = b->clients[id];
  if (c.last_K == 0 || (size_t)c.out_off + c.last_K > b->h_out_alloc) {  // (joined since the latest call: a row, but nothing in it yet)
    *output = nullptr;
    *output_len = 0;
    return c.last_K == 0 ? 0 : -EINVAL;
  }
  *output = b->h_out ? reinterpret_cast<const int16_t *>(b->h_out + c.out_off) : nullptr;
  *output_len = c.last_K;
  return 0;
}

extern "C" int xlating_batch_output_host(xlating_batch *b, int id, const float **output, size_t *output_len) {
  if (b == nullptr || id < 0 || (size_t)id >= b->clients.size() || !b->clients[id].alive || !b->fetched ||
      output == nullptr || output_len == nullptr || b->last_q15)
    return -EINVAL;
  const Client &c = b->clients[id];
  // (a client that joined since the latest call has a row -- assigned at add_client -- but no outputs, and its row may lie
  // beyond what the fetched image holds: the images grow with the next plan)
  if (c.last_K == 0 || (size_t)c.out_off + c.last_K > b->h_out_alloc) {
    *output = nullptr;
    *output_len = 0;
    return c.last_K == 0 ? 0 : -EINVAL;
  }
  *output = b->h_out ? reinterpret_cast<const float *>(b->h_out + c.out_off) : nullptr;
  *output_len = c.last_K;
  return 0;
}

extern "C" int xlating_batch_output_device(xlating_batch *b, int id, const void **d_output, size_t *output_len) {
  if (b == nullptr || id < 0 || (size_t)id >= b->clients.size() || !b->clients[id].alive || d_output == nullptr ||
      output_len == nullptr || b->d_out[b->ocur] == nullptr)  // (a dirty engine still holds the latest call's rows: the plan
                                                               // is only rebuilt by the next process call)
    return -EINVAL;
  const Client &c = b->clients[id];
  if (c.last_K == 0 || (size_t)c.out_off + c.last_K > b->out_alloc) {  // (joined since the latest call: a row, but nothing in it yet)
    *d_output = nullptr;
    *output_len = 0;
    return c.last_K == 0 ? 0 : -EINVAL;
  }
  *d_output = b->d_out[b->ocur] + c.out_off;
  *output_len = c.last_K;
  return 0;
}

extern "C" int xlating_batch_outputs_device(xlating_batch *b, size_t n, const int *ids, const void **d_outputs, size_t *output_lens) {
  if (b == nullptr || (n > 0 && (ids == nullptr || d_outputs == nullptr || output_lens == nullptr))) return -EINVAL;
  // (checked for every id before anything is filled: what xlating_batch_output_device refuses)
  if (n > 0 && b->d_out[b->ocur] == nullptr) return -EINVAL;
  for (size_t i = 0; i < n; ++i) {
    if (ids[i] < 0 || (size_t)ids[i] >= b->clients.size() || !b->clients[ids[i]].alive) return -EINVAL;
    const Client &c = b->clients[ids[i]];
    if (c.last_K != 0 && (size_t)c.out_off + c.last_K > b->out_alloc) return -EINVAL;
  }
  for (size_t i = 0; i < n; ++i) {
    const Client &c = b->clients[ids[i]];
    d_outputs[i] = c.last_K == 0 ? nullptr : b->d_out[b->ocur] + c.out_off;
    output_lens[i] = c.last_K;
  }
  return 0;
}

extern "C" int xlating_batch_client_phase(xlating_batch *b, int id, float *re, float *im) {
  if (b == nullptr || id < 0 || (size_t)id >= b->clients.size() || !b->clients[id].alive) return -EINVAL;
  if (hipSetDevice(b->device) != hipSuccess) return -EIO;
  xl_batch_sync_all(b);
  // the look-ahead may already have produced the phases behind the next calls further along the ring; the committed ones
  // (behind the latest processed call) are d_phase[pcur]
  float2 ph;
  if (hipMemcpy(&ph, b->d_phase[b->ahead.pcur] + id, sizeof(ph), hipMemcpyDeviceToHost) != hipSuccess) return -EIO;
  *re = ph.x;
  *im = ph.y;
  return 0;
}

extern "C" int xlating_batch_client_phase_q15(xlating_batch *b, int id, int16_t *re, int16_t *im) {
  if (b == nullptr || id < 0 || (size_t)id >= b->clients.size() || !b->clients[id].alive || b->fmt == XL_FMT_CF32 || re == nullptr ||
      im == nullptr)
    return -EINVAL;
  if (hipSetDevice(b->device) != hipSuccess) return -EIO;
  xl_batch_sync_all(b);
  // (option "q15_nco": a pending look-ahead has already written the phases AFTER the next call beside the committed ones: xl_q15_ahead.h)
  short2 ph;
  if (hipMemcpy(&ph, b->d_qphase[b->qahead.cur] + id, sizeof(ph), hipMemcpyDeviceToHost) != hipSuccess) return -EIO;
  *re = ph.x;
  *im = ph.y;
  return 0;
}

static int xl_batch_drain_events(xlating_batch *b) {
  xl_batch_sync_all(b);
  for (size_t i = 0; i + 2 <= b->ev.size(); i += 2) {
    float ms = 0.0f;
    if (hipEventElapsedTime(&ms, b->ev[i], b->ev[i + 1]) != hipSuccess) return -EIO;
    b->fir_ms += ms;
    b->timed_launches++;
  }
  for (size_t i = 0; i + 2 <= b->ev_ncot.size(); i += 2) {
    float ms = 0.0f;
    if (hipEventElapsedTime(&ms, b->ev_ncot[i], b->ev_ncot[i + 1]) != hipSuccess) return -EIO;
    b->nco_ms += ms;
    b->timed_nco++;
  }
  for (size_t i = 0; i + 4 <= b->ev_poly.size(); i += 4) {
    for (int k = 0; k < 3; ++k) {
      float ms = 0.0f;
      if (hipEventElapsedTime(&ms, b->ev_poly[i + k], b->ev_poly[i + k + 1]) != hipSuccess) return -EIO;
      b->poly_ms[k] += ms;
    }
    b->timed_poly++;
  }
  b->ev_pool.insert(b->ev_pool.end(), b->ev_poly.begin(), b->ev_poly.end());
  b->ev_poly.clear();
  b->ev_pool.insert(b->ev_pool.end(), b->ev.begin(), b->ev.end());
  b->ev_pool.insert(b->ev_pool.end(), b->ev_ncot.begin(), b->ev_ncot.end());
  b->ev.clear();
  b->ev_ncot.clear();
  return 0;
}

// tuning: cycles / wall ticks of the chain wave of the first `n` chain workgroups of the latest side-stream launch
extern "C" int xlating_batch_debug_chain_stats(xlating_batch *b, unsigned long long *out, int n) {
  if (b == nullptr || out == nullptr || b->d_chain_stats == nullptr || n < 1 || n > 4096) return -EINVAL;
  xl_batch_sync_all(b);
  return hipMemcpy(out, b->d_chain_stats, (size_t)n * 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost) == hipSuccess ? 0 : -EIO;
}

extern "C" int xlating_batch_timing(xlating_batch *b, int enable) {
  if (b == nullptr) return -EINVAL;
  if (hipSetDevice(b->device) != hipSuccess) return -EIO;
  if (b->timing && !enable) (void)xl_batch_drain_events(b);
  if (enable > 0 && b->ev_pool.size() < 2048) {  // pre-create so that the timed region itself creates none
    for (int i = 0; i < 2048; ++i) {
      hipEvent_t e;
      if (hipEventCreate(&e) != hipSuccess) break;
      b->ev_pool.push_back(e);
    }
  }
  b->timing = enable < 0 ? 0 : (enable > 2 ? 2 : enable);
  return 0;
}

extern "C" int xlating_batch_timing_stride(xlating_batch *b, unsigned every_n) {
  if (b == nullptr) return -EINVAL;
  b->timing_every = every_n ? every_n : 1;
  return 0;
}

extern "C" int xlating_batch_timing_polyphase(xlating_batch *b, double ms_total[3], int reset) {
  if (b == nullptr || ms_total == nullptr) return -EINVAL;
  if (hipSetDevice(b->device) != hipSuccess) return -EIO;
  int rc = xl_batch_drain_events(b);
  if (rc != 0) return rc;
  for (int k = 0; k < 3; ++k) ms_total[k] = b->poly_ms[k];
  const int n = b->timed_poly;
  if (reset) {
    b->poly_ms[0] = b->poly_ms[1] = b->poly_ms[2] = 0.0;
    b->timed_poly = 0;
  }
  return n;
}

extern "C" int xlating_batch_timing_read(xlating_batch *b, double *fir_ms_total, double *nco_ms_total, int reset) {
  if (b == nullptr) return -EINVAL;
  if (hipSetDevice(b->device) != hipSuccess) return -EIO;
  int rc = xl_batch_drain_events(b);
  if (rc != 0) return rc;
  if (fir_ms_total) *fir_ms_total = b->fir_ms;
  // the NCO launches are not one-to-one with calls (one extra look-ahead): report the per-call equivalent
  if (nco_ms_total) *nco_ms_total = b->timed_nco ? b->nco_ms / b->timed_nco * b->timed_launches : 0.0;
  const int n = b->timed_launches;
  if (reset) {
    b->fir_ms = b->nco_ms = 0.0;
    b->timed_launches = b->timed_nco = 0;
  }
  return n;
}
