// xl_plan.h -- the HOST LOGIC of the batch engine's plan (xl_batch.cpp: xl_batch_plan), as plain structs and free functions: which
// clients form which classes, which column a class member gets, the measured size rules, the images of the direct launches, the
// output rows.  Nothing here calls the HIP runtime or needs a device (device pointers inside the structs are plain data to this code):
// tests/c/plan_sweep.cpp drives it on the CPU under ASan and UBSan (tests/test_plan_cpu.py).  Allocation, upload, streams and launches
// stay in xl_batch.cpp.
#ifndef XL_PLAN_H_
#define XL_PLAN_H_

#include <map>
#include <vector>

#include "xl_device.h"
#include "xl_polyphase.h"
#include "xl_q15_mm.h"

#define XL_NLAUNCH 7

// The engine's settings that the plan's host logic reads: xlating_batch_t's fields of the same names (documented there).
struct XlPlanOpts {
  int fmt;
  uint32_t max_samples, gcap;
  int poly_mode;
  bool poly_min_set;
  uint32_t poly_min_clients, poly_m, mix_kernel;
  int mix_img;
  bool riders;
  int riders_min_wgs, exp_h, nco_side;
  uint32_t expected_clients;
  uint32_t q15_kernel;
};

struct Client {
  bool alive = false;
  uint32_t D = 0, T = 0, Tpad = 0;
  std::vector<float> rt;  // [Tpad] interleaved re,im, zero padded
  std::vector<int16_t> rtq;  // [T] the same taps in Q15 (xlating.c:486-487), interleaved re,im
  float incr[2] = {1.0f, 0.0f};
  int16_t qincr[2] = {0, 0};  // Q15 phase increment (xlating.c:548-549)
  uint64_t consumed = 0;
  uint32_t out_off = 0, out_cap = 0;  // the client's row in the output / phase-table images: assigned when it joins, kept for its lifetime
  uint32_t row_len = 0;               // elements reserved for the row (out_cap rounded up to the table-entry pair)
  uint64_t uid = 0;                   // unique over the engine's life (client ids are recycled, their taps are not)
  uint32_t last_K = 0;
  std::vector<uint32_t> last_Kg;  // outputs per block of the latest call
  bool planned_mature = false;
  bool qmm_digits = false;  // every entry of its Q15 rows has an int8 digit pair (xl_q15_digits.h, proof (a)): the matrix-core Q15 launch may carry it
  bool wide = false;  // no LDS tile of the direct kernel fits its window image (xl_wide.h), or its window exceeds XL_HCAP: the wide kernel
};

// every window of the client's next outputs lies inside its own stream (no zeros below its join point are needed)
static inline bool xl_mature(const Client &c) { return c.consumed >= (uint64_t)c.T - 1u; }

struct DirectClass {
  uint32_t D, T, rem0, hv0;
  std::vector<int> members;
};

struct Launch {
  int ct = 0;
  int nw = XL_NW_DEFAULT;  // waves (tiles) per workgroup
  uint32_t ota = 64;       // outputs per wave (smaller only when a 64-output window image exceeds the LDS)
  std::vector<XlGroup> groups;
  XlGroup *d_groups = nullptr;
  size_t lds = 0;  // window image bytes of the launch (max over its groups)
  uint32_t idle_waves = 0;  // spare waves over all groups (NCO rider slots per output tile)
  bool all_wide = true;  // every group has an even decimation
  uint32_t maxD = 1, minD = 0xFFFFFFFFu;
};

// A class of clients evaluated by the polyphase overlap-save path (xl_polyphase.hip) in optimized mode: all mature
// clients of one (D, T), whatever their grid offsets -- or clients of one (D, T) that joined together and are still
// inside their zero history (one grid, one zero_below).
#define XL_SIDE_ONE_BLOCK_MAX 2048u  // one-block polyphase calls: side-stream chain kernel up to this many clients

struct PolyClass {
  uint32_t D = 0, Dpad = 0, T = 0, A = 0, V = 0;
  uint32_t M = 256;          // transform length (64, 128 or 256), V = M - A + 1
  uint32_t ncols = 0, ncg = 0, nseg_cap = 0;
  uint32_t rem_ref0 = 0;     // plan-time record of the shared grid's reference client (xl_grid.h)
  uint32_t hv0 = XL_HCAP;    // plan-time valid history of the members (XL_HCAP: mature)
  uint32_t dmax = 0;         // largest grid offset of a member
  std::vector<int> members;
  // The class outlives re-plans (incremental planning): a member keeps its column for its lifetime, a column that a leaving
  // member frees is handed to the next joiner, and the branch spectra are computed for NEW columns only -- a join costs
  // one column of R (8 D M bytes), not the class's whole image.
  std::vector<int> col_client;        // column -> client id, -1 = free
  std::vector<uint32_t> col_delta;    // delay the column's spectra were built with
  std::vector<uint64_t> col_uid;      // ... and for whom (Client::uid)
  std::map<int, uint32_t> col_of;     // client id -> column
  uint32_t ncg_cap = 0;               // column groups the R / Y / cols buffers hold
  bool keep = false;                  // (planning scratch: the class was taken over by the new plan)
  // The branch spectra live in the mix launch's B-operand order (d_Rh).  mix_kind 1 (xlp_mix_mfma_kernel): scaled per column by a power
  // of two and split in two halves; per column the scale (host) and what undoes it (device).  mix_kind 3 (xlp_mix_f32_kernel): float32
  uint32_t mix_kind = 1, nkb = 0;
  void *d_Rh = nullptr;
  std::vector<float> col_scale;
  float *d_cscale = nullptr;
  float2 *d_X = nullptr;     // shared spectra [passes][Dpad][M][16]
  bool ximg = false;         // ... instead in the two-half mix's A-operand form (xl_xop_layout.h: the forward launch converts each value once;
                             // option "mix_operand_image"): [passes][M][2][2 nkb][16] 16-byte slots in the same buffer
  // two-half mix of a cf32 stream: per segment the largest component of its shared spectra, found by the forward launch (XlpArgs::segmax):
  // two buffers of seg_cap entries, a call uses buffer seg_par; lives and dies with d_X
  uint32_t *d_segmax = nullptr;
  uint32_t seg_cap = 0, seg_par = 0;
  float2 *d_Y = nullptr;     // mixed spectra  [cg][nseg_cap][sub][bin M][CW columns] (xl_y_layout.h)
  XlpCol *d_cols = nullptr;  // per column: output row, grid offset, NCO increment
  int last_inv = -1;         // which inverse kernel the class's latest launch took (describe; xlp_inverse_pick): 3 / 5 / 6, -1 = none yet
  uint64_t calls = 0;        // calls that enqueued the class's three launches (describe: "calls=N"); a call that falls back to the direct
                             // kernel does not count.  Carried over re-plans that keep the class, 0 for a class formed anew
};

// ---- output rows: free extents (offset -> length) below rows_end
uint32_t xl_row_alloc(std::map<uint32_t, uint32_t> &free_rows, uint32_t &rows_end, uint32_t len);
void xl_row_free(std::map<uint32_t, uint32_t> &free_rows, uint32_t &rows_end, uint32_t off, uint32_t len);

// End of a call of G blocks of S samples: every live client's outputs per block and in all (the block ends of its grid, xl_grid.h),
// and its stream position.  (Inline, like xl_direct_is_light: xl_batch_run's own per-call work.)
static inline void xl_clients_commit(std::vector<Client> &clients, uint32_t S, uint32_t G) {
  for (Client &c : clients) {
    if (!c.alive) continue;
    const uint32_t j0 = (uint32_t)((c.D - c.consumed % c.D) % c.D);
    c.last_Kg.resize(G);
    uint32_t prev = 0;
    for (uint32_t g = 1; g <= G; ++g) {
      const uint32_t ms = xl_grid_mstart(j0, c.D, S, g);
      c.last_Kg[g - 1] = ms - prev;
      prev = ms;
    }
    c.last_K = prev;
    c.consumed += S * G;
  }
}

// Direct FIR launches whose own work is short against the NCO chain (~25-32 us per block) gain from the side-stream chain
// kernel on reserved CUs like the polyphase launches do; heavier ones hide the chain in their spare waves for free and
// would only lose the reserved CUs.  Measured, 8 blocks per call, us per block fused -> side: 128 clients x 101 taps
// (40 M complex MACs per block) 29.9 -> 27.1; 128 x 505 native (202 M) 40.5 -> 35.5; 1024 x 101 (323 M) 37.9 -> 40.4;
// 1024 x 505 native (1615 M) 203 -> 227.
static inline bool xl_direct_is_light(double macs_per_block) { return macs_per_block < 250e6; }

// Who tabulates the NEXT call's phases: the NCO role inside this call's launches (false), or xl_nco_chain_kernel on the side
// stream, concurrently with them (true).  q15: a Q15 call (its family has a look-ahead of its own); nco_side: option
// "nco_side_stream"; light: xl_direct_is_light of the call's direct launches; masked_pair: the CU-masked stream pair exists;
// engine_stream: the call runs on the engine's stream (a caller's own, unmasked stream would keep filling the chain's CUs).
// The side stream pays for calls of several blocks on the polyphase path, whose three launches are short against the chain
// (measured, 8 blocks per call: 42.7 -> 36.8 us per block at 1024 clients, 30.7 -> 28.8 at 128); a direct FIR launch hides the
// chain in its spare waves for free and would only lose the chain kernel's CUs (1024 clients, native: 203 -> 212 us per block),
// and with one block per call the cross-stream events cost more than the overlap gains (51.3 -> 58.6).
// One-block calls (the reference's call granularity) on the polyphase path: the three launches are short since the mix runs on
// the matrix cores, and a slice of the recurrence inside each made every one of them last as long as its slice (1024 clients:
// 50.2 us per block; the chain kernel beside them, four calls per launch: 47.7; 128 clients: 40.4 -> 29.2; 4096: 129 -> 134,
// hence the limit XL_SIDE_ONE_BLOCK_MAX).
static inline bool xl_side_call(bool q15, int nco_side, unsigned G, bool use_poly, size_t nclients, bool light, bool masked_pair,
                                bool engine_stream) {
  const bool one_block_side = G == 1 && use_poly && nclients <= XL_SIDE_ONE_BLOCK_MAX;
  return !q15 && (nco_side > 0 || (nco_side < 0 && (G >= 2 || one_block_side) && (use_poly || (light && masked_pair && engine_stream))));
}

// ---- direct launches
extern const int kHeights[XL_NLAUNCH];
bool xl_riders_window(size_t wgs, int nw, uint32_t Tpad, int ct, uint32_t K, size_t lds, int min_wgs);
void xl_direct_classes(const std::vector<Client> &clients, const std::vector<bool> &use, std::vector<DirectClass> *out);
int xl_build_launches(const XlPlanOpts &o, const std::vector<Client> &clients, Launch *Ls, const std::vector<DirectClass> &classes,
                      int big_h, std::vector<float> *image, std::vector<double> *imageq);
double xl_direct_macs(const std::vector<DirectClass> &classes);  // complex MACs per sample of a block
int xl_pick_tile_height(const XlPlanOpts &o, const std::vector<DirectClass> &classes);

// ---- the matrix-core Q15 launch (option "q15_kernel"; xl_q15_mm.h)
struct XlQmmPlan {
  std::vector<XlQmmTile> tiles;
  std::vector<int8_t> image;  // the tiles' A images (xl_q15mm_fill_row)
  size_t lds = 0;             // window image bytes of the launch (max over its tiles)
  uint32_t nclients = 0;      // clients the launch carries
  uint32_t fb_digits = 0;     // non-wide clients left on the float64 launches: an entry without an int8 digit pair (proof (a))
  uint32_t fb_window = 0;     // ... no window image of the launch fits their (D, T), or proof (b) fails (no non-wide shape does either)
};
// Tiles of up to 32 clients per direct class over the eligible members of `classes`; the clients the launch carries are cleared in
// `rest_use` (the float64 launch set is built over what stays set).
void xl_build_q15mm(const XlPlanOpts &o, const std::vector<Client> &clients, const std::vector<DirectClass> &classes, XlQmmPlan *plan,
                    std::vector<bool> *rest_use);

// ---- polyphase classes
uint32_t xl_poly_pick_m(const XlPlanOpts &o, uint32_t A, size_t members, uint32_t D);
uint32_t xl_poly_mix_kind(const XlPlanOpts &o, uint32_t D);
bool xl_poly_ximg(const XlPlanOpts &o, uint32_t D, uint32_t M, size_t members);
float xl_poly_col_scale(const Client &c, uint32_t D, uint32_t T);

struct XlPolyPending {  // what the device images of next[idx] lack: the branch spectra of new_cols (fresh: all of its images)
  size_t idx;
  std::vector<uint32_t> new_cols;
  bool fresh;
};
// Forms the polyphase classes of a plan from the live, non-wide clients (planned_mature set) and the previous plan's classes, made
// `advanced` samples ago.  A class of `prev` that the new plan takes over is moved into `next` and marked keep (the others are the
// caller's to release); the members of the new classes are cleared in `rest_use`.
void xl_poly_form_classes(const XlPlanOpts &o, const std::vector<Client> &clients, std::vector<PolyClass> &prev, uint32_t advanced,
                          std::vector<PolyClass> *next, std::vector<XlPolyPending> *pending, std::vector<bool> *rest_use);

// ---- CU reservation for the side-stream chain kernel
struct XlReserve {
  uint32_t want;  // CUs per XCD
  int band;       // band of the rule the plan is in (xl_chain_band)
};
// nclients: the plan's NCO records; last_band: the previous plan's band (-1: none); exp_*: the tuning switches XL_EXP_NOMASK,
// XL_EXP_ROUNDS1 and XL_EXP_RESERVE as values (exp_reserve < 0: not set)
XlReserve xl_reserve_want(const XlPlanOpts &o, size_t nclients, const std::vector<DirectClass> &classes_rest,
                          const std::vector<PolyClass> &poly, double macs_all, double macs_rest, int last_band, bool exp_nomask,
                          bool exp_rounds1, int exp_reserve);
bool xl_reserve_recreate(uint32_t want, uint32_t reserve_r);

#endif  // XL_PLAN_H_
