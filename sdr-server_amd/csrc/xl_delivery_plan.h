/* xl_delivery_plan.h -- the layout of a delivery batch (include/xlating_delivery.h): where each row lies in the packed image, the
 * table of runs the pack kernel reads, which rows a workgroup's chunk holds.  Pure integers, plain C, no HIP (compiled by gcc, with the
 * sanitizers, in tests/c/delivery_plan_sweep.c).  The only place that decides them: xl_delivery.cpp and xl_delivery.hip read this struct
 * and call these functions.
 *
 * The image: rows in the order given, row i at the lowest offset at or behind the end of row i - 1 that is CONGRUENT TO ITS SOURCE
 * ADDRESS MOD 16 (at most 12 bytes of padding in front of a row; the first row starts at its source's residue).  A 16-byte slot of the
 * image then corresponds to an aligned 16-byte slot of the source: the body of a row moves in 16-byte accesses, its head and tail (and
 * a slot that two short rows share) in dwords.  The image's size -- what crosses to the host -- is the end of the last row.
 * The NARROWED image (xl_dlv_plan_narrow; the rows are cf32, 8 bytes a sample at 8-byte aligned addresses, and cross as cs16, 4 bytes a
 * sample): the same, with row i at the lowest offset at or behind its predecessor's end that is congruent to (SOURCE ADDRESS MOD 32) / 2
 * MOD 16.  Image offset p of a run then comes from address src + 2 (p - off) (xl_dlv_narrow_src), and a whole 16-byte slot of the image
 * inside a row is exactly one 32-byte-aligned 32-byte span of the source: two aligned 16-byte loads, eight conversions
 * (xl_dlv_narrow.h), one aligned 16-byte store; a slot a row covers in part moves sample by sample.  Runs, chunks and the search are
 * the same, all in image offsets: a chunk of XL_DLV_CHUNK image bytes is 4096 samples, 32 KiB of source.
 * Runs: one per row of at least one byte (an empty row has no run, no bytes and no place), in image order; s16 = off / 16 is the sum
 * xl_ragged_find searches: nondecreasing, 0 for the first run.
 * Chunks: workgroup c moves image bytes [c * XL_DLV_CHUNK, (c + 1) * XL_DLV_CHUNK).  xl_ragged_find(key = c * XL_DLV_CHUNK / 16) gives the
 * LAST run that begins in or before the chunk's first slot; xl_dlv_first steps back over the runs before it that still reach into the
 * chunk (short rows sharing that slot, or the row that crosses the chunk's start: at most four steps); from there the workgroup walks
 * forward until a run begins at or behind the chunk's end, moving xl_dlv_span of each. */
#ifndef XL_DELIVERY_PLAN_H_
#define XL_DELIVERY_PLAN_H_

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define XL_DLV_FN static inline __host__ __device__
#else
#define XL_DLV_FN static inline
#endif

#define XL_DLV_CHUNK 16384u                      /* bytes of the image per workgroup */
#define XL_DLV_THREADS 256u                      /* threads per workgroup: XL_DLV_CHUNK / 16 / XL_DLV_THREADS = 4 slots each */
#define XL_DLV_SLOTS_PER_THREAD (XL_DLV_CHUNK / 16u / XL_DLV_THREADS)
#define XL_DLV_ROW_MAX ((uint64_t)0xFFFFFFFCu)   /* bytes of one row */
#define XL_DLV_IMAGE_MAX ((uint64_t)1 << 34)     /* bytes of one image: its chunks and s16 fit 32 bits with room to spare */

typedef struct {
  uint64_t src;   /* device address of the row's first byte (4-byte aligned; of a narrowed run 8-byte aligned) */
  uint64_t off;   /* the row's first byte in the image: off % 16 == src % 16 (of a narrowed run: == src % 32 / 2) */
  uint32_t bytes; /* of the image: > 0, a multiple of 4 */
  uint32_t s16;   /* off / 16 */
} XlDlvRun;

/* the lowest offset at or behind `end` that is congruent to `residue` (< 16) mod 16 */
XL_DLV_FN uint64_t xl_dlv_place_at(uint64_t end, uint64_t residue) {
  const uint64_t x = (end & ~(uint64_t)15) + residue;
  return x < end ? x + 16u : x;
}

/* where a row from address src begins behind image offset `end` */
XL_DLV_FN uint64_t xl_dlv_place(uint64_t end, uint64_t src) { return xl_dlv_place_at(end, src & 15u); }

/* the same for a narrowed row: two source bytes a byte of the image, so the residue is that of the source in its 32-byte span, halved */
XL_DLV_FN uint64_t xl_dlv_place_narrow(uint64_t end, uint64_t src) { return xl_dlv_place_at(end, (src & 31u) >> 1); }

/* the source address of image offset p (in the run, a multiple of 4) of a narrowed run: the 8-byte sample that becomes that dword */
XL_DLV_FN uint64_t xl_dlv_narrow_src(const XlDlvRun *r, uint64_t p) { return r->src + 2u * (p - r->off); }

/* Both layouts.  narrow == 0: count[i] is the row's bytes; otherwise its cf32 samples, each 8 bytes of the source and 4 of the image. */
static inline int xl_dlv_plan_rows(int narrow, size_t n, const uint64_t *src, const uint64_t *count, uint64_t *off, XlDlvRun *runs,
                                   size_t *nruns, uint64_t *total) {
  uint64_t end = 0;
  size_t k = 0;
  for (size_t i = 0; i < n; ++i) {
    if (count[i] == 0) {
      off[i] = ~(uint64_t)0;
      continue;
    }
    if (src[i] == 0 || (src[i] & (narrow ? 7u : 3u)) != 0) return -1;
    if (narrow ? count[i] > XL_DLV_ROW_MAX / 4u : ((count[i] & 3u) != 0 || count[i] > XL_DLV_ROW_MAX)) return -1;
    const uint64_t bytes = narrow ? 4u * count[i] : count[i];
    const uint64_t at = narrow ? xl_dlv_place_narrow(end, src[i]) : xl_dlv_place(end, src[i]);
    off[i] = at;
    runs[k].src = src[i], runs[k].off = at, runs[k].bytes = (uint32_t)bytes, runs[k].s16 = (uint32_t)(at >> 4);
    ++k;
    end = at + bytes;
    if (end > XL_DLV_IMAGE_MAX) return -1;
  }
  *nruns = k;
  *total = end;
  return 0;
}

/* Lays out n rows.  off[i] (n entries): row i's image offset, or (uint64_t)-1 for an empty row.  runs (room for n): the runs, *nruns of
 * them.  *total: the image's bytes.  0, or -1: a row that is not 4-byte aligned, not a multiple of 4, too long, or an image too large. */
static inline int xl_dlv_plan(size_t n, const uint64_t *src, const uint64_t *bytes, uint64_t *off, XlDlvRun *runs, size_t *nruns,
                              uint64_t *total) {
  return xl_dlv_plan_rows(0, n, src, bytes, off, runs, nruns, total);
}

/* Lays out n narrowed rows of n_complex[i] cf32 samples each: the same outputs, a run's bytes being the 4 * n_complex[i] of the image.
 * 0, or -1: a row that is not 8-byte aligned, of more than XL_DLV_ROW_MAX output bytes, or an image too large. */
static inline int xl_dlv_plan_narrow(size_t n, const uint64_t *src, const uint64_t *n_complex, uint64_t *off, XlDlvRun *runs,
                                     size_t *nruns, uint64_t *total) {
  return xl_dlv_plan_rows(1, n, src, n_complex, off, runs, nruns, total);
}

/* workgroups of the launch */
XL_DLV_FN uint32_t xl_dlv_chunks(uint64_t total) { return (uint32_t)((total + XL_DLV_CHUNK - 1u) / XL_DLV_CHUNK); }

/* the first run of chunk c, given `found` = xl_ragged_find's answer for key = c * XL_DLV_CHUNK / 16 */
XL_DLV_FN uint32_t xl_dlv_first(const XlDlvRun *runs, uint32_t found, uint32_t c) {
  const uint64_t lo = (uint64_t)c * XL_DLV_CHUNK;
  while (found > 0u && runs[found - 1u].off + runs[found - 1u].bytes > lo) --found;
  return found;
}

/* the image bytes [*a, *b) of run r that chunk c moves; 0 when there are none */
XL_DLV_FN int xl_dlv_span(const XlDlvRun *r, uint32_t c, uint64_t *a, uint64_t *b) {
  const uint64_t lo = (uint64_t)c * XL_DLV_CHUNK, hi = lo + XL_DLV_CHUNK, end = r->off + r->bytes;
  *a = r->off > lo ? r->off : lo;
  *b = end < hi ? end : hi;
  return *a < *b;
}

/* ------------------------------------------------------------------- the narrowed layout with a gain and a level a row
 * (xlating_delivery_pack_device_cs16_gain, xl_delivery_gain.hip).  The image is xl_dlv_plan_narrow's, byte for byte in the same places:
 * the run record below carries an XlDlvRun, so xl_dlv_span and xl_dlv_narrow_src serve it as they are; beside it the run's gain (the
 * gain belongs to the RUN: two short rows that share a 16-byte slot may differ) and the index of its entry of the LEVEL TABLE, which
 * lies behind the image at the next 16-byte boundary: XL_DLV_LEVEL_WORDS uint32 a run (peak_bits, clipped, nans: xl_dlv_gain.h), in
 * the order of the runs.  Image and table cross to the host in one copy of *full bytes. */
#define XL_DLV_GAIN_LO (-48) /* xl_dlv_gain.h's XL_DLV_GAIN_MIN .. XL_DLV_GAIN_MAX (tests/c/delivery_gain_sweep.c holds them equal) */
#define XL_DLV_GAIN_HI 48
#define XL_DLV_LEVEL_WORDS 3u
#define XL_DLV_LEVEL_PEAK 0u
#define XL_DLV_LEVEL_CLIPPED 1u
#define XL_DLV_LEVEL_NANS 2u
#define XL_DLV_NO_LEVEL (~(uint32_t)0) /* an empty row's */

typedef struct {
  XlDlvRun r;    /* as xl_dlv_plan_narrow fills it */
  int32_t gain;  /* XL_DLV_GAIN_LO .. XL_DLV_GAIN_HI */
  uint32_t lvl;  /* its entry of the level table */
} XlDlvGainRun;

/* Lays out n narrowed rows with gain[i] each.  off, *total: as of xl_dlv_plan_narrow (scratch: room for n XlDlvRun).  lvl[i] (n
 * entries): row i's entry of the level table, or XL_DLV_NO_LEVEL for an empty row.  runs (room for n), *nruns.  *lvl_off: where the
 * table begins, *full: where it ends -- both 0 when there is no run.  0, or -1: xl_dlv_plan_narrow's refusals, or a gain outside
 * XL_DLV_GAIN_LO .. XL_DLV_GAIN_HI (an empty row's included); nothing is to be used then. */
static inline int xl_dlv_plan_gain(size_t n, const uint64_t *src, const uint64_t *n_complex, const int8_t *gain, uint64_t *off,
                                   uint32_t *lvl, XlDlvRun *scratch, XlDlvGainRun *runs, size_t *nruns, uint64_t *total,
                                   uint64_t *lvl_off, uint64_t *full) {
  for (size_t i = 0; i < n; ++i)
    if (gain[i] < XL_DLV_GAIN_LO || gain[i] > XL_DLV_GAIN_HI) return -1;
  if (xl_dlv_plan_narrow(n, src, n_complex, off, scratch, nruns, total) != 0) return -1;
  size_t k = 0;
  for (size_t i = 0; i < n; ++i) {
    if (n_complex[i] == 0) {
      lvl[i] = XL_DLV_NO_LEVEL;
      continue;
    }
    runs[k].r = scratch[k], runs[k].gain = gain[i], runs[k].lvl = (uint32_t)k;
    lvl[i] = (uint32_t)k;
    ++k;
  }
  *lvl_off = k > 0 ? (*total + 15u) & ~(uint64_t)15 : 0u;
  *full = k > 0 ? *lvl_off + 4u * XL_DLV_LEVEL_WORDS * (uint64_t)k : 0u;
  return 0;
}

/* xl_dlv_first for these records */
XL_DLV_FN uint32_t xl_dlv_gain_first(const XlDlvGainRun *runs, uint32_t found, uint32_t c) {
  const uint64_t lo = (uint64_t)c * XL_DLV_CHUNK;
  while (found > 0u && runs[found - 1u].r.off + runs[found - 1u].r.bytes > lo) --found;
  return found;
}

#endif /* XL_DELIVERY_PLAN_H_ */
