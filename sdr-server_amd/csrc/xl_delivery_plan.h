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

#endif /* XL_DELIVERY_PLAN_H_ */
