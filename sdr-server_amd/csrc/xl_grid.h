/* xl_grid.h -- the integer bookkeeping of the streaming rule, shared by host code, device code and the CPU tests
 * (tests/test_grid.py compiles this header with gcc and checks it against brute force).
 *
 * Reference: src/xlating.c:52-83.  A filter created at stream position `join` produces output k from
 * the T samples that END at sample k*D of ITS stream (the reference's working buffer starts with T-1 zeros,
 * xlating.c:552-559), in the process_* call during which that newest sample arrives, and renormalises its NCO phase
 * once at the end of every call that produced output (xlating.c:73).
 *
 * One engine call covers G consecutive blocks of S samples each (G = 1: the reference's call; G > 1: a "group", the
 * results of G successive calls from one set of launches).  With
 *     consumed = samples the client has seen before the call        j0 = (-consumed) mod D
 * output m of the call (m = 0 .. K-1, K = ceil((G*S - j0) / D)) has its newest sample at call-local position
 * j0 + m*D, belongs to block (j0 + m*D) / S, and its window starts at XL_HCAP - (T-1) + j0 + m*D in
 * [history | blocks] coordinates.  Plans are resident: a class stores (rem0, hv0) = (consumed mod D,
 * min(consumed, XL_HCAP)) at plan time and every launch gets the stream position since then (XlPos) as a kernel
 * argument -- nothing per class travels per call, whatever the number of classes.
 */
#ifndef XL_GRID_H_
#define XL_GRID_H_
#include <stdint.h>

#define XL_HCAP 16384u /* raw history kept on the device, in samples; T - 1 + D <= XL_HCAP */
#define XL_PH_STRIDE 16u /* the NCO phase table holds every 16th phase (xl_device.h says why): entry (out_off + m) / 16 = phase of */
#define XL_PH_SHIFT 4u   /* output m, m = 0 mod 16 */

#if defined(__HIPCC__)
#define XL_HD __host__ __device__ static inline
#else
#define XL_HD static inline
#endif

typedef struct XlPos {
  uint32_t trel; /* samples the engine consumed between the plan and the start of this call (< 2^31; the engine re-plans before it overflows) */
  uint32_t S;    /* samples per block of this call */
  uint32_t G;    /* blocks in this call (>= 1) */
  uint32_t pad;  /* flags: XL_POS_NORENORM = the call never renormalises the NCO phase (the reference's x86 AVX build, xlating.c:338-339) */
} XlPos;
#define XL_POS_NORENORM 1u
#define XL_POS_FMA_STEP 2u /* the phase recurrence step as gcc -ffast-math -mfma contracts `phase * phase_incr`: re = fma(pr, ir, -(pi*ii)),
                              im = fma(pr, ii, pi*ir) -- reference builds with FMA enabled (e.g. -march=native on an AVX2 host) */

typedef struct XlDyn {
  uint32_t base;       /* sample index in [history | blocks] coordinates of the first tap of output 0 */
  uint32_t K;          /* outputs of the call */
  uint32_t zero_below; /* samples with index < zero_below read as 0 (the client joined mid-stream) */
  uint32_t j0;         /* call-local position of output 0's newest sample */
} XlDyn;

/* per-call numbers of a class from its plan-time record, for a raw history of `hcap` samples in front of the call's blocks
 * (hv0 = min(consumed, hcap) at plan time).  The wide direct kernel (xl_wide.hip) may read a history longer than XL_HCAP. */
XL_HD XlDyn xl_grid_dyn_cap(uint32_t D, uint32_t T, uint32_t rem0, uint32_t hv0, XlPos p, uint32_t hcap) {
  const uint32_t rem = (rem0 % D + p.trel % D) % D;
  const uint32_t j0 = (D - rem) % D;
  const uint32_t N = p.S * p.G;
  uint32_t hv = hv0 + (p.trel < hcap ? p.trel : hcap);
  XlDyn d;
  if (hv > hcap) hv = hcap;
  d.j0 = j0;
  d.K = N > j0 ? (N - j0 + D - 1u) / D : 0u;
  d.base = hcap - (T - 1u) + j0;
  d.zero_below = hcap - hv;
  return d;
}

/* the same for the XL_HCAP history every other kernel reads */
XL_HD XlDyn xl_grid_dyn(uint32_t D, uint32_t T, uint32_t rem0, uint32_t hv0, XlPos p) {
  return xl_grid_dyn_cap(D, T, rem0, hv0, p, XL_HCAP);
}

/* stream position of the NEXT call if it has the same shape (the guess the NCO look-ahead makes) */
XL_HD XlPos xl_grid_next(XlPos p) {
  XlPos n = p;
  n.trel = p.trel + p.S * p.G;
  return n;
}

/* index of the first output of block g (g = 0 .. G): the outputs whose newest sample lies before g*S */
XL_HD uint32_t xl_grid_mstart(uint32_t j0, uint32_t D, uint32_t S, uint32_t g) {
  const uint32_t n = g * S;
  return n > j0 ? (n - j0 + D - 1u) / D : 0u;
}

/* Block boundaries of a call on one client's output index (NCO renormalisation points, xlating.c:73). */
typedef struct XlBnd {
  uint32_t j0, D, S, G, K;
  uint32_t flags; /* XL_POS_NORENORM: no renormalisation point exists */
} XlBnd;

/* smallest block-start index > m, or K when m lies in the last block: the phase is renormalised between
 * outputs xl_bnd_next(m) - 1 and xl_bnd_next(m).  Needs every block of a multi-block call to hold an output (S >= D). */
XL_HD uint32_t xl_bnd_next(const XlBnd b, uint32_t m) {
  uint32_t g, nb;
  if (b.flags & XL_POS_NORENORM) return 0xFFFFFFFFu; /* never reached: nobody renormalises */
  if (b.G <= 1u) return b.K;
  g = (b.j0 + m * b.D) / b.S;
  if (g + 1u >= b.G) return b.K;
  nb = xl_grid_mstart(b.j0, b.D, b.S, g + 1u);
  return nb < b.K ? nb : b.K;
}

/* ---- merged polyphase classes (xl_polyphase.hip): clients of one (D, T) whose output grids are offset against each
 * other share ONE grid of D-spaced window starts, the "shared grid", whose point q = 0 lies D samples before the
 * window of output 0 of a virtual reference client with j0 = j0_ref.  A member with
 *     delta = (j0_c - j0_ref) mod D        (constant over the calls: both move by -G*S mod D per call)
 * is evaluated with its taps delayed by delta samples (delta leading zeros baked into its branch spectra), and its
 * output k is the shared point q = k + 1 - wrap, wrap = (j0_ref + delta >= D). */
XL_HD uint32_t xl_merge_j0(uint32_t j0_ref, uint32_t delta, uint32_t D) {
  const uint32_t j = j0_ref + delta;
  return j >= D ? j - D : j;
}
/* q - k of a member */
XL_HD uint32_t xl_merge_shift(uint32_t j0_ref, uint32_t delta, uint32_t D) { return j0_ref + delta >= D ? 0u : 1u; }
/* shared points a call must evaluate so that every member gets all its outputs (q < Kq) */
XL_HD uint32_t xl_merge_points(uint32_t D, XlPos p) { return (p.S * p.G + D - 1u) / D + 1u; }
/* outputs a member owns in the call: one more than floor(N / D) when its j0 < N mod D (= XlDyn::K of its own grid) */
XL_HD uint32_t xl_merge_outputs(uint32_t j0_ref, uint32_t delta, uint32_t D, XlPos p) {
  const uint32_t N = p.S * p.G, Ka = N / D;
  return Ka + (xl_merge_j0(j0_ref, delta, D) < N - Ka * D ? 1u : 0u);
}

/* Phase expansion duty of the inverse launches, per (member column, segment s of V shared points, group g of XL_PH_STRIDE points):
 * the phases of the column's outputs that are the shared points s V + 16 g .. + 15, walked from ONE entry of the phase table. */
typedef struct XlColDuty {
  XlBnd bnd;      /* the column's block boundaries in this call (K: the outputs it owns, whether vacant or not) */
  uint32_t shift; /* q - k of the column */
  uint32_t ibeg;  /* 1: the group's first shared point is nobody's output (shared point 0 of a column with shift 1) */
  uint32_t m0;    /* the column's output index of the first phase to expand */
  uint32_t ok;    /* 0: nothing to expand (vacant column, group beyond V, outputs beyond K) */
  uint32_t tab;   /* entry of the column's part of the phase table the walk starts from, m0 / 16 (0 when there is nothing to expand) */
} XlColDuty;
XL_HD XlColDuty xl_col_duty(uint32_t j0_ref, uint32_t delta, uint32_t D, XlPos p, uint32_t V, uint32_t s, uint32_t g, int vacant) {
  XlColDuty d;
  uint32_t q0;
  d.bnd.j0 = xl_merge_j0(j0_ref, delta, D), d.bnd.D = D, d.bnd.S = p.S, d.bnd.G = p.G, d.bnd.flags = p.pad;
  d.bnd.K = xl_merge_outputs(j0_ref, delta, D, p);
  d.shift = xl_merge_shift(j0_ref, delta, D);
  q0 = s * V + g * XL_PH_STRIDE;
  d.ibeg = q0 < d.shift ? 1u : 0u;
  d.m0 = q0 + d.ibeg - d.shift;
  d.ok = !vacant && g * XL_PH_STRIDE < V && d.m0 < d.bnd.K ? 1u : 0u;
  d.tab = d.ok ? d.m0 >> XL_PH_SHIFT : 0u;
  return d;
}
/* phases to expand from output m0 on: to the end of the group or of the column's outputs; 0 when there is nothing to expand.  (A
 * function of the duty, not a field: a kernel takes it where the walk starts and does not carry it through its transforms.) */
XL_HD uint32_t xl_col_duty_count(XlColDuty d) {
  const uint32_t left = d.bnd.K - d.m0, span = XL_PH_STRIDE - d.ibeg;
  return d.ok ? (left < span ? left : span) : 0u;
}

/* ---- the same expansion with the duties on the TABLE's grid (the inverse launches; xl_col_duty above stays for its test and as the
 * statement these duties are checked against).  A column's outputs in segment s are m in [m_lo, m_hi): the shared points s V .. s V + V - 1
 * that are its outputs, less its shift.  With t0 = m_lo / 16, lane g of the column (g < M / 16) takes table entry t0 + g and expands
 * exactly the XL_PH_STRIDE phases m = 16 (t0 + g) .. + 15 -- no step before its first phase; phase m belongs to row position
 * m + shift - s V and is stored where m lies in the window.  m_lo - 16 t0 <= 15 and m_hi - m_lo <= V, so the M / 16 lanes cover the
 * window but for at most xl_grid_extra() phases, which the last lane reaches by stepping on from its running phase. */
XL_HD uint32_t xl_grid_extra(uint32_t M, uint32_t V) { return V + (XL_PH_STRIDE - 1u) > M ? V + (XL_PH_STRIDE - 1u) - M : 0u; }

typedef struct XlGridDuty {
  XlBnd bnd;      /* as XlColDuty */
  uint32_t shift; /* q - k of the column */
  uint32_t ma;    /* the lane's first phase, 16 (t0 + g): the output its table entry belongs to */
  uint32_t pos;   /* row position of phase ma, ma + shift - s V; below 0 (wrapped) where ma lies before the window */
  uint32_t rel;   /* ma - m_lo (wrapped): phase ma + i is stored exactly when rel + i < span in unsigned arithmetic */
  uint32_t span;  /* m_hi - m_lo; 0 when the lane has nothing to store (vacant column, empty window, entry beyond the window) */
  uint32_t tab;   /* t0 + g, the entry of the column's part of the phase table (0 when span = 0) */
} XlGridDuty;
XL_HD XlGridDuty xl_grid_duty(uint32_t j0_ref, uint32_t delta, uint32_t D, XlPos p, uint32_t V, uint32_t s, uint32_t g, int vacant) {
  XlGridDuty d;
  uint32_t qlo, qhi, m_lo, m_hi;
  d.bnd.j0 = xl_merge_j0(j0_ref, delta, D), d.bnd.D = D, d.bnd.S = p.S, d.bnd.G = p.G, d.bnd.flags = p.pad;
  d.bnd.K = xl_merge_outputs(j0_ref, delta, D, p);
  d.shift = xl_merge_shift(j0_ref, delta, D);
  qlo = s * V > d.shift ? s * V : d.shift;
  qhi = s * V + V < d.shift + d.bnd.K ? s * V + V : d.shift + d.bnd.K;
  m_lo = qlo - d.shift;
  m_hi = qhi > qlo ? qhi - d.shift : m_lo;
  d.ma = (m_lo & ~(XL_PH_STRIDE - 1u)) + g * XL_PH_STRIDE;
  d.pos = d.ma + d.shift - s * V;
  d.rel = d.ma - m_lo;
  d.span = !vacant && d.ma < m_hi ? m_hi - m_lo : 0u;
  d.tab = d.span ? d.ma >> XL_PH_SHIFT : 0u;
  return d;
}

/* floor(x / d) from rcp = xl_rcp32(d): a multiply-high and one correction, exact for every 32-bit x and d >= 1
 * (x rcp / 2^32 lies in (x / d - 1, x / d]).  The inverse launches get the reciprocals of S and D as arguments. */
XL_HD uint32_t xl_rcp32(uint32_t d) { return d > 1u ? (uint32_t)(0x100000000ull / d) : 0xFFFFFFFFu; }
XL_HD uint32_t xl_div_rcp(uint32_t x, uint32_t d, uint32_t rcp) {
  const uint32_t q = (uint32_t)(((uint64_t)x * rcp) >> 32);
  return q + (x - q * d >= d ? 1u : 0u);
}
/* xl_bnd_next without a division: rS = xl_rcp32(b.S), rD = xl_rcp32(b.D) */
XL_HD uint32_t xl_bnd_next_rcp(const XlBnd b, uint32_t rS, uint32_t rD, uint32_t m) {
  uint32_t g, n, nb;
  if (b.flags & XL_POS_NORENORM) return 0xFFFFFFFFu;
  if (b.G <= 1u) return b.K;
  g = xl_div_rcp(b.j0 + m * b.D, b.S, rS);
  if (g + 1u >= b.G) return b.K;
  n = (g + 1u) * b.S;
  nb = n > b.j0 ? xl_div_rcp(n - b.j0 + b.D - 1u, b.D, rD) : 0u;
  return nb < b.K ? nb : b.K;
}

#endif /* XL_GRID_H_ */
