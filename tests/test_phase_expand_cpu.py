"""CPU tests of the inverse launches' phase expansion on the table's grid (sdr-server_amd/csrc/xl_grid.h: xl_grid_duty, xl_grid_extra,
xl_div_rcp, xl_bnd_next_rcp) and of the control flow of its device-side walk (xl_dev_inline.h: xl_phase_expand), restated in C beside
the header and compiled with gcc like tests/test_grid.py -- the logic, not the HIP code itself (tests/test_phase_expand_gpu.py runs
that).

The sweep: D in {8, 21, 42, 100}; the classes (M, V) = (64, 52), (128, 116), (256, 244) of a 505-tap filter on 42 branches and V at
its extremes M / 2 + 1 and M - 1 for each M (a class has 2 <= A <= M / 2 taps per branch, V = M - A + 1); calls of G = 1, 2 and 8
blocks; for G > 1 block lengths S0 + r D, r < 16 (G = 8: r = 0, 5, 10, 15 and blocks short enough that most segments hold a block
end), which move every block end through all residues mod 16; EVERY (j0_ref, delta) pair and every segment of the call.  Checked per
column:

* same stores: the (output m, row position) pairs the new duties store are those xl_col_duty + xl_phase_walk stored at the positions
  the epilogues read (below V: the old duty's last group ran on past the segment's end into positions nobody reads), each exactly once,
  and together they are the column's outputs, each at its shared point's place in its segment;
* step bound: a lane's stores lie within 16 + extra phases of its table entry, extra = max(0, V + 15 - M), and only the last lane
  uses more than 16;
* block-end index: xl_bnd_next_rcp equals the block ends counted off sample by sample at every phase of every lane's range, and
  xl_bnd_next equals them at each range's first and last phase (the division at every phase is what makes the sweep slow;
  tests/test_grid.py holds xl_bnd_next to brute force); xl_div_rcp equals the division on random and edge operands;
* same bits (on a sample of the pairs, every D, class, G and length): a float32 model of the walk -- straight line where no lane of the
  column has a block end in front of a phase it stores, xl_phase_walk otherwise, and xl_phase_walk everywhere when forced -- gives the
  bits of a model of the producer's chain (xl_nco_client_chain: three IEEE operations per step, renormalised at block ends with the
  double hypot of xl_nco_renorm) from the same table entries."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sdr-server_amd", "csrc")

SHIM = r"""
#include <math.h>
#include <string.h>
#include "xl_grid.h"

#define MAXPOS 320
#define MAXK 8192

static XlPos pos_of(uint32_t S, uint32_t G) { XlPos p = {0, S, G, 0}; return p; }

/* one column: 0 = fine, else the line of the first check that failed (what[] = s, g, i) */
static int column(uint32_t D, uint32_t M, uint32_t V, uint32_t S, uint32_t G, uint32_t j0_ref, uint32_t delta, uint32_t *what) {
  const XlPos p = pos_of(S, G);
  const uint32_t GQ = M / XL_PH_STRIDE, extra = xl_grid_extra(M, V);
  const uint32_t rS = xl_rcp32(S), rD = xl_rcp32(D);
  const uint32_t K = xl_merge_outputs(j0_ref, delta, D, p), shift = xl_merge_shift(j0_ref, delta, D);
  const uint32_t nseg = (xl_merge_points(D, p) + V - 1u) / V;
  static unsigned char seen[MAXK];
  static uint32_t nbref[MAXK + 64]; /* xl_bnd_next by brute force: the blocks counted off sample by sample, no division */
  uint32_t s, g, i, total = 0;
  if (K > MAXK || extra > 14u) return __LINE__;
  memset(seen, 0, K);
  {
    const uint32_t j0 = xl_merge_j0(j0_ref, delta, D);
    uint32_t m, b = 0, first = 0; /* first: outputs whose newest sample lies before the end of block b */
    for (m = 0; m < K + 64u; ++m) {
      while (b < G && j0 + m * D >= (b + 1u) * S) ++b;
      if (m >= first) { /* the end of block b as an output index */
        uint64_t e = (uint64_t)(b + 1u) * S;
        first = e > j0 ? (uint32_t)((e - j0 + D - 1u) / D) : 0u;
      }
      nbref[m] = G <= 1u || b + 1u >= G ? K : (first < K ? first : K);
    }
  }
  for (s = 0; s < nseg; ++s) {
    uint32_t oldm[MAXPOS], newm[MAXPOS]; /* output index + 1 stored at a row position */
    memset(oldm, 0, sizeof oldm), memset(newm, 0, sizeof newm);
    what[0] = s;
    for (g = 0; g < GQ; ++g) {
      const XlColDuty d = xl_col_duty(j0_ref, delta, D, p, V, s, g, 0);
      const uint32_t cnt = xl_col_duty_count(d);
      for (i = 0; i < cnt; ++i) {
        const uint32_t at = g * XL_PH_STRIDE + d.ibeg + i;
        if (at >= V) continue; /* (never read) */
        if (oldm[at]) return __LINE__;
        oldm[at] = d.m0 + i + 1u;
      }
    }
    for (g = 0; g < GQ; ++g) {
      const XlGridDuty d = xl_grid_duty(j0_ref, delta, D, p, V, s, g, 0);
      const uint32_t n = XL_PH_STRIDE + (g == GQ - 1u ? extra : 0u);
      what[1] = g;
      if (s < 2u) { /* vacant: nothing, entry 0 */
        const XlGridDuty v = xl_grid_duty(j0_ref, delta, D, p, V, s, g, 1);
        if (v.span != 0u || v.tab != 0u) return __LINE__;
      }
      if (d.bnd.K != K || d.shift != shift || d.bnd.j0 != xl_merge_j0(j0_ref, delta, D)) return __LINE__;
      if (d.ma % XL_PH_STRIDE != 0u || d.pos != d.ma + shift - s * V) return __LINE__;
      if (d.span == 0u ? d.tab != 0u : (d.tab != d.ma / XL_PH_STRIDE || d.ma >= K)) return __LINE__;
      for (i = 0; i < n + 4u; ++i) { /* (a few beyond: nothing may lie there) */
        const int st = d.rel + i < d.span;
        what[2] = i;
        if (i >= n) {
          if (st && g == GQ - 1u) return __LINE__; /* the window reaches past 16 + extra steps of the last lane */
          continue; /* (an inner lane's later phases are the next lane's) */
        }
        if (st) {
          const uint32_t at = d.pos + i;
          if (at >= V || newm[at]) return __LINE__;
          newm[at] = d.ma + i + 1u;
          ++total;
        }
        if (d.span != 0u && xl_bnd_next_rcp(d.bnd, rS, rD, d.ma + i) != nbref[d.ma + i]) return __LINE__;
        if (d.span != 0u && (i == 0u || i + 1u == n) && xl_bnd_next(d.bnd, d.ma + i) != nbref[d.ma + i]) return __LINE__;
      }
    }
    for (i = 0; i < V; ++i) {
      what[2] = i;
      if (oldm[i] != newm[i]) return __LINE__;
      if (newm[i]) {
        const uint32_t m = newm[i] - 1u;
        if (m >= K || seen[m] || m + shift != s * V + i) return __LINE__;
        seen[m] = 1;
      }
    }
  }
  if (total != K) return __LINE__;
  return 0;
}

/* every (j0_ref, delta) of a class and call shape; returns the failed line, out = {j0_ref, delta, s, g, i}.  The first pair of each
 * (own offset, shift) gets the full check; every other pair must have, for every segment and lane, the very duties of that first pair
 * (old and new, compared as structs), which is all the full check looks at. */
int sweep(uint32_t D, uint32_t M, uint32_t V, uint32_t S, uint32_t G, uint32_t *out) {
  static uint32_t rep[512][2][2];
  const XlPos p = pos_of(S, G);
  const uint32_t nseg = (xl_merge_points(D, p) + V - 1u) / V;
  uint32_t j0_ref, delta, s, g;
  if (D > 512u) return __LINE__;
  memset(rep, 0xFF, sizeof rep);
  for (j0_ref = 0; j0_ref < D; ++j0_ref)
    for (delta = 0; delta < D; ++delta) {
      uint32_t *const r = rep[xl_merge_j0(j0_ref, delta, D)][xl_merge_shift(j0_ref, delta, D)];
      out[0] = j0_ref, out[1] = delta;
      if (r[0] == 0xFFFFFFFFu) {
        const int line = column(D, M, V, S, G, j0_ref, delta, out + 2);
        if (line) return line;
        r[0] = j0_ref, r[1] = delta;
        continue;
      }
      for (s = 0; s < nseg; ++s)
        for (g = 0; g < M / XL_PH_STRIDE; ++g) {
          const XlGridDuty a = xl_grid_duty(j0_ref, delta, D, p, V, s, g, 0), b = xl_grid_duty(r[0], r[1], D, p, V, s, g, 0);
          const XlColDuty c = xl_col_duty(j0_ref, delta, D, p, V, s, g, 0), d = xl_col_duty(r[0], r[1], D, p, V, s, g, 0);
          out[2] = s, out[3] = g, out[4] = 0;
          if (memcmp(&a, &b, sizeof a) != 0 || memcmp(&c, &d, sizeof c) != 0) return __LINE__;
        }
    }
  return 0;
}

/* xl_div_rcp against the division: edge operands and n pseudo-random ones; returns the number of mismatches */
uint32_t div_check(uint32_t n) {
  static const uint32_t edge[] = {0u, 1u, 2u, 3u, 41u, 42u, 43u, 0x7FFFFFFFu, 0x80000000u, 0x80000001u, 0xFFFFFFFEu, 0xFFFFFFFFu, 65535u, 65536u, 65537u};
  const uint32_t ne = sizeof edge / sizeof edge[0];
  uint32_t bad = 0, i, k;
  uint64_t st = 0x9E3779B97F4A7C15ull;
  for (i = 0; i < ne; ++i)
    for (k = 1; k < ne; ++k) bad += xl_div_rcp(edge[i], edge[k], xl_rcp32(edge[k])) != edge[i] / edge[k];
  for (i = 0; i < n; ++i) {
    uint32_t x, d;
    st = st * 6364136223846793005ull + 1442695040888963407ull;
    x = (uint32_t)(st >> 32);
    st = st * 6364136223846793005ull + 1442695040888963407ull;
    d = (uint32_t)(st >> 32) >> (i % 32u);
    if (d == 0u) d = 1u;
    if (i % 3u == 0u) x = x / d * d - (i % 2u); /* around a multiple of d */
    bad += xl_div_rcp(x, d, xl_rcp32(d)) != x / d;
  }
  return bad;
}

/* ---- float32 models (compiled -ffp-contract=off: every operation rounded once) */
typedef struct { float x, y; } ph_t;
static ph_t nco_next(ph_t p, ph_t inc) { /* xl_nco_next */
  const float t1x = p.x * inc.x, t1y = p.y * inc.x, t2x = p.x * inc.y, t2y = p.y * inc.y;
  ph_t r = {t1x - t2y, t1y + t2x};
  return r;
}
static ph_t renorm(ph_t p) { /* xl_nco_renorm */
  const double mag2 = (double)p.x * (double)p.x + (double)p.y * (double)p.y;
  const float mag = (float)sqrt(mag2);
  ph_t r = {p.x / mag, p.y / mag};
  return r;
}
static int same(ph_t a, ph_t b) { return memcmp(&a, &b, sizeof a) == 0; }

/* xl_phase_walk on the phases it would store: compares instead; returns mismatches */
static uint32_t walk_cmp(ph_t p, uint32_t m0, uint32_t count, ph_t inc, XlBnd bnd, const ph_t *want, uint32_t *steps) {
  uint32_t m = m0 & ~(XL_PH_STRIDE - 1u), nb = xl_bnd_next(bnd, m), bad = 0;
  const uint32_t end = m0 + count;
  for (; m < end; ++m) {
    if (m >= m0) bad += !same(p, want[m]);
    p = nco_next(p, inc), ++*steps;
    if (m + 1u == nb) p = renorm(p), nb = xl_bnd_next(bnd, m + 1u);
  }
  return bad;
}

/* One column: the producer's chain over the call, then xl_phase_expand's control flow per segment (the ballot taken over the column's
 * lanes), each stored phase compared with the chain's.  force_slow: every lane takes xl_phase_walk.  Returns mismatches + violations of
 * the step bound; stats[0] += segments on the straight-line path, stats[1] += segments on the other, stats[2] += phases compared. */
uint32_t bits_check(uint32_t D, uint32_t M, uint32_t V, uint32_t S, uint32_t G, uint32_t j0_ref, uint32_t delta, float incx, float incy,
                    int force_slow, uint32_t *stats) {
  static ph_t want[MAXK];
  const XlPos pp = pos_of(S, G);
  const uint32_t GQ = M / XL_PH_STRIDE, extra = xl_grid_extra(M, V);
  const uint32_t rS = xl_rcp32(S), rD = xl_rcp32(D);
  const uint32_t nseg = (xl_merge_points(D, pp) + V - 1u) / V;
  const ph_t inc = {incx, incy};
  XlGridDuty du[16];
  uint32_t s, g, i, m, bad = 0;
  {
    const XlGridDuty d0 = xl_grid_duty(j0_ref, delta, D, pp, V, 0, 0, 0);
    ph_t p = {0.6f, -0.8f};
    uint32_t nb = xl_bnd_next(d0.bnd, 0);
    if (d0.bnd.K > MAXK) return 1u << 30;
    for (m = 0; m < d0.bnd.K; ++m) { /* xl_nco_client_chain */
      want[m] = p;
      p = nco_next(p, inc);
      if (m + 1u == nb) p = renorm(p), nb = xl_bnd_next(d0.bnd, m + 1u);
    }
  }
  for (s = 0; s < nseg; ++s) {
    int slow = force_slow, any = 0;
    for (g = 0; g < GQ; ++g) {
      const uint32_t n = XL_PH_STRIDE + (g == GQ - 1u ? extra : 0u);
      uint32_t iend;
      du[g] = xl_grid_duty(j0_ref, delta, D, pp, V, s, g, 0);
      iend = du[g].span - du[g].rel < n ? du[g].span - du[g].rel : n;
      any |= du[g].span != 0u;
      if (G > 1u && du[g].span != 0u && xl_bnd_next_rcp(du[g].bnd, rS, rD, du[g].ma) - du[g].ma < iend) slow = 1;
    }
    if (!any) continue;
    stats[slow ? 1 : 0]++;
    for (g = 0; g < GQ; ++g) {
      const XlGridDuty d = du[g];
      const int last = g == GQ - 1u;
      const uint32_t n = XL_PH_STRIDE + (last ? extra : 0u);
      const uint32_t iend = d.span - d.rel < n ? d.span - d.rel : n;
      uint32_t steps = 0;
      ph_t p = want[d.tab * XL_PH_STRIDE]; /* the table entry (entry 0 where there is nothing to store) */
      if (!slow) {
        if (d.rel < d.span) bad += !same(p, want[d.ma]), stats[2]++;
        for (i = 1; i < XL_PH_STRIDE; ++i) {
          p = nco_next(p, inc), ++steps;
          if (d.rel + i < d.span) bad += !same(p, want[d.ma + i]), stats[2]++;
        }
        for (i = 0; i < extra; ++i) {
          p = nco_next(p, inc), ++steps;
          if (last && d.rel + XL_PH_STRIDE + i < d.span) bad += !same(p, want[d.ma + XL_PH_STRIDE + i]), stats[2]++;
        }
      } else if (d.span != 0u) {
        const uint32_t i0 = (int32_t)d.rel < 0 ? 0u - d.rel : 0u;
        bad += walk_cmp(p, d.ma + i0, iend - i0, inc, d.bnd, want, &steps);
        stats[2] += iend - i0;
      }
      if (steps > XL_PH_STRIDE + extra) ++bad;
    }
  }
  return bad;
}
"""

DS = (8, 21, 42, 100)
CLASSES = [(64, 33), (64, 52), (64, 63), (128, 65), (128, 116), (128, 127), (256, 129), (256, 244), (256, 255)]


def call_shapes(D, V):
    """(G, S) of the sweep: one block; two blocks of about 2.3 V outputs, the second one's first output moved through 16 consecutive
    indices; eight blocks of about 0.6 V outputs (a block end in most segments), moved in steps of 5."""
    shapes = [(1, D * (3 * V + 7) + 3)]
    shapes += [(2, D * (2 * V + V // 3 + r) + 5) for r in range(16)]
    shapes += [(8, D * (V // 2 + V // 9 + r) + 1) for r in (0, 5, 10, 15)]
    return shapes


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("phase_expand")
    src = d / "shim.c"
    src.write_text(SHIM)
    so = d / "libphase_expand.so"
    extra = os.environ.get("XL_SANITIZE_CFLAGS", "").split()  # (tools/sanitize.sh: -fsanitize=address,undefined)
    subprocess.run(["gcc", "-O3", "-ffp-contract=off", "-Wall", "-Werror", "-shared", "-fPIC"] + extra +
                   ["-I", CSRC, str(src), "-o", str(so), "-lm"], check=True)
    L = C.CDLL(str(so))
    L.sweep.restype = C.c_int
    L.sweep.argtypes = [C.c_uint32] * 5 + [C.POINTER(C.c_uint32)]
    L.div_check.restype = C.c_uint32
    L.div_check.argtypes = [C.c_uint32]
    L.bits_check.restype = C.c_uint32
    L.bits_check.argtypes = [C.c_uint32] * 7 + [C.c_float, C.c_float, C.c_int, C.POINTER(C.c_uint32)]
    return L


def test_reciprocal_division_is_exact(lib):
    assert lib.div_check(2000000) == 0


def test_block_ends_reach_every_residue():
    """The lengths of call_shapes() do what their docstring says: over the 16 two-block lengths the second block's first output takes
    16 consecutive indices for every offset j0, so every residue mod 16 -- every step of a lane's walk -- meets a block end."""
    for D in DS:
        for _, V in CLASSES:
            for j0 in (0, D // 2, D - 1):
                nbs = sorted((S - j0 + D - 1) // D for G, S in call_shapes(D, V) if G == 2)
                assert nbs == list(range(nbs[0], nbs[0] + 16)), (D, V, j0)


@pytest.mark.parametrize("D", DS)
def test_grid_duties_store_what_the_column_duties_stored(lib, D):
    out = (C.c_uint32 * 5)()
    for M, V in CLASSES:
        for G, S in call_shapes(D, V):
            line = lib.sweep(D, M, V, S, G, out)
            assert line == 0, "shim line %d: D %d M %d V %d S %d G %d j0_ref %d delta %d segment %d lane %d step %d" % (
                (line, D, M, V, S, G) + tuple(out))


@pytest.mark.parametrize("D", DS)
def test_walk_gives_the_chain_s_bits(lib, D):
    stats = (C.c_uint32 * 3)()
    incs = [(0.99939084, -0.03489950), (-0.70710677, 0.70710677)]  # (rounded to float32 by the call; |inc| near 1)
    pairs = sorted({(0, 0), (0, D - 1), (D - 1, 1), (D // 2, D // 2), (D // 3, D - 1 - D // 3), (D - 1, D - 1), (1, D // 2)})
    for M, V in CLASSES:
        for G, S in call_shapes(D, V):
            for n, (j0_ref, delta) in enumerate(pairs):
                ix, iy = incs[n % 2]
                for force_slow in (0, 1):
                    bad = lib.bits_check(D, M, V, S, G, j0_ref, delta, ix, iy, force_slow, stats)
                    assert bad == 0, (D, M, V, S, G, j0_ref, delta, force_slow, bad)
    assert stats[0] > 0 and stats[1] > 0 and stats[2] > 0, list(stats)  # both paths were taken
