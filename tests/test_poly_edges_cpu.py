"""CPU tests of tests/poly_edges.py: (a) its restatement of the merged-class arithmetic is pinned to sdr-server_amd/csrc/xl_grid.h itself
(compiled with gcc behind a shim, as tests/test_grid.py does) and to brute force; (b) for every shape and transform length the call
sequences it chose hold every call-length edge of the segment grid, each case asserted on the call that is NAMED for it -- a later
change of V, of a length or of the protocol fails here, not silently on the GPU (tests/test_poly_edges_gpu.py runs the same
sequences against the oracle)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import poly_edges as pe

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sdr-server_amd", "csrc")

SHIM = r"""
#include "xl_grid.h"
uint32_t g_merge_j0(uint32_t j0_ref, uint32_t delta, uint32_t D) { return xl_merge_j0(j0_ref, delta, D); }
uint32_t g_merge_shift(uint32_t j0_ref, uint32_t delta, uint32_t D) { return xl_merge_shift(j0_ref, delta, D); }
uint32_t g_merge_points(uint32_t D, uint32_t S, uint32_t G) { XlPos p = {0, S, G, 0}; return xl_merge_points(D, p); }
uint32_t g_merge_outputs(uint32_t j0_ref, uint32_t delta, uint32_t D, uint32_t S, uint32_t G) {
  XlPos p = {0, S, G, 0};
  return xl_merge_outputs(j0_ref, delta, D, p);
}
uint32_t g_mstart(uint32_t j0, uint32_t D, uint32_t S, uint32_t g) { return xl_grid_mstart(j0, D, S, g); }
void g_dyn(uint32_t D, uint32_t T, uint32_t rem0, uint32_t hv0, uint32_t trel, uint32_t S, uint32_t G, uint32_t *out) {
  XlPos p = {trel, S, G, 0};
  XlDyn d = xl_grid_dyn(D, T, rem0, hv0, p);
  out[0] = d.K; out[1] = d.j0;
}
"""


@pytest.fixture(scope="module")
def grid(tmp_path_factory):
    d = tmp_path_factory.mktemp("poly_edges_grid")
    src = d / "shim.c"
    src.write_text(SHIM)
    so = d / "libgrid.so"
    extra = os.environ.get("XL_SANITIZE_CFLAGS", "").split()  # (tools/sanitize.sh: -fsanitize=address,undefined)
    subprocess.run(["gcc", "-O1", "-Wall", "-Werror", "-shared", "-fPIC"] + extra + ["-I", CSRC, str(src), "-o", str(so)], check=True)
    L = C.CDLL(str(so))
    for n, k in (("g_merge_j0", 3), ("g_merge_shift", 3), ("g_merge_points", 3), ("g_merge_outputs", 5), ("g_mstart", 4)):
        getattr(L, n).restype = C.c_uint32
        getattr(L, n).argtypes = [C.c_uint32] * k
    L.g_dyn.argtypes = [C.c_uint32] * 7 + [C.POINTER(C.c_uint32)]
    return L


# ---------------------------------------------------------------------------------------------------------------
# (a) the restatement against the header
def _sweep():
    """(D, S, G, consumed of the reference member, consumed of another member): random ones, and every (S G mod D, offset) of small D"""
    rng = np.random.default_rng(41)
    for _ in range(1500):
        D = int(rng.integers(1, 420))
        G = int(rng.choice([1, 1, 2, 3, 8]))
        S = int(rng.integers(max(D, 1), 70000))
        yield D, S, G, int(rng.integers(0, 1 << 20)), int(rng.integers(0, 1 << 20))
    for D in (1, 2, 3, 8):
        for S in range(D, 4 * D + 1):
            for G in (1, 2, 3):
                for a in range(D):
                    for b in range(D):
                        yield D, S, G, 5 * D + a, b


def test_restatement_matches_the_header_and_brute_force(grid):
    """xl_merge_points / xl_merge_outputs / xl_merge_shift / xl_merge_j0 / xl_grid_mstart and the K, j0 of xl_grid_dyn: the header's
    value == poly_edges' == brute force (outputs are the multiples of D in the client's stream; a member's output k is the shared
    point k + shift, whose newest sample lies at j0_ref - D + (k + shift) D + delta)."""
    out = (C.c_uint32 * 2)()
    n = 0
    for D, S, G, ca, cb in _sweep():
        N = S * G
        j0_ref, j0_c = pe.grid_j0(ca, D), pe.grid_j0(cb, D)
        delta = (j0_c - j0_ref) % D
        Kq = grid.g_merge_points(D, S, G)
        assert Kq == pe.merge_points(D, S, G) == -(-N // D) + 1
        assert grid.g_merge_j0(j0_ref, delta, D) == pe.merge_j0(j0_ref, delta, D) == j0_c
        shift = grid.g_merge_shift(j0_ref, delta, D)
        assert shift == pe.merge_shift(j0_ref, delta, D) == (0 if j0_c < j0_ref else 1)
        K = grid.g_merge_outputs(j0_ref, delta, D, S, G)
        brute = len(range(-(-cb // D) * D, cb + N, D))  # multiples of D in [cb, cb + N)
        assert K == pe.merge_outputs(j0_ref, delta, D, S, G) == pe.grid_outputs(cb, D, S, G) == brute
        grid.g_dyn(D, 1, cb % D, 0, 0, S, G, out)
        assert (out[0], out[1]) == (K, j0_c)
        # every output of the member is a shared point below Kq, at the member's own sample
        for k in {0, K - 1} - {-1}:
            q = k + shift
            assert q < Kq and j0_ref - D + q * D + delta == j0_c + k * D
        for g in range(G + 1):
            assert grid.g_mstart(j0_c, D, S, g) == pe.grid_mstart(j0_c, D, S, g) == len(range(-(-cb // D) * D, cb + g * S, D))
        n += 1
    assert n > 2000


# ---------------------------------------------------------------------------------------------------------------
# (b) the sequences
CASES = [(name, M) for name, sh in sorted(pe.SHAPES.items()) for M in sh.Ms]


def _recs(shape, M, seq):
    calls = pe.sequences(shape, M)[seq]
    recs = pe.walk(shape, M, calls, second=(seq == "thresh" and shape.second is not None))
    assert len({c.name for c in calls}) == len(calls)
    return {r.call.name: r for r in recs}, recs


@pytest.mark.parametrize("name,M", CASES)
def test_protocol_assumptions(name, M):
    """What `walk` takes for granted about the plan (xl_plan.cpp): the first offset does not change the taps per branch, the class
    fits the transform, cohort A's grid is the reference (its largest delay r is the smaller one), both cohorts are mature when they
    merge, blocks of a multi-block call hold an output of every client, and no call exceeds its engine or its segment capacity."""
    sh = pe.SHAPES[name]
    A = pe.taps_per_branch(sh.T, sh.D, sh.r)
    assert 0 < sh.r < sh.D - sh.r and A == pe.taps_per_branch(sh.T, sh.D) and 2 <= A <= M // 2
    V = pe.valid_points(M, sh.T, sh.D, sh.r)
    assert V == M - A + 1 and V > 2 * pe.XL_PH_STRIDE
    if sh.second:
        D2, T2, _ = sh.second
        A2 = pe.taps_per_branch(T2, D2)
        assert 2 <= A2 <= M // 2 and D2 <= 504
        assert (7 * D2 + -(-T2 // 12) * 12) * 8 <= 160 * 1024 and T2 - 1 + D2 <= 16384  # (xl_wide.h: an LDS tile holds its window)
    assert set(pe.SEQUENCES_OF[name]) <= set(pe.sequences(sh, M))
    for seq in pe.SEQUENCES_OF[name]:
        by, recs = _recs(sh, M, seq)
        cap_s, gcap = pe.engine_limits([r.call for r in recs])
        assert recs[0].call.G == 1 and recs[0].call.S * 1 % sh.D == sh.r
        assert recs[0].call.S >= sh.T - 1 and recs[1].call.S * recs[1].call.G >= sh.T - 1  # mature behind their first call
        if sh.second and seq == "thresh":
            assert recs[0].call.S >= sh.second[1] - 1
        assert pe.LEAVE_AFTER >= 2 and pe.LEAVE_AFTER + 1 < len(recs) and pe.NA > pe.NB and pe.NA + pe.NB - 1 > 32
        assert sum(r.call.variant == "native" for r in recs) == 1
        for r in recs:
            c = r.call
            assert 1 <= c.G <= gcap and c.S <= cap_s and (c.G == 1 or c.S >= sh.D)
            assert r.nseg <= pe.nseg_cap(cap_s * gcap, sh.D, V) - 1, (seq, c.name)  # never -EIO
            if r.merged:
                assert r.delta_b == sh.r and r.shift_a == 1
                assert r.k_a == pe.merge_outputs(r.j0_ref, 0, sh.D, c.S, c.G) and r.k_b == pe.merge_outputs(r.j0_ref, r.delta_b, sh.D, c.S, c.G)
            if c.quiet and sh.fmt == "cf32":  # (the passages exist in cf32 streams only)
                assert r.poly and r.nseg >= 3  # (a loud segment in front of the quiet pair)
                lo, hi = pe.quiet_span(sh, M, r)
                assert hi <= c.S * c.G and lo > (c.G - 1) * c.S + sh.T or (c.quiet == "head" and lo == 0 and hi + sh.T < c.S)
        # a "head" call directly follows a "tail" call: its segment 0 (an even entry of the pair of segment scales) holds nothing loud,
        # its segment 1 (the odd entry) is loud
        for a, b in zip(recs, recs[1:]):
            if b.call.quiet == "head":
                assert a.call.quiet == "tail" and b.nseg >= 2
        if name in ("B", "C"):
            assert {r.call.quiet for r in recs} >= {"tail", "head"}
            tails = [r for r in recs if r.call.quiet == "tail"]
            for r in tails:  # the passage covers every sample the last two segments read
                lo, hi = pe.quiet_span(sh, M, r)
                assert lo <= (r.nseg - 2) * V * sh.D + r.j0_ref - sh.D - (sh.T - 1) and hi == r.call.S * r.call.G
            if seq == "edges":
                assert {r.nseg % 2 for r in tails} == {0, 1}  # the quiet pair starts on an even and on an odd segment


@pytest.mark.parametrize("name,M", CASES)
def test_edges_sequence_holds_cases_1_2_3_6_8(name, M):
    sh = pe.SHAPES[name]
    V = pe.valid_points(M, sh.T, sh.D, sh.r)
    by, recs = _recs(sh, M, "edges")
    # case 1: Kq = 0, 1, 2, V - 1 (mod V)
    assert by["warm"].Kq % V == 2 and by["cap"].Kq % V == 2
    assert by["full16"].Kq % V == 0 and by["n15"].Kq % V == 0
    assert by["one-mult"].Kq % V == 1 and by["one-rem"].Kq % V == 1
    assert by["vm1"].Kq % V == V - 1 and by["vm1"].last_points == V - 1
    # case 2: the single point of the last segment, in a class with members at two offsets
    om, orr = by["one-mult"], by["one-rem"]
    for r in (om, orr):
        assert r.merged and r.poly and r.last_points == 1 and r.nseg == pe.XLP_SEG + 1 and r.passes == 2
    assert om.call.S % sh.D == 0 and (om.shift_a, om.shift_b) == (1, 0) and om.k_a == om.k_b == om.Kq - 1
    assert om.k_a - 1 + om.shift_a == om.Kq - 1 and om.k_b - 1 + om.shift_b == om.Kq - 2  # cohort A owns the point, cohort B does not
    assert orr.call.S % sh.D != 0 and (orr.shift_a, orr.shift_b) == (1, 0) and orr.k_b == orr.k_a + 1  # K and K + 1 outputs
    assert orr.k_a - 1 + orr.shift_a == orr.Kq - 2 and orr.k_b - 1 + orr.shift_b == orr.Kq - 2         # ... and the point is nobody's
    # case 3: nseg = 0, 1, 15 (mod 16), both parities; the last pass of one segment
    assert by["full16"].nseg == 16 and by["full16"].passes == 1 and by["vm1"].nseg == 16
    assert om.nseg % pe.XLP_SEG == 1 and by["n15"].nseg == 15
    assert {r.nseg % 2 for r in recs if r.poly} == {0, 1}
    # case 6: the largest call the engine admits, and the one a sample shorter
    cap_s, gcap = pe.engine_limits([r.call for r in recs])
    assert gcap == 1 and by["cap"].call.S == cap_s and om.call.S == cap_s - 1
    assert by["cap"].nseg == 17 and pe.nseg_cap(cap_s * gcap, sh.D, V) == 18
    # case 8: successive lengths differ mod D, the reference grid moves between the cases
    assert len({r.call.S % sh.D for r in recs}) >= 4 and len({r.j0_ref for r in recs if r.merged}) >= 4
    assert all(r.poly for r in recs if r.call.variant == "optimized")
    if sh.fmt == "cf32":
        assert orr.call.quiet == "tail" and by["vm1"].call.quiet == "tail" and by["n15"].call.quiet == "head"


@pytest.mark.parametrize("name,M", [c for c in CASES if "thresh" in pe.SEQUENCES_OF[c[0]]])
def test_threshold_sequence_holds_cases_4_5(name, M):
    sh = pe.SHAPES[name]
    by, recs = _recs(sh, M, "thresh")
    # case 5: 512 is polyphase, 511 direct, in one sequence with polyphase calls on both sides
    a, b, c = by["k512"], by["k511"], by["k512-some"]
    assert (a.k_a, a.k_b, a.max_k, a.poly) == (512, 512, 512, True)
    assert (b.k_a, b.k_b, b.max_k, b.poly) == (511, 511, 511, False)
    assert (c.k_a, c.k_b, c.max_k, c.poly) == (511, 512, 512, True)
    names = [r.call.name for r in recs]
    assert names.index("k520") < names.index("k512") < names.index("k511") < names.index("k512-some") < names.index("k512-again")
    assert [r.poly for r in recs] == [r.call.name not in ("k511", "native") for r in recs]
    assert all(r.merged for r in (a, b, c))
    # case 4: a second class whose whole call is a fraction of one segment, beside the class that carries the call over the threshold
    if sh.second:
        for r in recs:
            assert r.nseg2 == 1 and 2 <= r.Kq2 <= 16, (r.call.name, r.Kq2)
        assert len({r.Kq2 for r in recs}) >= 2
    else:
        assert name == "C"  # (poly_edges.SHAPES says why it has none)
    cap_s, gcap = pe.engine_limits([r.call for r in recs])
    assert gcap == 1 and by["warm"].call.S == cap_s  # (this engine's capacity call)


@pytest.mark.parametrize("G", [2, 3])
@pytest.mark.parametrize("name,M", [c for c in CASES if "g2" in pe.SEQUENCES_OF[c[0]]])
def test_group_sequences_hold_cases_6_7(name, M, G):
    sh = pe.SHAPES[name]
    V = pe.valid_points(M, sh.T, sh.D, sh.r)
    by, recs = _recs(sh, M, "g%d" % G)
    pts = {n: pe.inner_block_points(sh, M, r) for n, r in by.items() if r.merged}
    for n in ("sV", "sV-1", "sV+1", "sV-2", "sV+16", "sV+15"):
        r = by[n]
        assert r.call.G == G and r.merged and r.poly and (r.shift_a, r.shift_b) == (1, 0), n
    # case 7: an inner block's first output on shared point sV, sV + 1, sV + V - 1 and sV + 16 g, for both shift values
    assert {(0, 0), (1, 1)} <= pts["sV"]
    assert {(0, V - 1), (1, 0)} <= pts["sV-1"]
    assert (0, 1) in pts["sV+1"] and (1, V - 1) in pts["sV-2"]
    assert (0, pe.XL_PH_STRIDE) in pts["sV+16"] and (1, pe.XL_PH_STRIDE) in pts["sV+15"]
    # case 6: S = max_input with G = group_blocks, and a sample less per block
    cap_s, gcap = pe.engine_limits([r.call for r in recs])
    assert gcap == G and (by["sV+16"].call.S, by["sV+16"].call.G) == (cap_s, G) and (by["cap-1"].call.S, by["cap-1"].call.G) == (cap_s - 1, G)
    assert by["cap-1"].poly and by["sV+16"].nseg <= pe.nseg_cap(cap_s * G, sh.D, V) - 1
    assert [r.poly for r in recs[1:]] == [r.call.variant == "optimized" for r in recs[1:]] and not recs[0].poly


@pytest.mark.parametrize("name,M", CASES)
def test_forward_launch_form(name, M):
    """Which calls give the forward launch its grouped form (cf32 streams, 96 workgroups of four branches): every optimized call of shape
    C's sequence "long" behind the warm-up -- four and five passes, with the one-point last pass and four full passes among them --
    and no other call of any shape: with D = 8 the form would need 48 passes per call."""
    sh = pe.SHAPES[name]
    V = pe.valid_points(M, sh.T, sh.D, sh.r)
    for seq in pe.SEQUENCES_OF[name]:
        by, recs = _recs(sh, M, seq)
        for r in recs:
            want = seq == "long" and r.poly and r.call.name != "warm"
            assert pe.forward_grouped(sh.fmt, sh.D, M, r.nseg) == want, (seq, r.call.name, r.nseg)
    if "long" not in pe.SEQUENCES_OF[name]:
        return
    by, recs = _recs(sh, M, "long")
    assert (by["p4-one-mult"].nseg, by["p4-one-mult"].passes, by["p4-one-mult"].last_points) == (49, 4, 1)
    assert (by["p4-one-rem"].nseg, by["p4-one-rem"].last_points, by["p4-one-rem"].k_b - by["p4-one-rem"].k_a) == (49, 1, 1)
    assert by["p4-one-mult"].k_a - 1 + 1 == by["p4-one-mult"].Kq - 1 and by["p4-one-rem"].k_b - 1 == by["p4-one-rem"].Kq - 2
    assert (by["p4-full"].nseg, by["p4-full"].last_points) == (64, V) and (by["cap"].nseg, by["cap-1"].nseg, by["cap-1"].last_points) == (65, 65, 1)
    cap_s, gcap = pe.engine_limits([r.call for r in recs])
    assert gcap == 1 and by["cap"].call.S == cap_s and by["cap-1"].call.S == cap_s - 1 and pe.nseg_cap(cap_s, sh.D, V) == 66
    assert by["p4-one-rem"].call.quiet == "tail" and by["p4-full"].call.quiet == "head"
