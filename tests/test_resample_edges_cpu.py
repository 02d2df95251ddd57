"""CPU tests (-m "not gpu") of tests/resample_edges.py: that every stream of its table takes the paths of the resampler banks' kernels
it is meant to take, under the exact piece lists tests/test_resample_edges_gpu.py feeds -- which tiles stage their window in LDS and
which read it in place, the spans 4096 and 4097 on the two sides of the limit, the path that flips with the split -- that the Q15
streams' tap tables and sums are on the side of their limits they are meant to be on, and that the restated cut is
xl_resample_cut.h's, compiled by gcc, for every (case, piece).

Nothing here observes the kernel: which branch a tile takes is computed by resample_edges.tile_paths, a restatement of xl_rs_tile
(xl_resample_dev.h) with the constants parsed from the headers.  The library holds no counter of the paths, by intent."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import resample_edges as E
import resample_q15_ref as QR
import resample_ref as RR

LIMIT = 4096  # what the table below was computed for; the headers' values are asserted against it first


def paths(name, pieces, bank="f"):
    """-> [[(nv, span, path) per tile] per feed] of a case under one of its piece lists"""
    c = E.CASE[name]
    return E.feed_paths(c.L, c.M, E.taps_per_phase(c), c.pieces[pieces], E.span_limit(bank))


def test_the_constants_are_the_headers():
    assert E.CONST == {"XL_RS_TILE": 256, "XL_RS_LDS_SPAN": LIMIT, "XL_RSQ_LDS_SPAN": LIMIT, "XL_RSQ_LDS_TAPS": 4096}
    # the kernels compare against these names and nothing else
    csrc = E.CSRC
    assert "t.span <= XL_RS_LDS_SPAN" in open(os.path.join(csrc, "xl_resample.hip")).read()
    q15 = open(os.path.join(csrc, "xl_resample_q15.hip")).read()
    assert "t.span <= XL_RSQ_LDS_SPAN" in q15 and "ntaps <= XL_RSQ_LDS_TAPS" in q15
    dev = open(os.path.join(csrc, "xl_resample_dev.h")).read()
    assert "t.span = (uint64_t)(t.nv - 1u) * Mq + ul / r.L + r.Q;" in dev and "ul = pt + (t.nv - 1u) * Mr" in dev
    assert "t.nv = min(XL_RS_TILE, r.nout - t.k0);" in dev


def test_the_table_is_well_formed():
    assert [c.name for c in E.CASES] == ["1/16 Q16", "1/16 Q17", "1/40 Q64", "3/50 Q40", "4/61 Q208", "5/81 Q1000", "5/81 Q1000 half",
                                         "1/40 wide", "4096/(2^31-1) Q3", "1/(2^31-1) Q5"]
    assert E.M_MAX == 2 ** 31 - 1
    for c in E.CASES:
        Q = E.taps_per_phase(c)
        assert math.gcd(c.L, c.M) == 1 and 1 <= c.L <= 4096 and c.M < 2 ** 31 and Q <= 1024
        m = re.match(r"(\d+)/(\d+|\(2\^31-1\))( Q(\d+))?", c.name)
        assert int(m.group(1)) == c.L and (m.group(2) == "(2^31-1)" and c.M == E.M_MAX or int(m.group(2)) == c.M)
        assert m.group(4) is None or int(m.group(4)) == Q
        assert list(c.pieces)[:2] == ["whole", "edge"] and len(c.pieces) >= 2
        assert c.pieces["whole"] == [c.N] and c.pieces["edge"][:4] == [Q - 1, 1, 300, 4097]
        assert all(sum(p) == c.N for p in c.pieces.values())
        assert c.taps.dtype == np.float32 and c.N * 8 <= 11 * 2 ** 20  # the largest input is about 10 MB
    assert E.FLOAT_CASES == ["1/16 Q16", "1/16 Q17", "1/40 Q64", "3/50 Q40", "4/61 Q208", "4096/(2^31-1) Q3", "1/(2^31-1) Q5"]
    assert E.Q15_CASES == ["1/16 Q16", "1/16 Q17", "3/50 Q40", "4/61 Q208", "5/81 Q1000", "5/81 Q1000 half", "1/40 wide",
                           "4096/(2^31-1) Q3", "1/(2^31-1) Q5"]


# ------------------------------------------------------------------------------------------------------------ the paths, fed whole
# name -> [(nv, span, path) per tile] of the one feed
WHOLE = {
    "1/16 Q16": [(256, 4096, "lds")] * 4 + [(226, 3616, "lds")],            # exactly the limit: all 5 tiles in LDS
    "1/16 Q17": [(256, 4097, "mem")] * 4 + [(226, 3617, "lds")],            # one past it; both paths in one launch
    "1/40 Q64": [(256, 10264, "mem")] * 2 + [(238, 9544, "mem")],
    "3/50 Q40": [(256, 4290, "mem")] * 7 + [(8, 157, "lds")],               # M % L != 0 in place
    "4/61 Q208": [(256, 4096, "lds")] * 7 + [(176, 2876, "lds")],           # every tile starts at phase 0
    "5/81 Q1000": [(256, 5131, "mem")] * 7 + [(60, 1956, "lds")],
    "5/81 Q1000 half": [(256, 5131, "mem")] * 7 + [(60, 1956, "lds")],
    "1/40 wide": [(256, 10264, "mem")] * 2 + [(238, 9544, "mem")],
    "4096/(2^31-1) Q3": [(3, 1048578, "mem")],                              # 3 outputs, 524288 inputs apart but for one
    "1/(2^31-1) Q5": [(1, 5, "lds")],                                       # output 0 only
}


@pytest.mark.parametrize("name", list(E.CASE))
def test_paths_of_the_whole_feed(name):
    for bank in E.CASE[name].banks:
        assert paths(name, "whole", bank) == [WHOLE[name]], (name, bank)
    assert set(WHOLE) == set(E.CASE)


# ------------------------------------------------------------------------------------------------------------ the paths, in pieces
# name -> [[(nv, span, path) per tile] per feed] under the "edge" pieces [Q - 1, 1, 300, 4097, rest]
EDGE = {
    "1/16 Q16": [[(1, 16, "lds")], [], [(19, 304, "lds")], [(256, 4096, "lds")], [(256, 4096, "lds")] * 3 + [(206, 3296, "lds")]],
    "1/16 Q17": [[(1, 17, "lds")], [(1, 17, "lds")], [(18, 289, "lds")], [(256, 4097, "mem")],
                 [(256, 4097, "mem")] * 3 + [(206, 3297, "lds")]],
    "1/40 Q64": [[(2, 104, "lds")], [], [(8, 344, "lds")], [(102, 4104, "mem")], [(256, 10264, "mem")] * 2 + [(126, 5064, "mem")]],
    "3/50 Q40": [[(3, 73, "lds")], [], [(18, 323, "lds")], [(246, 4123, "mem")], [(256, 4290, "mem")] * 5 + [(253, 4240, "mem")]],
    "4/61 Q208": [[(14, 406, "lds")], [], [(20, 498, "lds")], [(256, 4097, "mem"), (12, 376, "lds")],
                  [(256, 4097, "mem")] * 6 + [(130, 2175, "lds")]],
    "5/81 Q1000": [[(62, 1988, "lds")], [], [(19, 1292, "lds")], [(253, 5082, "mem")], [(256, 5131, "mem")] * 5 + [(238, 4840, "mem")]],
    "1/40 wide": [[(2, 104, "lds")], [], [(8, 344, "lds")], [(102, 4104, "mem")], [(256, 10264, "mem")] * 2 + [(126, 5064, "mem")]],
    "4096/(2^31-1) Q3": [[(1, 3, "lds")], [], [], [], [(2, 524291, "mem")]],
    "1/(2^31-1) Q5": [[(1, 5, "lds")], [], [], [], []],
}
EDGE["5/81 Q1000 half"] = EDGE["5/81 Q1000"]
# ... and under the split chosen to flip the path
FLIP = {
    # from phase 1 on a full tile spans 255 * 15 + (1 + 255) / 4 + 208 = 4097: the outputs the whole feed computes from LDS
    "4/61 Q208": [[(1, 208, "lds")], [(256, 4097, "mem")] * 7 + [(175, 2861, "lds")]],
    # the second feed consumes 5000 samples, moves the carry and has no output: a run without workgroups
    "1/(2^31-1) Q5": [[(1, 5, "lds")], []],
}


@pytest.mark.parametrize("name", list(E.CASE))
def test_paths_of_the_pieces(name):
    c = E.CASE[name]
    for bank in c.banks:
        assert paths(name, "edge", bank) == EDGE[name], (name, bank)
        assert ("flip" in c.pieces) == (name in FLIP)
        if name in FLIP:
            assert paths(name, "flip", bank) == FLIP[name], (name, bank)
    assert set(EDGE) == set(E.CASE)


def test_the_cells_of_the_table():
    """the sentences of the table, one by one (the lists above hold them too; here they are spelt out)"""
    kinds = lambda name, pieces: [[t[2] for t in feed] for feed in paths(name, pieces)]
    spans = lambda name, pieces: {t[1] for feed in paths(name, pieces) for t in feed if t[0] == E.TILE}
    assert spans("1/16 Q16", "whole") == {LIMIT} and kinds("1/16 Q16", "whole") == [["lds"] * 5]
    assert spans("1/16 Q17", "whole") == {LIMIT + 1} and kinds("1/16 Q17", "whole") == [["mem"] * 4 + ["lds"]]
    assert paths("1/16 Q17", "whole")[0][-1][:2] == (226, 3617)
    assert kinds("1/40 Q64", "whole") == [["mem"] * 3] and spans("1/40 Q64", "whole") == {10264}
    assert 50 % 3 != 0 and kinds("3/50 Q40", "whole") == [["mem"] * 7 + ["lds"]] and spans("3/50 Q40", "whole") == {4290}
    assert paths("3/50 Q40", "whole")[0][-1][0] == 8
    # the phase-dependent path: the same outputs, all in LDS fed whole, 7 full tiles in place behind a first piece of one sample
    assert (61 // 4, 61 % 4) == (15, 1)
    assert kinds("4/61 Q208", "whole") == [["lds"] * 8] and spans("4/61 Q208", "whole") == {LIMIT}
    assert E.CASE["4/61 Q208"].pieces["flip"] == [1, 29999]
    assert kinds("4/61 Q208", "flip") == [["lds"], ["mem"] * 7 + ["lds"]] and spans("4/61 Q208", "flip") == {LIMIT + 1}
    # M at its limit
    c = E.CASE["4096/(2^31-1) Q3"]
    assert RR.counts(c.L, c.M, c.N) == 3 and [int(v) for v in RR.positions(c.L, c.M, np.arange(3))[0]] == [0, 524287, 1048575]
    assert paths(c.name, "whole") == [[(3, 1048578, "mem")]]
    c = E.CASE["1/(2^31-1) Q5"]
    assert c.pieces["flip"] == [1000, 5000] and RR.counts(c.L, c.M, 1000) == 1 == RR.counts(c.L, c.M, 6000)
    assert E.cut(c.L, c.M, 5, 1000, 5000) == (1, 0, 2 ** 31 - 1 - 1000, 0)  # n_first approaches 2^31 and still fits the run's int32


# ------------------------------------------------------------------------------------------------------------ the Q15 streams
def test_q15_tables_and_sums():
    facts = {}
    for name in E.Q15_CASES:
        c = E.CASE[name]
        Q = E.taps_per_phase(c)
        q = QR.quantize(c.taps)  # (raises where xlating_resample_q15_quantize answers -ERANGE)
        assert q.size == c.taps.size and np.abs(q).max() > 0
        facts[name] = (c.L * Q, int(QR.phase_abs_sums(c.L, c.taps).min()), int(QR.phase_abs_sums(c.L, c.taps).max()))
    taps_limit = E.CONST["XL_RSQ_LDS_TAPS"]
    for name in ("1/16 Q16", "1/16 Q17", "3/50 Q40", "4/61 Q208", "1/(2^31-1) Q5"):
        assert facts[name][0] <= taps_limit and facts[name][2] <= 65535, name  # table in LDS, 32-bit sums
    # table and window both in place: with 64-bit sums, and at half the gain with 32-bit sums
    assert facts["5/81 Q1000"][0] == 5000 > taps_limit and facts["5/81 Q1000"][1] > 65535
    assert facts["5/81 Q1000 half"][0] == 5000 > taps_limit and facts["5/81 Q1000 half"][2] <= 65535
    # 64-bit sums over an in-place window, the table in LDS
    assert facts["1/40 wide"] == (64, 64 * 32440, 64 * 32440) and 64 * 32440 > 65535
    assert facts["4096/(2^31-1) Q3"][0] == 12288 > taps_limit and facts["4096/(2^31-1) Q3"][2] > 65535


def test_q15_restatement_is_not_trivial():
    """the streams' expected outputs are neither all zero nor all clipped on full-range input (a condition on the inputs)"""
    rng = np.random.default_rng(2)
    for name in E.Q15_CASES:
        c = E.CASE[name]
        n = min(c.N, 4000) if c.M < 4096 else c.N
        x = rng.integers(-32768, 32768, (n, 2)).astype(np.int16)
        y = QR.restate(c.L, c.M, c.taps, x)
        assert (y != 0).any(), name
        if y.shape[0] > 3:
            assert ((y > -32768) & (y < 32767)).any(), name


# ------------------------------------------------------------------------------------------------------------ the cut
SHIM = r"""
#include "xl_resample_cut.h"
void cut(uint32_t L, uint32_t M, uint32_t Q, uint64_t P0, uint64_t n, int64_t *o) {
  XlResampleCut c = xl_resample_cut(L, M, Q, P0, n);
  o[0] = (int64_t)c.m_first, o[1] = (int64_t)c.count, o[2] = c.n_first, o[3] = c.p_first;
}
"""


@pytest.fixture(scope="module")
def cutlib(tmp_path_factory):
    d = tmp_path_factory.mktemp("rsedges")
    src = d / "shim.c"
    src.write_text(SHIM)
    so = d / "librsedges.so"
    subprocess.run(["gcc", "-O1", "-Wall", "-Werror", "-shared", "-fPIC", "-I", E.CSRC, str(src), "-o", str(so)], check=True)
    lib = C.CDLL(str(so))
    lib.cut.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, C.POINTER(C.c_int64)]
    lib.cut.restype = None
    return lib


def test_the_restated_cut_is_the_headers(cutlib):
    o = (C.c_int64 * 4)()
    seen = 0
    for c in E.CASES:
        Q = E.taps_per_phase(c)
        lists = list(c.pieces.values())
        if c.name in ("1/16 Q17", "3/50 Q40"):
            lists += [E.poison_plan(c, where, seed)[1] for where, seed in E.POISON]
        for pieces in lists:
            pos = 0
            for n in pieces:
                cutlib.cut(c.L, c.M, Q, pos, n, o)
                assert tuple(o) == E.cut(c.L, c.M, Q, pos, n), (c.name, pos, n)
                m_first, count, n_first, p_first = tuple(o)
                assert m_first == RR.counts(c.L, c.M, pos) and count == RR.counts(c.L, c.M, pos + n) - m_first
                assert sum(t[0] for t in E.tile_paths(c.L, c.M, Q, pos, n, LIMIT)) == count
                assert 0 <= n_first < 2 ** 31 and (count == 0 or n_first < n)
                pos += n
                seen += 1
            assert pos == c.N
    assert seen == (1 + 5) * len(E.CASES) + 2 * len(FLIP) + 2 * 2 * len(E.POISON)


# ------------------------------------------------------------------------------------------------------------ the poisoned sample
@pytest.mark.parametrize("name", ["1/16 Q17", "3/50 Q40"])
def test_the_poisoned_positions(name):
    """each position has a reader that takes it from the source and one that takes it from the carry, in tiles of the path meant;
    the readers are those of the definition, by brute force"""
    c = E.CASE[name]
    Q = E.taps_per_phase(c)
    n_all = [int(v) for v in RR.positions(c.L, c.M, np.arange(RR.counts(c.L, c.M, c.N)))[0]]
    whole = E.tile_paths(c.L, c.M, Q, 0, c.N, LIMIT)
    for where, seed in E.POISON:
        n_bad, pieces = E.poison_plan(c, where, seed)
        ms, ns = E.readers(c.L, c.M, Q, c.N, n_bad)
        assert ms == [m for m, n in enumerate(n_all) if n - (Q - 1) <= n_bad <= n] and ns == [n_all[m] for m in ms]
        assert len(ms) >= 2 and sum(pieces) == c.N and len(pieces) == 2
        B = pieces[0]
        assert ns[0] < B == ns[1] and n_bad < B <= n_bad + Q - 1  # the sample lies in the second feed's carry
        assert {whole[m // E.TILE][2] for m in ms} == {where}
        second = E.tile_paths(c.L, c.M, Q, B, c.N - B, LIMIT)
        assert second[0][2] == where  # the readers behind the cut are in the second feed's first tile
        assert ms[-1] - RR.counts(c.L, c.M, B) < second[0][0]
    assert [w for w, _ in E.POISON] == ["mem", "lds"]
