"""GPU tests (-m gpu) that hold EVERY k-block count of every polyphase mix kernel to the oracle: one test per (arm, count) of
tests/mix_kblock_cases.py, running that count's two decimations -- D = 8 nkb without a padding row and D = 8 nkb - 7 with seven -- in
every format and transform length the table gives it.  The arms: the two-half kernels with the converting staging of the integer
formats (plain), with cf32's per-segment scales (seg) and with the operand image (img: xlp_mix_mfma_kernel, 1 .. 8 k-blocks only), the
wide two-half kernel behind plain and seg from 9 k-blocks on, the float32 matrix mix (f32, 1 .. 14) and its streamed form (15).
tests/test_mix_kblocks_cpu.py asserts that these are all the instantiations the dispatch switches reach and what the calls are.

Per engine: FS = 2016000, blocks of 16384 samples, three calls of 8 blocks (16 in the seven cases whose 8 blocks are fewer than 17
segments), 37 clients -- wave 0 full, wave 1 with five columns, waves 2 and 3 vacant --, in the plain arm at 4, 10 and 14 k-blocks
also 160: a second, partial column group.  Noise in the arm's format.  Asserted: describe() shows the forced class, its transform
length and the arm's mix tag, and ends the class with calls=3 -- every call ran the launches under test, none the direct fall-back --;
every client's length is the oracle's; max|d| / max|y| <= 1e-5 per client over the stream (REL_TOL: the project's bar, DESIGN 5, not
fitted here); and an img engine's outputs are bit for bit the plain engine's at the same D -- the promise of xl_mixh.hip.

The oracle population is computed once per (D, format, clients, call length) and shared between the arms of a count, the plain run
once per D between the plain and the img test.  Each test prints its cases' worst ratios (pytest -s; profiles/mix_kblock_counts.txt)."""
import functools
import re

import numpy as np
import pytest

import mix_kblock_cases as mk
import siggen
from mix_harness import ELEMS, FS, NCALLS, REL_TOL, _fcs, _rel_err, _run, _stream, population

pytestmark = pytest.mark.gpu
assert ELEMS == 2 * mk.NSAMP and NCALLS == 3


def _taps(D):
    return siggen.hamming_sinc(mk.taps_of(D), 0.45 / D)


@functools.lru_cache(maxsize=8)
def _input(fmt, blocks, D):
    x = _stream(fmt, blocks * NCALLS, 9100 + D)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=12)
def _oracle(D, fmt, clients, blocks):
    """every client of the population over the whole stream, shared (and left unchanged) by the arms that run this shape"""
    want = population(D, _taps(D), _fcs(clients), FS, ELEMS, fmt, _input(fmt, blocks, D), blocks * NCALLS)
    for w in want:
        w.setflags(write=False)
    return want


def _engine(case):
    """One engine of the case over its three calls; the plan's assertions -> outputs per client"""
    got, d = _run(case.fmt, case.D, _taps(case.D), _fcs(case.clients), 0, None, _input(case.fmt, case.blocks, case.D), case.blocks,
                  options=case.options)
    cls = re.search(r" cls0 [^|]*?(?= \||$)", d)
    assert cls and "cls1" not in d, d
    cls = cls.group(0)
    assert ("polyphase: cls0 D%d T%d cols%d " % (case.D, case.T, case.clients)) in d and " M%d " % case.M in cls, d
    assert case.tag + " " in cls and (case.not_tag is None or case.not_tag not in cls), d
    assert cls.endswith(" calls=%d" % NCALLS), d  # every call took the polyphase launches
    return got


@functools.lru_cache(maxsize=4)
def _plain_run(case):
    got = _engine(case)
    for g in got:
        g.setflags(write=False)
    return got


def _plain_case_of(case):
    (p,) = [c for c in mk.cases_of("plain", case.nkb) if (c.D, c.M, c.fmt, c.clients, c.blocks) == (case.D, case.M, case.fmt, case.clients,
                                                                                                  case.blocks)]
    return p


@pytest.mark.parametrize("arm,nkb", mk.tests(), ids=lambda v: str(v))
def test_every_kblock_count_against_the_oracle(arm, nkb):
    cases = mk.cases_of(arm, nkb)
    assert cases
    worst_of_test = 0.0
    for case in cases:
        got = _plain_run(case) if arm == "plain" else _engine(case)
        if arm == "img":
            plain = _plain_run(_plain_case_of(case))
            for c in range(case.clients):
                assert got[c].shape == plain[c].shape and np.array_equal(got[c], plain[c]), (case, c, _rel_err(got[c], plain[c]))
        want = _oracle(case.D, case.fmt, case.clients, case.blocks)
        assert len(got) == len(want) == case.clients
        worst, worst_c = 0.0, None
        for c in range(case.clients):
            assert len(got[c]) == len(want[c]) and len(want[c]) >= NCALLS * 512, (case, c, len(got[c]), len(want[c]))
            e = _rel_err(got[c], want[c])
            if e > worst:
                worst, worst_c = e, c
        print("mix_kblocks %-6s nkb %2d D %3d M %3d %-4s clients %3d blocks %2d worst %.3g (client %s)" % (
            arm, nkb, case.D, case.M, case.fmt, case.clients, case.blocks, worst, worst_c))
        assert worst <= REL_TOL, (case, worst_c, worst)
        worst_of_test = max(worst_of_test, worst)
    print("mix_kblocks %-6s nkb %2d worst of the test %.3g" % (arm, nkb, worst_of_test))
