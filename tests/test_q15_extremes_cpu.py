"""The Q15 (cs16 output) family at saturation and wrap, on the CPU: tests/xlating_q15_ref.py -- the int64 restatement with a count
per saturating line -- pinned to the oracle on every input tests/test_q15_extremes_gpu.py feeds the kernels; the conditions on those
inputs (how often each line acts), so that the GPU comparisons cannot quietly test nothing; the oracle's cut of the shifted sum to
32 bits against a recorded run of the unmodified reference; the kernels' narrowing helper against plain integer arithmetic.
Every comparison is exact equality."""
import os
import subprocess

import numpy as np
import pytest

import q15_extremes_cases as QC
import xlating_q15_ref as QR
from conftest import GOLDEN, ROOT
from pyoracle import Oracle, RefLib

CSRC = os.path.join(ROOT, "sdr-server_amd", "csrc")


def _pair(shape, fc, maxin=QC.MAXIN):
    o = Oracle(QC.SHAPE_D[shape], QC.taps(shape), fc, QC.FS, maxin)
    return o, QR.of_oracle(o)


def _run_calls(fmt, clients, calls):
    """every distinct (shape, fc) of `clients` through `calls` on the oracle and the restatement: equal per block, equal final phase
    -> the restatement's counts summed over the clients (a client listed twice counts twice)"""
    total = dict.fromkeys(QR.SITES, 0)
    per = {}
    for key in sorted(set(clients)):
        o, s = _pair(*key)
        for k, (G, n, kinds) in enumerate(calls):
            for bl in np.split(QC.call_input(fmt, k, G, n, kinds), G):
                want, got = o.process(fmt, bl, "cs16"), s.process(fmt, bl)
                assert got.shape == want.shape and np.array_equal(got, want), (fmt, key, k)
        assert s.phase == o.phase_q15, (fmt, key)
        assert s.hist.shape[0] == o.history
        per[key] = dict(s.counts)
        o.close()
    for key in clients:
        for site in QR.SITES:
            total[site] += per[key][site]
    return total, per


def test_increment_and_conversions():
    """the Q15 increment from the oracle's float32 one, at the offsets of the issue's table; the three conversions at their extremes"""
    for fc in (-700000, 345678, 1234, 0):
        o = Oracle(42, QC.taps("d42"), fc, QC.FS, QC.MAXIN)
        s = QR.of_oracle(o)
        x = QC.block("noise", "cs16", 4096, seed=fc & 7)
        assert np.array_equal(s.process("cs16", x), o.process("cs16", x, "cs16")) and s.phase == o.phase_q15, fc
        o.close()
    assert QR.increment((np.float32(1.0), np.float32(0.0))) == (32767, 0)
    assert QR.convert("cu8", np.array([0, 255, 128, 127], np.uint8)).tolist() == [[-32768, 32512], [0, -256]]
    assert QR.convert("cs8", np.array([-128, 127, 0, -1], np.int8)).tolist() == [[-32768, 32512], [0, -256]]
    assert QR.convert("cs16", np.array([-32768, 32767, 5], np.int16)).tolist() == [[-32768, 32767]]
    assert QR.wrap32(np.array([2 ** 31, 2 ** 31 - 1, -2 ** 31 - 1, -2 ** 31, 2 ** 32 + 5])).tolist() == [-2 ** 31, 2 ** 31 - 1, 2 ** 31 - 1, -2 ** 31, 5]
    assert QC.taps("edge7").min() == -1.0 and QC.taps("edge7").max() < 1.0
    o = Oracle(2, QC.taps("edge7"), 0, QC.FS, QC.MAXIN)
    assert o.rtaps_q15[:, 0].min() == -32768 and o.rtaps_q15[:, 0].max() == 32767
    o.close()


@pytest.mark.parametrize("fmt", QC.FMTS)
def test_saturating_engine_inputs(fmt):
    """the saturation engine's population and calls: restatement == oracle; >= 32 sums and >= 32 outputs clipped on each side"""
    total, per = _run_calls(fmt, QC.SAT_CLIENTS, QC.SAT_CALLS)
    for site in ("sum_hi", "sum_lo", "out_hi", "out_lo"):
        assert total[site] >= 32, (fmt, total)
    assert total["wrap_hi"] == 0 and total["wrap_lo"] == 0
    # the population keeps a client whose sums clip while its outputs never do (fc = 0: the Q15 phase only decays from 32767), a
    # stop-band client that clips nowhere, and the taps of -32768 and 32767 at work
    c0 = per[("d42", 0)]
    assert c0["sum_hi"] >= 32 and c0["sum_lo"] >= 32 and c0["out_hi"] == 0 and c0["out_lo"] == 0, c0
    assert not any(per[("d42", QC.STOP_BAND[0])].values())
    assert per[("edge7", 1234)]["sum_hi"] > 0 and per[("edge7", 1234)]["sum_lo"] > 0


def test_square_block_site_counts():
    """the counts of one full-scale square block per class, as measured when the inputs were chosen (DESIGN.md quotes them)"""
    table = {("d42", 1234): {"cu8": (357, 353, 76, 64), "cs8": (357, 353, 76, 64), "cs16": (359, 353, 76, 69)},
             ("d21", 1234): {"cu8": (778, 769, 637, 625), "cs8": (778, 769, 637, 625), "cs16": (778, 769, 639, 628)},
             ("d7", 1234): {"cu8": (2296, 2287, 1723, 1692), "cs8": (2296, 2287, 1723, 1692), "cs16": (2296, 2287, 1729, 1701)}}
    for (shape, fc), row in table.items():
        for fmt, want in row.items():
            _, per = _run_calls(fmt, [(shape, fc)], QC.SAT_CALLS[:1])
            c = per[(shape, fc)]
            assert (c["sum_hi"], c["sum_lo"], c["out_hi"], c["out_lo"]) == want, (shape, fmt, c)


@pytest.mark.parametrize("fmt", QC.FMTS)
def test_tile_height_and_single_filter_inputs(fmt):
    """the tile-height engine's saturating call and the single filter's calls: restatement == oracle, both sides of both lines reached"""
    total, _ = _run_calls(fmt, QC.HEIGHT_CLIENTS, QC.HEIGHT_CALLS)
    for site in ("sum_hi", "sum_lo", "out_hi", "out_lo"):
        assert total[site] >= 32, (fmt, total)
    calls = [(1, n, (kind,)) for n, kind in QC.SINGLE_CALLS]
    for key in QC.SINGLE_SHAPES:
        total, _ = _run_calls(fmt, [key], calls)
        for site in ("sum_hi", "sum_lo", "out_hi", "out_lo"):
            assert total[site] >= 32, (fmt, key, total)


@pytest.mark.parametrize("fmt", QC.WRAP_FMTS)
def test_wrap_inputs(fmt):
    """windows of 65000 .. 70000 taps of 0.9999 over full-scale blocks: restatement == oracle.  The shifted sum never leaves the int32
    range at 65000 taps and leaves it on both sides in every other case -- except where arithmetic forbids it: cs8's maximum is 127 << 8
    = 32512, and 65700 x 32764 x 32512 >> 15 = 2135777653 < 2^31 (that case wraps on the low side only: -128 << 8 = -32768).  The client
    at fc = 500 wraps on the two tone blocks alone: its rotated taps cancel over a constant."""
    for name, T, fc in QC.WRAP_CASES:
        o = Oracle(QC.WRAP_D, QC.wrap_taps(T), fc, QC.FS, 2 * QC.WRAP_SAMPLES)
        s = QR.of_oracle(o)
        per_block = []
        for b in range(len(QC.WRAP_BLOCKS)):
            x = QC.wrap_block(fmt, b)
            want, got = o.process(fmt, x, "cs16"), s.process(fmt, x)
            assert got.shape == want.shape == (QC.WRAP_SAMPLES // QC.WRAP_D, 2) and np.array_equal(got, want), (fmt, name, b)
            per_block.append((s.last["wrap_hi"], s.last["wrap_lo"]))
        assert s.phase == o.phase_q15
        o.close()
        print(fmt, name, s.counts, per_block)
        if name == "below":
            assert QC.wrap_reachable(fmt, T) == (False, False)
            assert s.counts["wrap_hi"] == 0 and s.counts["wrap_lo"] == 0, (fmt, name, s.counts)
            assert s.counts["sum_hi"] >= 32 and s.counts["sum_lo"] >= 32  # (saturates without wrapping)
        elif fc == 0:
            hi, lo = QC.wrap_reachable(fmt, T)
            assert lo and (hi or (fmt, T) == ("cs8", 65700)), (fmt, name)
            assert (s.counts["wrap_hi"] >= 1) == hi and s.counts["wrap_lo"] >= 1, (fmt, name, s.counts)
            assert per_block[0][0] >= (1 if hi else 0) and per_block[1][1] >= 1  # (on the constant blocks already)
        else:
            assert s.counts["wrap_hi"] >= 1 and s.counts["wrap_lo"] >= 1, (fmt, name, s.counts)
            assert all(p == (0, 0) for p in per_block[:3])


def test_wrap_semantics_of_the_reference():
    """65700 taps of 0.9999, D = 1000, fc = 0, I = +32767: the unmodified reference's outputs (recorded; live where its build is at
    hand) turn negative once the shifted sum passes 2^31 - 1 -- and the oracle and the restatement say the same"""
    g = QC.GOLDEN_WRAP
    rec = np.load(os.path.join(GOLDEN, "q15_wrap_t65700.npz"))["y"]
    x = QC.wrap_block(g["fmt"], g["block"], g["samples"])
    o = Oracle(g["D"], QC.wrap_taps(g["T"]), g["fc"], QC.FS, 2 * g["samples"])
    s = QR.of_oracle(o)
    want = o.process(g["fmt"], x, "cs16")
    assert rec.dtype == np.int16 and rec.shape == want.shape == (71, 2) and np.array_equal(rec, want)
    assert np.array_equal(s.process(g["fmt"], x), rec) and s.counts["wrap_hi"] == 5 and s.counts["wrap_lo"] == 0
    # full windows: 65700 x 32764 x 32767 >> 15 = 2152529108 -> -2142438188 -> -32768, rotated by a phase a little below 32767
    assert rec[:66, 0].min() > 32700 and rec[66:, 0].max() < -32690 and not rec[:, 1].any()
    o.close()
    if RefLib.available("canon"):
        r = RefLib(g["D"], QC.wrap_taps(g["T"]), g["fc"], QC.FS, 2 * g["samples"])
        live = r.process(g["fmt"], x, "cs16")
        r.close()
        assert np.array_equal(live, rec)


@pytest.mark.parametrize("fmt", QC.FMTS)
def test_restatement_from_a_given_history_and_phase(fmt):
    """what the mixing test relies on: a stream started from an explicit history (the T - 1 samples before the call) and phase equals
    the oracle's call that had that state -- block A twice through the oracle, the second call restated on its own"""
    A, C = QC.mix_blocks(fmt)
    qa = QR.convert(fmt, A)
    for key in sorted(set(QC.MIX_CLIENTS)):
        o, _ = _pair(*key)
        o.process(fmt, A, "cs16")
        T = o.rtaps_q15.shape[0]
        assert o.history == T - 1  # (every decimation divides the block)
        s = QR.of_oracle(o, history=qa[qa.shape[0] - (T - 1):], phase=o.phase_q15)
        for x in (A, C):
            assert np.array_equal(s.process(fmt, x), o.process(fmt, x, "cs16")), (fmt, key)
        assert s.phase == o.phase_q15
        o.close()
    # the Q15 call of the mixing test itself (history A's tail, a fresh phase) saturates on both sides of both lines
    total = dict.fromkeys(QR.SITES, 0)
    for shape, fc in QC.MIX_CLIENTS:
        o, _ = _pair(shape, fc)
        T = o.rtaps_q15.shape[0]
        s = QR.of_oracle(o, history=qa[qa.shape[0] - (T - 1):])
        s.process(fmt, A)
        o.close()
        for site in QR.SITES:
            total[site] += s.counts[site]
    assert min(total[k] for k in ("sum_hi", "sum_lo", "out_hi", "out_lo")) >= 32, total


@pytest.mark.parametrize("seed,fmt", QC.CHURN_RUNS)
def test_churn_inputs(seed, fmt):
    """the churn schedule: every client from its join to its leave on the oracle and the restatement; the schedule has joins after
    leaves (slot reuse), blocks of 2 elements and calls of 3 blocks"""
    sched = QC.churn_schedule(seed)
    assert any(n == 2 for _, _, _, n, _ in sched) and any(G == 3 for _, _, G, _, _ in sched)
    assert any(st[0] and any(prev[1] for prev in sched[:i + 1]) for i, st in enumerate(sched))
    assert {kind for st in sched for kind in st[4]} == set(QC.KINDS)
    alive = {}
    total = dict.fromkeys(QR.SITES, 0)
    for k, (joins, leaves, G, n, kinds) in enumerate(sched):
        for u in leaves:
            alive.pop(u)[0].close()
        for u, shape, fc in joins:
            alive[u] = _pair(shape, fc)
        for bl in np.split(QC.call_input(fmt, k, G, n, kinds), G):
            for u, (o, s) in alive.items():
                assert np.array_equal(s.process(fmt, bl), o.process(fmt, bl, "cs16")), (seed, k, u)
                for site in QR.SITES:
                    total[site] += s.last[site]
    assert min(total[k] for k in ("sum_hi", "sum_lo", "out_hi", "out_lo")) >= 32, total


def test_narrow_helper_sweep(tmp_path):
    """sdr-server_amd/csrc/xl_q15_narrow.h with a main of its own (tests/c/q15_narrow_sweep.c) under a host compiler: equal to
    saturate_to_int16((int32_t)(sum >> 15)) in integer arithmetic on every sum swept"""
    exe = str(tmp_path / "q15_narrow_sweep")
    r = subprocess.run(["gcc", "-std=c11", "-O1", "-Wall", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "c", "q15_narrow_sweep.c"),
                        "-o", exe, "-lm"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok ") and r.stderr == "", (r.stdout[-500:], r.stderr[-2000:])
    assert int(r.stdout.split()[1]) >= 400000


def test_float64_q15_kernels_narrow_in_one_place():
    """both kernels that carry the Q15 sums in float64 narrow them with the helper, and nothing else in the kernel sources converts a
    floor() to a 32-bit integer"""
    for name, calls in (("xl_kernels.hip", 2), ("xl_wide.hip", 2)):
        src = open(os.path.join(CSRC, name)).read()
        assert src.count("xl_q15_narrow_sum(") == calls, name
        assert "(int32_t)__builtin_floor" not in src, name
    hdr = open(os.path.join(CSRC, "xl_dev_inline.h")).read()
    assert '#include "xl_q15_narrow.h"' in hdr and "int32_t xl_sat16(" not in hdr
