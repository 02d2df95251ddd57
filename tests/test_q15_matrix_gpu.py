"""GPU tests (-m gpu) of the matrix-core Q15 FIR (engine option "q15_kernel" = 1; csrc/q15mm/xl_q15_mm.hip): every client the launch
carries against the oracle's process_<fmt>_cs16 (xlating.c:92-140), exactly -- the operand maps of v_mfma_i32_32x32x32_i8 on asymmetric
integer data, partial tiles, every window alignment, joins and churn, the saturating extremes, beside wide clients -- and, at the
workload's shape, against the float64 launch of the same library, which tests/test_q15_extremes_gpu.py holds to the oracle.
xlating_batch_describe says how many clients ride which launch: tests/test_q15_matrix_cpu.py pins who may fall back (the edge7 taps
alone), so no test passes on a silent fallback.  Every comparison is exact equality."""
import os
import re

import numpy as np
import pytest

import q15_extremes_cases as QC
import sdr_server_amd as xl
import xlating_q15_ref as QR
from conftest import ROOT, bits_equal
from pyoracle import Oracle

pytestmark = pytest.mark.gpu
REL_TOL = 1e-5  # the project's bound on optimized calls (tests/test_batch_gpu.py)


def _counts(eng):
    """-> (clients on the matrix launch, its tiles, clients on the float64 launches, of these: digits, window)"""
    d = eng.describe()
    m = re.search(r"\| q15 matrix: (\d+) clients x (\d+) tiles, float64: (\d+) clients \(digits (\d+), window (\d+)\)", d)
    assert m, d
    return tuple(int(v) for v in m.groups())


def _first_difference(got, want):
    if got.shape != want.shape:
        return f"shapes {got.shape} / {want.shape}"
    bad = np.nonzero((got != want).any(axis=1))[0]
    return f"index {int(bad[0])}: got {got[bad[0]].tolist()}, want {want[bad[0]].tolist()} ({bad.size} of {len(want)} outputs differ, the last at {int(bad[-1])})"


def _q15_call(eng, ors, fmt, x, G, tag):
    """one Q15 call of G blocks: every client's cs16 stream == its oracle's, exactly"""
    eng.process_host_group(x, G, "q15")
    eng.fetch()
    for cid, o in ors.items():
        want = np.concatenate([o.process(fmt, bl, "cs16") for bl in np.split(x, G)])
        got = eng.output_cs16(cid)
        assert got.shape == want.shape and np.array_equal(got, want), (tag, f"client {cid}", _first_difference(got, want))


def _close(eng, ors):
    eng.close()
    for o in ors.values():
        o.close()


def _engine(fmt, group_blocks=1, maxin=QC.MAXIN):
    eng = xl.BatchEngine(QC.FS, fmt, maxin, group_blocks=group_blocks)
    eng.set_option("q15_kernel", 1)
    return eng


def test_option_and_describe():
    """the option exists (the parent answers -ENOENT), takes 0 and 1 only, and describe names the matrix launch once a Q15 call has
    built it; with the option at 0 the line does not mention it"""
    eng = xl.BatchEngine(QC.FS, "cu8", QC.MAXIN)
    cid = eng.add_client(42, QC.taps("d42"), 1234)
    plain = eng.describe()
    assert "q15 matrix" not in plain
    with pytest.raises(xl.XlatingError) as e:
        eng.set_option("q15_kernel", 2)
    assert e.value.code == -22
    eng.set_option("q15_kernel", 1)
    assert "| q15 matrix: (built by the first Q15 call)" in eng.describe()
    o = Oracle(42, QC.taps("d42"), 1234, QC.FS, QC.MAXIN)
    _q15_call(eng, {cid: o}, "cu8", QC.block("noise", "cu8", 20002), 1, "on")
    assert _counts(eng) == (1, 1, 0, 0, 0)
    eng.set_option("q15_kernel", 0)
    _q15_call(eng, {cid: o}, "cu8", QC.block("noise", "cu8", 20002, seed=1), 1, "off")
    assert "q15 matrix" not in eng.describe()
    _close(eng, {cid: o})


def test_operand_map():
    """33 clients (a full tile and one row of the next) of ONE tap (c + 1) / 64 at D = 1, fc = 0, over a ramp whose I and Q differ:
    output n of client c is a known multiple of sample n -- a swapped row and column, a permuted k, a wrong digit plane or a wrong
    accumulator row each show as a pattern in the first difference"""
    n = 4096
    x = np.empty((n, 2), np.int64)
    x[:, 0] = np.arange(n)
    x[:, 1] = -3 * np.arange(n) + 7
    x = x.astype(np.int16).reshape(-1)
    eng = _engine("cs16", maxin=2 * n)
    ors = {}
    for c in range(33):
        tap = np.array([(c + 1) / 64.0], np.float32)
        ors[eng.add_client(1, tap, 0)] = Oracle(1, tap, 0, QC.FS, 2 * n)
    _q15_call(eng, ors, "cs16", x, 1, "ramp")
    assert _counts(eng) == (33, 2, 0, 0, 0)
    _close(eng, ors)


@pytest.mark.parametrize("fmt", QC.FMTS)
def test_tile_edges(fmt):
    """classes of 1, 31, 32, 33 and 65 clients of the 505-tap filter in one engine (one sample of stream between the joins: five grids,
    five classes; 1 + 1 + 1 + 2 + 3 tiles, fewer clients than rows in five of them): noise, a full-scale square, the format's minimum and
    maximum held for a block each, three ragged blocks in a call, a block of one sample"""
    eng = _engine(fmt, group_blocks=3)
    ors, c = {}, 0
    for k, size in enumerate((1, 31, 32, 33, 65)):
        for _ in range(size):
            fc = QC.FC_D42[c % len(QC.FC_D42)] + 3 * (c // len(QC.FC_D42))
            ors[eng.add_client(42, QC.taps("d42"), fc)] = Oracle(42, QC.taps("d42"), fc, QC.FS, QC.MAXIN)
            c += 1
        _q15_call(eng, ors, fmt, QC.block("noise", fmt, 2, seed=90 + k), 1, (fmt, "join", k))
    calls = [(1, QC.MAXIN, ("noise",)), (1, QC.MAXIN, ("square",)), (1, QC.MAXIN, ("min",)), (1, QC.MAXIN, ("max",)),
             (3, 30002, ("square", "max", "noise")), (1, 2, ("square",))]
    for k, (G, n, kinds) in enumerate(calls):
        _q15_call(eng, ors, fmt, QC.call_input(fmt, k, G, n, kinds), G, (fmt, k))
        assert _counts(eng) == (162, 8, 0, 0, 0), eng.describe()
    _close(eng, ors)


# (D, T): every D of 1, 2, 3, 7, 8, 21, 42, 64 -- 8, 4, 2 and 1 window residues, odd and even -- and every T of 1, 2, 7, 16, 81, 505.
# D <= T throughout: with fewer taps than the decimation the reference's own process call writes past its working buffer (glibc aborts
# the oracle at its destroy: D = 64 with one tap, D = 7 with two), so no oracle exists for such a pair.
ALIGN_SHAPES = [(1, 1), (2, 2), (3, 7), (7, 16), (8, 81), (21, 505), (42, 505), (64, 505), (1, 505), (64, 81), (3, 81), (7, 7)]


def _align_taps(T):
    if T == 505:
        return QC.taps("d42")
    if T == 81:
        return QC.taps("d7")
    return np.random.default_rng(1000 + T).uniform(-0.9, 0.9, T).astype(np.float32)


@pytest.mark.parametrize("fmt", ("cu8", "cs16"))
def test_alignments_and_tap_counts(fmt):
    """five clients per (D, T): two noise calls -- the second of 20002 elements, so that every grid moves -- and a full-scale square"""
    eng = _engine(fmt)
    ors = {}
    for D, T in ALIGN_SHAPES:
        assert D <= T and T - 1 + D <= 16384
        for fc in QC.FC_D42[:5]:
            assert xl.q15_matrix_admits(D, _align_taps(T), fc, QC.FS), (D, T, fc)
            ors[eng.add_client(D, _align_taps(T), fc)] = Oracle(D, _align_taps(T), fc, QC.FS, QC.MAXIN)
    for k, (n, kind) in enumerate(((QC.MAXIN, "noise"), (20002, "noise"), (QC.MAXIN, "square"))):
        _q15_call(eng, ors, fmt, QC.call_input(fmt, k, 1, n, (kind,)), 1, (fmt, k))
        assert _counts(eng) == (5 * len(ALIGN_SHAPES), len(ALIGN_SHAPES), 0, 0, 0), eng.describe()
    _close(eng, ors)


@pytest.mark.parametrize("seed,fmt", QC.CHURN_RUNS)
def test_joins_and_churn(seed, fmt):
    """tests/test_q15_extremes_gpu.py's churn with the option on: clients join and leave between calls, so the grids and the zero
    histories differ inside a (D, T) -- every client against an oracle created at its join.  The float64 launches carry the edge7
    clients alive at the call (taps without an int8 digit pair: tests/test_q15_matrix_cpu.py) and nobody else.  Last, a client of 505
    taps joins and receives a block of 100 samples, shorter than its T - 1."""
    eng = _engine(fmt, group_blocks=3)
    cid_of, ors, shape_of = {}, {}, {}
    for k, (joins, leaves, G, n, kinds) in enumerate(QC.churn_schedule(seed)):
        for u in leaves:
            cid = cid_of.pop(u)
            eng.remove_client(cid)
            ors.pop(cid).close()
            shape_of.pop(cid)
        for u, shape, fc in joins:
            cid = eng.add_client(QC.SHAPE_D[shape], QC.taps(shape), fc)
            cid_of[u] = cid
            ors[cid] = Oracle(QC.SHAPE_D[shape], QC.taps(shape), fc, QC.FS, QC.MAXIN)
            shape_of[cid] = shape
        _q15_call(eng, ors, fmt, QC.call_input(fmt, k, G, n, kinds), G, (seed, k))
        edge = sum(s == "edge7" for s in shape_of.values())
        got = _counts(eng)
        assert (got[0], got[2], got[3], got[4]) == (len(ors) - edge, edge, edge, 0), (k, eng.describe())
    cid = eng.add_client(42, QC.taps("d42"), -1234)
    ors[cid] = Oracle(42, QC.taps("d42"), -1234, QC.FS, QC.MAXIN)
    _q15_call(eng, ors, fmt, QC.block("square", fmt, 200, seed=5), 1, (seed, "short"))
    _q15_call(eng, ors, fmt, QC.block("noise", fmt, 2000, seed=6), 1, (seed, "after"))
    _close(eng, ors)


@pytest.mark.parametrize("fmt", QC.FMTS)
def test_extremes(fmt):
    """the saturation engine of tests/test_q15_extremes_gpu.py with the option on: the two edge7 clients on the float64 launch, the
    other 23 on the matrix launch, every one exact"""
    eng = _engine(fmt, group_blocks=3)
    ors = {}
    for shape, fc in QC.SAT_CLIENTS:
        ors[eng.add_client(QC.SHAPE_D[shape], QC.taps(shape), fc)] = Oracle(QC.SHAPE_D[shape], QC.taps(shape), fc, QC.FS, QC.MAXIN)
    for k, (G, n, kinds) in enumerate(QC.SAT_CALLS):
        _q15_call(eng, ors, fmt, QC.call_input(fmt, k, G, n, kinds), G, (fmt, k))
        got = _counts(eng)
        assert (got[0], got[2], got[3], got[4]) == (23, 2, 2, 0), eng.describe()
    _close(eng, ors)


@pytest.mark.parametrize("fmt", ("cu8", "cs16"))
def test_between_float_calls(fmt):
    """calls A native, A Q15 (matrix launch), C optimized on one engine, every decimation dividing the blocks: one raw history behind
    both families, float phases the Q15 call never moved -- the native call bit for bit the oracle's, the Q15 call the restatement
    started on A's tail, the optimized call within the project's 1e-5 of an oracle fed (A, C), with its phase"""
    A, C = QC.mix_blocks(fmt)
    eng = _engine(fmt)
    ors = {}
    for shape, fc in QC.MIX_CLIENTS:
        ors[eng.add_client(QC.SHAPE_D[shape], QC.taps(shape), fc)] = Oracle(QC.SHAPE_D[shape], QC.taps(shape), fc, QC.FS, QC.MAXIN)
    qa = QR.convert(fmt, A)
    eng.process_host(A, "native")
    eng.fetch()
    for cid, o in ors.items():
        assert bits_equal(eng.output(cid), o.process(fmt, A)), (fmt, cid)
    eng.process_host(A, "q15")
    eng.fetch()
    got = _counts(eng)
    assert (got[0], got[2]) == (23, 2), eng.describe()
    for cid, o in ors.items():
        T = o.rtaps_q15.shape[0]
        want = QR.of_oracle(o, history=qa[qa.shape[0] - (T - 1):]).process(fmt, A)
        out = eng.output_cs16(cid)
        assert out.shape == want.shape and np.array_equal(out, want), (fmt, cid, _first_difference(out, want))
    eng.process_host(C, "optimized")
    eng.fetch()
    for cid, o in ors.items():
        want, out = o.process(fmt, C), eng.output(cid)
        assert out.shape == want.shape, (fmt, cid)
        err = float(np.abs(out.astype(np.complex128) - want).max() / np.abs(want).max())
        assert err <= REL_TOL, (fmt, cid, err)
        assert eng.phase(cid) == o.phase, (fmt, cid)
    _close(eng, ors)


def test_beside_a_wide_client():
    """option "max_window" set: the recorded reference run's client (65700 taps at D = 1000, cs16) on the wide launch still wraps as the
    golden file says, ten clients of 505 taps beside it ride the matrix launch, exactly"""
    g = QC.GOLDEN_WRAP
    rec = np.load(os.path.join(ROOT, "tests", "golden", "q15_wrap_t65700.npz"))["y"]
    maxin = 2 * g["samples"]
    eng = xl.BatchEngine(QC.FS, g["fmt"], maxin)
    eng.set_option("max_window", QC.WRAP_MAX_WINDOW)
    eng.set_option("q15_kernel", 1)
    wide = eng.add_client(g["D"], QC.wrap_taps(g["T"]), g["fc"])
    ors = {}
    for c in range(10):
        fc = QC.FC_D42[c % len(QC.FC_D42)] + 5 * (c // len(QC.FC_D42))
        ors[eng.add_client(42, QC.taps("d42"), fc)] = Oracle(42, QC.taps("d42"), fc, QC.FS, maxin)
    _q15_call(eng, ors, g["fmt"], QC.wrap_block(g["fmt"], g["block"], g["samples"]), 1, "wrap")
    assert np.array_equal(eng.output_cs16(wide), rec)
    assert "| wide: 1 clients" in eng.describe() and _counts(eng) == (10, 1, 0, 0, 0), eng.describe()
    _close(eng, ors)


@pytest.mark.parametrize("fmt", ("cu8", "cs16"))
def test_workload_shape_device_against_device(fmt):
    """1024 clients of the server's own filter (D = 42, 505 taps), one call of one block and one call of eight blocks of 131072
    samples: an engine with the option at 1 against an engine at 0 on the same blocks, every client's rows bit for bit.  (The float64
    launch is the yardstick here: the tests above and tests/test_q15_extremes_gpu.py hold it to the oracle.)"""
    S = 131072
    engs = []
    for opt in (0, 1):
        eng = xl.BatchEngine(QC.FS, fmt, 2 * S, group_blocks=8)
        eng.set_option("q15_kernel", opt)
        ids = [eng.add_client(42, QC.taps("d42"), -1000000 + 1953 * c) for c in range(1024)]
        engs.append((eng, ids))
    for k, G in enumerate((1, 8)):
        x = np.concatenate([QC.block("noise" if g % 3 else "square", fmt, 2 * S, seed=20 * k + g) for g in range(G)])
        rows = []
        for eng, ids in engs:
            eng.process_host_group(x, G, "q15")
            eng.fetch()
            rows.append([eng.output_cs16(cid) for cid in ids])
        assert _counts(engs[1][0]) == (1024, 32, 0, 0, 0), engs[1][0].describe()
        assert "q15 matrix" not in engs[0][0].describe()
        for c, (a, b) in enumerate(zip(*rows)):
            assert a.shape == b.shape and a.shape[0] >= G * (S // 42) and np.array_equal(a, b), (fmt, G, c, _first_difference(b, a))
    for eng, _ in engs:
        eng.close()
