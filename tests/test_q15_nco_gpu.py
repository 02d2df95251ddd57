"""GPU tests (-m gpu) of the Q15 phase look-ahead (engine option "q15_nco" = 1; csrc/xl_kernels.hip: xl_nco_q15_ahead_kernel, csrc/xl_batch.cpp:
xl_call_q15): the phase table of a Q15 call tabulated a call ahead on the side stream, or on the call's stream after a wrong guess, by
the packed five-instruction step.  Every client's whole cs16 stream of every call against the oracle's process_<fmt>_cs16
(xlating.c:92-140), exactly, with the matrix-core FIR and without it; xlating_batch_describe counts the look-aheads used and dropped,
and every test that says a look-ahead served a call asserts the count, so none passes on tables tabulated in-stream throughout.  At the
workload's shape the yardstick is an engine with the option at 0 in the same process.  Every comparison is exact equality.

A look-ahead is launched only behind a call whose plan holds no immature client (csrc/xl_q15_ahead.h): the first call after a join
never launches one, the call after it re-plans and tabulates in-stream.  Where a test counts from a known state it warms up with two
calls and sets the option again, which drops the pending look-ahead and restarts both counts ("counted since the option was set")."""
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
    """-> (look-aheads used, dropped) since the option was set"""
    m = re.search(r"\| q15 nco: ahead, (\d+) used, (\d+) dropped", eng.describe())
    assert m, eng.describe()
    return int(m.group(1)), int(m.group(2))


def _first_difference(got, want):
    if got.shape != want.shape:
        return f"shapes {got.shape} / {want.shape}"
    bad = np.nonzero((got != want).any(axis=1))[0]
    return f"index {int(bad[0])}: got {got[bad[0]].tolist()}, want {want[bad[0]].tolist()} ({bad.size} of {len(want)} outputs differ, the last at {int(bad[-1])})"


def _check(eng, ors, fmt, x, G, tag):
    eng.fetch()
    for cid, o in ors.items():
        want = np.concatenate([o.process(fmt, bl, "cs16") for bl in np.split(x, G)])
        got = eng.output_cs16(cid)
        assert got.shape == want.shape and np.array_equal(got, want), (tag, f"client {cid}", _first_difference(got, want))


def _q15_call(eng, ors, fmt, x, G, tag):
    """one Q15 call of G blocks: every client's cs16 stream == its oracle's, exactly"""
    eng.process_host_group(x, G, "q15")
    _check(eng, ors, fmt, x, G, tag)


def _close(eng, ors):
    eng.close()
    for o in ors.values():
        o.close()


def _engine(fmt, q15_kernel, group_blocks=1, maxin=QC.MAXIN, nco=1):
    eng = xl.BatchEngine(QC.FS, fmt, maxin, group_blocks=group_blocks)
    eng.set_option("q15_kernel", q15_kernel)
    eng.set_option("q15_nco", nco)
    return eng


def _recount(eng):
    """drop the pending look-ahead and count from zero"""
    eng.set_option("q15_nco", 1)
    assert _counts(eng) == (0, 0)


# five clients for each (D, T); D = 1 walks 32768 phases per block of QC.MAXIN: the longest chain such a block allows
SHAPES = [(1, 16), (3, 81), (7, 81), (42, 505), (64, 505)]


def _shape_taps(T):
    if T == 505:
        return QC.taps("d42")
    if T == 81:
        return QC.taps("d7")
    return np.random.default_rng(1000 + T).uniform(-0.9, 0.9, T).astype(np.float32)


def _population(eng):
    ors = {}
    for D, T in SHAPES:
        for fc in QC.FC_D42[:5]:
            ors[eng.add_client(D, _shape_taps(T), fc)] = Oracle(D, _shape_taps(T), fc, QC.FS, QC.MAXIN)
    return ors


def _warm_up(eng, ors, fmt):
    """two calls: every client is mature behind the first, the second runs on the final plan (and launches a look-ahead)"""
    for k in range(2):
        _q15_call(eng, ors, fmt, QC.call_input(fmt, 50 + k, 1, QC.MAXIN, ("noise",)), 1, ("warm-up", k))


def test_option_describe_accessor():
    """the option exists (the parent answers -ENOENT) and takes 0 and 1 only; describe carries the counts with the option at 1 and is
    unchanged with it at 0; phase_q15 is the COMMITTED phase -- after each of four equal calls the int64 restatement's phase after that
    many calls, not the one a pending look-ahead has already computed for the call behind --; an engine destroyed right behind a
    call, the look-ahead pending, goes cleanly and the next engine works"""
    eng = xl.BatchEngine(QC.FS, "cu8", QC.MAXIN)
    cid = eng.add_client(42, QC.taps("d42"), 1234)
    plain = eng.describe()
    assert "q15 nco" not in plain
    for bad in (2, -1):
        with pytest.raises(xl.XlatingError) as e:
            eng.set_option("q15_nco", bad)
        assert e.value.code == -22
    eng.set_option("q15_nco", 0)
    assert eng.describe() == plain
    eng.set_option("q15_nco", 1)
    line = " | q15 nco: ahead, 0 used, 0 dropped"
    assert line in eng.describe() and eng.describe().replace(line, "") == plain
    assert eng.phase_q15(cid) == (32767, 0)
    with pytest.raises(xl.XlatingError) as e:
        eng.phase_q15(cid + 1)
    assert e.value.code == -22
    o = Oracle(42, QC.taps("d42"), 1234, QC.FS, QC.MAXIN)
    ref = QR.of_oracle(o)
    for k in range(4):
        x = QC.block("noise", "cu8", QC.MAXIN, seed=k)
        _q15_call(eng, {cid: o}, "cu8", x, 1, ("call", k))
        ref.process("cu8", x)
        assert eng.phase_q15(cid) == ref.phase, (k, eng.phase_q15(cid), ref.phase)
    assert _counts(eng) == (2, 0)  # (call 0 ran on a plan with an immature client, call 1 re-planned)
    eng.set_option("q15_nco", 0)
    x = QC.block("noise", "cu8", QC.MAXIN, seed=9)
    _q15_call(eng, {cid: o}, "cu8", x, 1, "off")
    ref.process("cu8", x)
    assert eng.phase_q15(cid) == ref.phase and "q15 nco" not in eng.describe()
    eng.set_option("q15_nco", 1)
    x = QC.block("noise", "cu8", QC.MAXIN, seed=10)
    eng.process_host(x, "q15")  # (launches a look-ahead)
    eng.close()
    o.process("cu8", x, "cs16")
    f32 = xl.BatchEngine(QC.FS, "cf32", QC.MAXIN)
    c32 = f32.add_client(42, QC.taps("d42"), 1234)
    with pytest.raises(xl.XlatingError) as e:
        f32.phase_q15(c32)
    assert e.value.code == -22
    f32.close()
    eng = _engine("cu8", 1)
    cid = eng.add_client(42, QC.taps("d42"), 1234)
    o2 = Oracle(42, QC.taps("d42"), 1234, QC.FS, QC.MAXIN)
    _q15_call(eng, {cid: o2}, "cu8", x, 1, "next engine")
    _close(eng, {cid: o, -1: o2})


@pytest.mark.parametrize("q15_kernel", (0, 1))
@pytest.mark.parametrize("fmt", ("cu8", "cs16"))
def test_steady_calls_use_the_look_ahead(fmt, q15_kernel):
    """six equal one-block calls behind the warm-up: six look-aheads used, none dropped; then four calls of three blocks of 30002
    elements: the first drops the one-block guess, the other three use theirs"""
    eng = _engine(fmt, q15_kernel, group_blocks=3)
    ors = _population(eng)
    _warm_up(eng, ors, fmt)
    used0, dropped0 = _counts(eng)
    for k in range(6):
        _q15_call(eng, ors, fmt, QC.call_input(fmt, k, 1, QC.MAXIN, (("noise", "square")[k & 1],)), 1, (fmt, "one block", k))
        assert _counts(eng) == (used0 + k + 1, dropped0), (k, eng.describe())
    for k in range(4):
        _q15_call(eng, ors, fmt, QC.call_input(fmt, 6 + k, 3, 30002, ("square", "max", "noise")), 3, (fmt, "three blocks", k))
        assert _counts(eng) == (used0 + 6 + k, dropped0 + 1), (k, eng.describe())
    _close(eng, ors)


@pytest.mark.parametrize("q15_kernel", (0, 1))
def test_wrong_guesses(q15_kernel):
    """calls of changing shape: a look-ahead is dropped exactly at the four shape changes and used exactly at the three repeats (the
    first call finds none: the count was restarted behind the warm-up); the block of one sample gives most clients no output"""
    fmt = "cs16"
    eng = _engine(fmt, q15_kernel, group_blocks=3)
    ors = _population(eng)
    _warm_up(eng, ors, fmt)
    _recount(eng)
    calls = [(1, QC.MAXIN), (1, QC.MAXIN), (1, 20002), (1, 20002), (3, 30002), (1, 2), (1, QC.MAXIN), (1, QC.MAXIN)]
    want = [(0, 0), (1, 0), (1, 1), (2, 1), (2, 2), (2, 3), (2, 4), (3, 4)]
    for k, (G, n) in enumerate(calls):
        _q15_call(eng, ors, fmt, QC.call_input(fmt, k, G, n, ("noise", "square", "noise")[:G]), G, (k, G, n))
        assert _counts(eng) == want[k], (k, eng.describe())
        if n == 2:
            assert sum(eng.output_len(cid) == 0 for cid in ors) >= 10  # (the ten clients of D = 42 and 64: the stream stands at an odd sample)
    _close(eng, ors)


@pytest.mark.parametrize("fmt", ("cu8", "cs16"))
def test_between_float_calls(fmt):
    """calls A native, A Q15, A Q15, C optimized, A Q15 on one engine (matrix-core FIR on), every decimation dividing the blocks: the
    second Q15 call uses the look-ahead of the first, the optimized call moves the stream and makes the third's stale.  The native call
    bit for bit the oracle's, the optimized call within the project's 1e-5 of an oracle fed (A, C), with its phase; the Q15 calls the
    restatement started on the tail of the block before them, its phase running through all three"""
    A, C = QC.mix_blocks(fmt)
    eng = _engine(fmt, 1)
    ors = {}
    for shape, fc in QC.MIX_CLIENTS:
        ors[eng.add_client(QC.SHAPE_D[shape], QC.taps(shape), fc)] = Oracle(QC.SHAPE_D[shape], QC.taps(shape), fc, QC.FS, QC.MAXIN)
    qa, qc = QR.convert(fmt, A), QR.convert(fmt, C)
    eng.process_host(A, "native")
    eng.fetch()
    for cid, o in ors.items():
        assert bits_equal(eng.output(cid), o.process(fmt, A)), (fmt, cid)
    refs = {cid: QR.of_oracle(o, history=qa[qa.shape[0] - (o.rtaps_q15.shape[0] - 1):]) for cid, o in ors.items()}

    def q15(tag):
        eng.process_host(A, "q15")
        eng.fetch()
        for cid in ors:
            want, out = refs[cid].process(fmt, A), eng.output_cs16(cid)
            assert out.shape == want.shape and np.array_equal(out, want), (fmt, tag, cid, _first_difference(out, want))
            assert eng.phase_q15(cid) == refs[cid].phase, (fmt, tag, cid)

    q15("first")
    assert _counts(eng) == (0, 0)
    q15("second")
    assert _counts(eng) == (1, 0)
    eng.process_host(C, "optimized")
    eng.fetch()
    for cid, o in ors.items():
        want, out = o.process(fmt, C), eng.output(cid)
        assert out.shape == want.shape, (fmt, cid)
        err = float(np.abs(out.astype(np.complex128) - want).max() / np.abs(want).max())
        assert err <= REL_TOL, (fmt, cid, err)
        assert eng.phase(cid) == o.phase, (fmt, cid)
        refs[cid].hist = qc[qc.shape[0] - (refs[cid].T - 1):]
    q15("third")
    assert _counts(eng) == (1, 1)
    _close(eng, ors)


@pytest.mark.parametrize("q15_kernel", (0, 1))
@pytest.mark.parametrize("seed,fmt", QC.CHURN_RUNS)
def test_joins_leaves_slot_reuse(seed, fmt, q15_kernel):
    """tests/test_q15_extremes_gpu.py's churn: clients join and leave between calls, every client against an oracle created at its
    join -- a client that takes over a removed client's slot starts at 32767 + 0j, whatever a look-ahead wrote there.  Every step's
    call is issued twice (the client set does not change between a call and its repeat: this covers every place where two steps
    follow each other without a join or a leave), so look-aheads are used -- behind steps without a join -- and dropped by the joins
    and leaves of the step behind"""
    eng = _engine(fmt, q15_kernel, group_blocks=3)
    cid_of, ors = {}, {}
    for k, (joins, leaves, G, n, kinds) in enumerate(QC.churn_schedule(seed)):
        for u in leaves:
            cid = cid_of.pop(u)
            eng.remove_client(cid)
            ors.pop(cid).close()
        for u, shape, fc in joins:
            cid = eng.add_client(QC.SHAPE_D[shape], QC.taps(shape), fc)
            assert eng.phase_q15(cid) == (32767, 0), (k, cid)
            cid_of[u] = cid
            ors[cid] = Oracle(QC.SHAPE_D[shape], QC.taps(shape), fc, QC.FS, QC.MAXIN)
        _q15_call(eng, ors, fmt, QC.call_input(fmt, k, G, n, kinds), G, (seed, k))
        _q15_call(eng, ors, fmt, QC.call_input(fmt, 100 + k, G, n, kinds), G, (seed, k, "repeat"))
    used, dropped = _counts(eng)
    assert used > 0 and dropped > 0, eng.describe()
    _close(eng, ors)


@pytest.mark.parametrize("fmt", QC.FMTS)
def test_extremes(fmt):
    """the saturation engine of tests/test_q15_extremes_gpu.py, every call issued twice: the second of each pair on a look-ahead"""
    eng = _engine(fmt, 1, group_blocks=3)
    ors = {}
    for shape, fc in QC.SAT_CLIENTS:
        ors[eng.add_client(QC.SHAPE_D[shape], QC.taps(shape), fc)] = Oracle(QC.SHAPE_D[shape], QC.taps(shape), fc, QC.FS, QC.MAXIN)
    for k, (G, n, kinds) in enumerate(QC.SAT_CALLS):
        for r in range(2):
            _q15_call(eng, ors, fmt, QC.call_input(fmt, k + 20 * r, G, n, kinds), G, (fmt, k, r))
    used, dropped = _counts(eng)
    # (the first four pairs have one shape: behind the first pair's re-plan six in a row are used; two shape changes, two more repeats)
    assert (used, dropped) == (8, 2), eng.describe()
    _close(eng, ors)


def test_beside_a_wide_client():
    """tests/test_q15_matrix_gpu.py's engine (option "max_window", the recorded 65700-tap client on the wide launch, ten 505-tap
    clients): the first call's wide client is the golden record; in two more equal calls the wide client is bit for bit that of an
    engine with the option at 0 fed the same blocks, and the third call reads a table tabulated ahead -- the wide launch takes the
    call's table, not the one before it"""
    g = QC.GOLDEN_WRAP
    rec = np.load(os.path.join(ROOT, "tests", "golden", "q15_wrap_t65700.npz"))["y"]
    maxin = 2 * g["samples"]
    engs, wides = [], []
    for nco in (1, 0):
        eng = xl.BatchEngine(QC.FS, g["fmt"], maxin)
        eng.set_option("max_window", QC.WRAP_MAX_WINDOW)
        eng.set_option("q15_kernel", 1)
        eng.set_option("q15_nco", nco)
        wides.append(eng.add_client(g["D"], QC.wrap_taps(g["T"]), g["fc"]))
        ids = []
        for c in range(10):
            ids.append(eng.add_client(42, QC.taps("d42"), QC.FC_D42[c % len(QC.FC_D42)] + 5 * (c // len(QC.FC_D42))))
        engs.append((eng, ids))
    eng, ids = engs[0]
    ors = {cid: Oracle(42, QC.taps("d42"), QC.FC_D42[c % len(QC.FC_D42)] + 5 * (c // len(QC.FC_D42)), QC.FS, maxin) for c, cid in enumerate(ids)}
    x = QC.wrap_block(g["fmt"], g["block"], g["samples"])
    for k in range(3):
        _q15_call(eng, ors, g["fmt"], x, 1, ("wrap", k))
        engs[1][0].process_host(x, "q15")
        engs[1][0].fetch()
        got, want = eng.output_cs16(wides[0]), engs[1][0].output_cs16(wides[1])
        assert got.shape == want.shape and got.shape[0] > 0 and np.array_equal(got, want), (k, _first_difference(got, want))
        if k == 0:
            assert np.array_equal(got, rec)
    assert "| wide: 1 clients" in eng.describe() and _counts(eng) == (1, 0), eng.describe()
    assert "q15 nco" not in engs[1][0].describe()
    engs[1][0].close()
    _close(eng, ors)


def test_caller_streams():
    """six equal calls through process_device on two caller streams and the engine's own in turn, a fetch after each: exact, and the
    five look-aheads launched behind the first five calls are all used"""
    import torch

    fmt = "cu8"
    eng = _engine(fmt, 1)
    ors = _population(eng)
    _warm_up(eng, ors, fmt)
    _recount(eng)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    xs = [QC.call_input(fmt, 30 + k, 1, QC.MAXIN, ("noise",)) for k in range(6)]
    dev = [torch.from_numpy(x).cuda() for x in xs]
    torch.cuda.synchronize()
    for k in range(6):
        st = (streams[0].cuda_stream, streams[1].cuda_stream, "engine")[k % 3]
        eng.process_device_group(dev[k].data_ptr(), QC.MAXIN, 1, "q15", st)
        _check(eng, ors, fmt, xs[k], 1, ("stream", k))
    assert _counts(eng) == (5, 0), eng.describe()
    _close(eng, ors)


@pytest.mark.parametrize("fmt", ("cu8", "cs16"))
def test_workload_shape_device_against_device(fmt):
    """1024 clients of the server's own filter (D = 42, 505 taps), blocks of 131072 samples: an engine with (q15_kernel, q15_nco) =
    (1, 1) against one with (1, 0) on the same blocks -- one call that matures the clients, then three calls of one block and three of
    eight, every client's rows of the six bit for bit, and its phase_q15 behind the last.  (Without the first call the six would use
    three look-aheads, not four: none is launched behind a call whose plan holds immature clients.)"""
    S = 131072
    engs = []
    for nco in (0, 1):
        eng = xl.BatchEngine(QC.FS, fmt, 2 * S, group_blocks=8)
        eng.set_option("q15_kernel", 1)
        eng.set_option("q15_nco", nco)
        ids = [eng.add_client(42, QC.taps("d42"), -1000000 + 1953 * c) for c in range(1024)]
        engs.append((eng, ids))
    info = np.iinfo(QC.NPDT[fmt])
    for k, G in enumerate((1, 1, 1, 1, 8, 8, 8)):
        x = np.random.default_rng(400 + k).integers(info.min, info.max + 1, 2 * S * G, dtype=QC.NPDT[fmt])
        rows = []
        for eng, ids in engs:
            eng.process_host_group(x, G, "q15")
            if k > 0:
                eng.fetch()
                rows.append([eng.output_cs16(cid) for cid in ids])
        if k > 0:
            for c, (a, b) in enumerate(zip(*rows)):
                assert a.shape == b.shape and a.shape[0] >= G * (S // 42) and np.array_equal(a, b), (fmt, k, c, _first_difference(b, a))
    for ca, cb in zip(engs[0][1], engs[1][1]):
        assert engs[0][0].phase_q15(ca) == engs[1][0].phase_q15(cb), ca
    used, dropped = _counts(engs[1][0])
    assert used >= 4 and dropped == 1, engs[1][0].describe()
    assert "q15 nco" not in engs[0][0].describe()
    for eng, _ in engs:
        eng.close()


LONG_RUN_CALLS = 1500


def test_long_run_beside_the_matrix_launch():
    """The look-ahead kernel's packed INTEGER instructions (v_dot2_i32_i16, v_cvt_pk_i16_i32) resident beside v_mfma_i32_32x32x32_i8 of
    the matrix-core FIR: 1024 clients (D = 42, 505 taps), cu8, 8 blocks of 32768 samples per call, LONG_RUN_CALLS = 1500 equal calls
    on one device-resident super-block (the phase does not depend on it) -- about 10^10 steps, three orders of magnitude beyond the rate
    at which packed FP32 lost lanes beside matrix instructions -- against an engine with (1, 0) in the same process on the
    same blocks: every client's phase_q15 every 100 calls and the whole outputs of the last call, identical.
    Running time: 2.0 s for the 1500 calls on an MI355X (the count would be lowered, never the client count, if it passed about ten
    seconds)."""
    import torch

    S, G = 32768, 8
    engs = []
    for nco in (0, 1):
        eng = xl.BatchEngine(QC.FS, "cu8", 2 * S, group_blocks=G)
        eng.set_option("q15_kernel", 1)
        eng.set_option("q15_nco", nco)
        ids = [eng.add_client(42, QC.taps("d42"), -1000000 + 1953 * c) for c in range(1024)]
        engs.append((eng, ids))
    x = torch.from_numpy(np.random.default_rng(77).integers(0, 256, 2 * S * G, dtype=np.uint8)).cuda()
    st = torch.cuda.current_stream().cuda_stream
    torch.cuda.synchronize()
    for k in range(LONG_RUN_CALLS):
        for eng, _ in engs:
            eng.process_device_group(x.data_ptr(), 2 * S, G, "q15", st)
        if (k + 1) % 100 == 0:
            a = [engs[0][0].phase_q15(c) for c in engs[0][1]]
            b = [engs[1][0].phase_q15(c) for c in engs[1][1]]
            bad = [c for c in range(1024) if a[c] != b[c]]
            assert not bad, (k + 1, len(bad), bad[:8], [(a[c], b[c]) for c in bad[:4]])
    rows = []
    for eng, ids in engs:
        eng.fetch()
        rows.append([eng.output_cs16(cid) for cid in ids])
    for c, (a, b) in enumerate(zip(*rows)):
        assert a.shape == b.shape and a.shape[0] >= G * (S // 42) and np.array_equal(a, b), (c, _first_difference(b, a))
    used, dropped = _counts(engs[1][0])
    assert used >= LONG_RUN_CALLS - 2 and dropped == 0, engs[1][0].describe()
    for eng, _ in engs:
        eng.close()
