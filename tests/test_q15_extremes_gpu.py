"""GPU tests (-m gpu) of the Q15 (cs16 output) family where its arithmetic saturates and wraps: the three Q15 FIR kernels
(xl_fir_q15_kernel, xl_fir_q15_batch_kernel at every tile height, xl_wide_q15_kernel) against the oracle's process_<fmt>_cs16
(xlating.c:92-140) on full-scale inputs, on windows long enough for the shifted sum to leave the int32 range, across client churn and
next to calls of the float families on the same engine.  tests/test_q15_extremes_cpu.py pins the inputs: how often each saturating
line acts on them.  Every Q15 comparison is exact equality."""
import numpy as np
import pytest

import q15_extremes_cases as QC
import sdr_server_amd as xl
import xlating_q15_ref as QR
from conftest import bits_equal
from pyoracle import Oracle

pytestmark = pytest.mark.gpu
REL_TOL = 1e-5  # the project's bound on optimized calls (tests/test_batch_gpu.py)


def _oracle(shape, fc, maxin=QC.MAXIN):
    return Oracle(QC.SHAPE_D[shape], QC.taps(shape), fc, QC.FS, maxin)


def _engine(fmt, clients, group_blocks=1, maxin=QC.MAXIN):
    eng = xl.BatchEngine(QC.FS, fmt, maxin, group_blocks=group_blocks)
    ors = {}
    for shape, fc in clients:
        ors[eng.add_client(QC.SHAPE_D[shape], QC.taps(shape), fc)] = _oracle(shape, fc, maxin)
    return eng, ors


def _first_difference(got, want):
    if got.shape != want.shape:
        return f"shapes {got.shape} / {want.shape}"
    i = int(np.nonzero((got != want).any(axis=1))[0][0])
    return f"index {i}: got {got[i].tolist()}, want {want[i].tolist()} ({int((got != want).any(axis=1).sum())} of {len(want)} outputs differ)"


def _same(got, want):
    return got.shape == want.shape and bool(np.array_equal(got, want))


def _q15_call(eng, ors, fmt, x, G, tag):
    """one Q15 call of G blocks: every client's cs16 stream == its oracle's, exactly"""
    eng.process_host_group(x, G, "q15")
    eng.fetch()
    for cid, o in ors.items():
        want = np.concatenate([o.process(fmt, bl, "cs16") for bl in np.split(x, G)])
        got = eng.output_cs16(cid)
        assert _same(got, want), (tag, f"client {cid}", _first_difference(got, want))


def _close(eng, ors):
    eng.close()
    for o in ors.values():
        o.close()


@pytest.mark.parametrize("fmt", QC.FMTS)
def test_engine_saturation(fmt):
    """xl_fir_q15_batch_kernel, classes of 13, 6, 3, 2 and 1 clients (taps of -32768 and 32767 among them): a full-scale square block,
    noise, the format's minimum and maximum held for a block each, a call of three ragged blocks, a block of one sample"""
    eng, ors = _engine(fmt, QC.SAT_CLIENTS, group_blocks=3)
    for k, (G, n, kinds) in enumerate(QC.SAT_CALLS):
        _q15_call(eng, ors, fmt, QC.call_input(fmt, k, G, n, kinds), G, (fmt, k))
    _close(eng, ors)


@pytest.mark.parametrize("height,fmt", [(8, "cu8"), (9, "cs8"), (10, "cs16"), (12, "cu8")])
def test_engine_every_tile_height(height, fmt, monkeypatch):
    """XL_EXP_H forces the tile height of the class of 25 (a partial last tile at each of 8, 9, 10, 12); classes of 6, 3, 2 and 1 take
    the heights 8, 4, 2 and 1.  A saturating and a noise Q15 call, exact; then a native call through xl_fir_kernel at the same height.
    The engine keeps one raw history and a float phase the Q15 calls never moved, and every decimation divides the blocks: the native
    call's outputs whose windows lie inside its own block are those of a fresh oracle; at fc = 0 (the phase stays 1) all of them are
    those of an oracle fed the three blocks."""
    monkeypatch.setenv("XL_EXP_H", str(height))
    eng, ors = _engine(fmt, QC.HEIGHT_CLIENTS)
    for k, (G, n, kinds) in enumerate(QC.HEIGHT_CALLS):
        _q15_call(eng, ors, fmt, QC.call_input(fmt, k, G, n, kinds), G, (height, fmt, k))
        if k == 0:
            d = eng.describe()
            for h in {height, 8, 4, 2, 1}:
                assert f" h{h} x" in d, d
            assert sum(f" h{h} x" in d for h in (8, 9, 10, 12)) == (1 if height == 8 else 2), d
    C = QC.block("noise", fmt, QC.MIX_N, seed=77)
    eng.process_host(C, "native")
    eng.fetch()
    for cid, (shape, fc) in zip(ors, QC.HEIGHT_CLIENTS):
        D, T = QC.SHAPE_D[shape], QC.taps(shape).size
        fresh = _oracle(shape, fc)
        want, got = fresh.process(fmt, C), eng.output(cid)
        skip = -(-(T - 1) // D)
        assert got.shape == want.shape and bits_equal(got[skip:], want[skip:]), (height, fmt, cid)
        fresh.close()
        if fc == 0:
            fed = _oracle(shape, fc)
            for k, (G, n, kinds) in enumerate(QC.HEIGHT_CALLS):
                fed.process(fmt, QC.call_input(fmt, k, G, n, kinds))
            assert bits_equal(got, fed.process(fmt, C)), (height, fmt, cid)
            fed.close()
    _close(eng, ors)


@pytest.mark.parametrize("fmt", QC.FMTS)
@pytest.mark.parametrize("variant", ["native", "optimized"])
def test_single_filter_saturation(variant, fmt):
    """xl_fir_q15_kernel through process_<variant>_<fmt>_cs16 at D = 42, 21 and 7 (odd m D: the window starts of odd outputs are not
    8-byte aligned, the kernel's single-sample loads), full-scale and noise blocks of several lengths over seven calls"""
    for shape, fc in QC.SINGLE_SHAPES:
        f = xl.XlatingFilter(QC.SHAPE_D[shape], QC.taps(shape), fc, QC.FS, QC.MAXIN)
        o = _oracle(shape, fc)
        for k, (n, kind) in enumerate(QC.SINGLE_CALLS):
            x = QC.call_input(fmt, k, 1, n, (kind,))
            got, want = f.process(variant, fmt, "cs16", x), o.process(fmt, x, "cs16")
            assert _same(got, want), (variant, fmt, shape, k, _first_difference(got, want))
        f.close()
        o.close()


@pytest.mark.parametrize("fmt", QC.WRAP_FMTS)
def test_engine_wrap(fmt):
    """xl_wide_q15_kernel on windows of 65000 (saturates, never wraps), 65700 and 70000 taps of 0.9999 at D = 1000: constant full-scale
    blocks and a full-scale tone for the client at fc = 500.  The reference cuts sum >> 15 to 32 bits before it saturates
    (xlating.c:118: saturate_to_int16 takes an int32_t), so a sum past 2^31 - 1 comes out at the other end of int16."""
    maxin = 2 * QC.WRAP_SAMPLES
    eng = xl.BatchEngine(QC.FS, fmt, maxin)
    eng.set_option("max_window", QC.WRAP_MAX_WINDOW)
    ors = {}
    for name, T, fc in QC.WRAP_CASES:
        ors[eng.add_client(QC.WRAP_D, QC.wrap_taps(T), fc)] = Oracle(QC.WRAP_D, QC.wrap_taps(T), fc, QC.FS, maxin)
    assert "wide: 4 clients" in eng.describe(), eng.describe()
    for b in range(len(QC.WRAP_BLOCKS)):
        _q15_call(eng, ors, fmt, QC.wrap_block(fmt, b), 1, (fmt, QC.WRAP_BLOCKS[b]))
    _close(eng, ors)


def test_single_filter_wrap():
    """xl_fir_q15_kernel (int64 sums) at 70000 taps: the same blocks, the same cut"""
    maxin = 2 * QC.WRAP_SAMPLES
    for fc in (0, 500):
        f = xl.XlatingFilter(QC.WRAP_D, QC.wrap_taps(70000), fc, QC.FS, maxin)
        o = Oracle(QC.WRAP_D, QC.wrap_taps(70000), fc, QC.FS, maxin)
        for b in range(len(QC.WRAP_BLOCKS)):
            x = QC.wrap_block("cs16", b)
            got, want = f.process("native", "cs16", "cs16", x), o.process("cs16", x, "cs16")
            assert _same(got, want), (fc, b, _first_difference(got, want))
        f.close()
        o.close()


@pytest.mark.parametrize("fmt", QC.FMTS)
def test_mixing_families_native(fmt):
    """include/xlating_batch.h at XL_MODE_Q15: the engine keeps ONE raw history behind both families (the reference keeps a sample
    buffer per family behind one counter).  Calls A (native), A (Q15), C (native), every decimation dividing the blocks: the history
    before C is A's tail either way, so C's outputs and the phase after it are those of an oracle fed (A, C); the Q15 call is the
    restatement started on A's tail with a fresh Q15 phase."""
    A, C = QC.mix_blocks(fmt)
    eng, ors = _engine(fmt, QC.MIX_CLIENTS)
    qa = QR.convert(fmt, A)
    eng.process_host(A, "native")
    eng.fetch()
    for cid, o in ors.items():
        assert bits_equal(eng.output(cid), o.process(fmt, A)), (fmt, cid)
    eng.process_host(A, "q15")
    eng.fetch()
    for cid, o in ors.items():
        T = o.rtaps_q15.shape[0]
        want = QR.of_oracle(o, history=qa[qa.shape[0] - (T - 1):]).process(fmt, A)
        got = eng.output_cs16(cid)
        assert _same(got, want), (fmt, cid, _first_difference(got, want))
    eng.process_host(C, "native")
    eng.fetch()
    for cid, o in ors.items():
        assert bits_equal(eng.output(cid), o.process(fmt, C)), (fmt, cid)
        assert eng.phase(cid) == o.phase, (fmt, cid)
    _close(eng, ors)


def test_mixing_families_optimized():
    """the same with optimized calls of two blocks and a class of 70 clients: the polyphase path with the next call's phase table
    tabulated ahead on the side stream, which a Q15 call drops (xl_call_q15).  Calls (A, C) optimized, (A, C) Q15, (C, A) optimized,
    (A, C) optimized: the optimized outputs within the project's 1e-5 of an oracle fed the optimized calls' blocks, the Q15 call
    exactly the restatement started on the first call's tail."""
    fmt = "cu8"
    A, C = QC.mix_blocks(fmt)
    eng, ors = _engine(fmt, QC.MIX_CLIENTS_BIG, group_blocks=2)
    qc = QR.convert(fmt, C)

    def optimized(blocks, tag):
        eng.process_host_group(np.concatenate(blocks), 2, "optimized")
        eng.fetch()
        for cid, o in ors.items():
            want = np.concatenate([o.process(fmt, bl) for bl in blocks])
            got = eng.output(cid)
            assert got.shape == want.shape, (tag, cid)
            err = float(np.abs(got.astype(np.complex128) - want).max() / np.abs(want).max())
            assert err <= REL_TOL, (tag, cid, err)
            assert eng.phase(cid) == o.phase, (tag, cid)

    optimized((A, C), 0)
    assert "polyphase: cls0 D42 T505 cols70" in eng.describe(), eng.describe()
    eng.process_host_group(np.concatenate((A, C)), 2, "q15")
    eng.fetch()
    for cid, o in ors.items():
        T = o.rtaps_q15.shape[0]
        s = QR.of_oracle(o, history=qc[qc.shape[0] - (T - 1):])
        want = np.concatenate([s.process(fmt, A), s.process(fmt, C)])
        got = eng.output_cs16(cid)
        assert _same(got, want), (cid, _first_difference(got, want))
    optimized((C, A), 2)
    optimized((A, C), 3)
    _close(eng, ors)


@pytest.mark.parametrize("seed,fmt", QC.CHURN_RUNS)
def test_q15_churn(seed, fmt):
    """clients of five shapes join, leave and take over freed slots between Q15 calls of 1 .. 3 blocks of 2 .. 65536 elements, each
    block noise, a square wave or a constant extreme: every client against an oracle created at its join"""
    eng = xl.BatchEngine(QC.FS, fmt, QC.MAXIN, group_blocks=3)
    cid_of, ors, seen = {}, {}, set()
    reused = False
    for k, (joins, leaves, G, n, kinds) in enumerate(QC.churn_schedule(seed)):
        for u in leaves:
            cid = cid_of.pop(u)
            eng.remove_client(cid)
            ors.pop(cid).close()
        for u, shape, fc in joins:
            cid = eng.add_client(QC.SHAPE_D[shape], QC.taps(shape), fc)
            reused |= cid in seen
            seen.add(cid)
            cid_of[u] = cid
            ors[cid] = _oracle(shape, fc)
        assert eng.num_clients == len(ors)
        _q15_call(eng, ors, fmt, QC.call_input(fmt, k, G, n, kinds), G, (seed, k))
    assert reused
    _close(eng, ors)
