"""GPU tests (-m gpu) of the polyphase path at the LOW end of the integer formats' range, and of level steps between the blocks of one call.

The two-half matrix-core mix (xl_mixh.hip / xl_mixh2.hip) scales the shared spectra of a cu8 / cs8 / cs16 stream by the constant
XLP_H_XSCALE = 128, so on a quiet stream the second halves of its operands are float16 SUBNORMALS: a 1-LSB cs16 sample is 2^-15, its
spectrum values times 128 are about 2^-8, their second halves 2^-19 .. 2^-24.  Every step that carries them -- the float32 -> float16
conversions of xlp_split_h, the LDS pack, the operand image the forward launch writes (option "mix_operand_image"), the matrix
instruction -- must keep them: tests/test_mix_split_model.py shows on the CPU that with the halves' subnormals flushed such streams
miss the bar by 6 to 24 times, while full-scale input (all the other tests of the path use) cannot tell.  Here the kernels themselves
run those streams, every client and every block against the oracle at the path's bar, max|d| <= 1e-5 max|y| of the block.

Blocks are 32768 complex samples (D = 42, D = 21) and 65536 (D = 100): at least 512 outputs per block (below that a call stays on the
direct kernel: xl_batch.cpp, use_poly), at least two overlap-save segments per block, and block ends inside segments (neither size is
a multiple of V x D = 10248 / 5124 / 6200).  Each test prints its worst figures (pytest -s; profiles/quiet_levels.txt)."""
import functools

import numpy as np
import pytest

import siggen
import sdr_server_amd as xl
from conftest import bits_equal
from pyoracle import Oracle

pytestmark = pytest.mark.gpu
REL_TOL = 1e-5
NCLIENTS = 6
MIN_POLY_OUTPUTS = 512  # (a call with fewer outputs per client falls back to the direct kernel)


@functools.lru_cache(maxsize=None)
def _shape(name):
    """-> (fs, D, taps, complex samples per block, the plan describe() must show)"""
    if name == "S42":      # the server default: 505 taps, 6 k-blocks of 8 branches (xl_mixh.hip)
        fs, D, n = 2016000, 42, 32768
        code, taps = xl.create_low_pass_filter(1.0, fs, 24000, 9600)
    elif name == "S21":    # 253 taps, 3 k-blocks
        fs, D, n = 2016000, 21, 32768
        code, taps = xl.create_low_pass_filter(1.0, fs, 48000, 19200)
    else:                  # S100: 257 taps, 13 k-blocks: the wide kernel (xl_mixh2.hip), 64-point transforms
        fs, D, n = 10000000, 100, 65536
        code, taps = 0, siggen.hamming_sinc(257, 0.004)
    assert code == 0 and len(taps) == {"S42": 505, "S21": 253, "S100": 257}[name]
    return fs, D, taps, n, "polyphase: cls0 D%d T%d cols%d " % (D, len(taps), NCLIENTS)


def _fcs(fs):
    return [int(-0.45 * fs + (0.9 * fs / (NCLIENTS - 1)) * c) - 17 * c for c in range(NCLIENTS)]  # spread over +-0.45 fs


# mix arms: (option, value) pairs and what describe() must say
ARMS = {"halves": ((("mix_operand_image", 0),), " mix=mfma "), "halves-img": ((("mix_operand_image", 1),), " mix=mfma/img "),
        "f32": ((("mix_kernel", 3),), " mix=mf32 ")}


def _engine(monkeypatch, shape, fmt, arm, group_blocks):
    fs, D, taps, n, plan = _shape(shape)
    monkeypatch.setenv("XL_EXP_POLY", "1")
    eng = xl.BatchEngine(fs, fmt, 2 * n, group_blocks=group_blocks)
    for name, value in ARMS[arm][0]:
        eng.set_option(name, value)
    ids = [eng.add_client(D, taps, fc) for fc in _fcs(fs)]
    d = eng.describe() + " "
    assert plan in d and ARMS[arm][1] in d, d
    return eng, ids


def _oracles(shape):
    fs, D, taps, n, _ = _shape(shape)
    return [Oracle(D, taps, fc, fs, 2 * n) for fc in _fcs(fs)]


def _dtype(fmt):
    return {"cu8": np.uint8, "cs8": np.int8, "cs16": np.int16, "cf32": np.float32}[fmt]


def _iq(fmt, i, q):
    """Raw sample values of I and Q, interleaved, in the format's type."""
    x = np.empty(2 * len(i), np.float64)
    x[0::2], x[1::2] = i, q
    return x.astype(_dtype(fmt))


def _lsb_noise(fmt, rng, n, lsb):
    lo, hi = (128 - lsb, 128 + lsb) if fmt == "cu8" else (-lsb, lsb + 1)  # cu8: 127 / 128 are +-0.5 LSB, 126 .. 129 +-1.5
    return _iq(fmt, rng.integers(lo, hi, n), rng.integers(lo, hi, n))


def _err(got, want):
    return float(np.abs(got.astype(np.complex128) - want.astype(np.complex128)).max())


# ---------------------------------------------------------------------------------------------------------------
# (a), (b): whole streams that are quiet from their first sample on
QUIET_KINDS = {"cs16": ["lsb1-noise", "lsb2-noise", "lsb1-impulse", "lsb1-every-977th", "zeros"], "cs8": ["lsb1-noise"],
               "cu8": ["lsb1-noise"]}


def _quiet_blocks(fmt, shape, kind):
    """Eight blocks of one kind: four one-block calls, then one call of four blocks."""
    n = _shape(shape)[3]
    rng = np.random.default_rng(1000 * _shape(shape)[1] + QUIET_KINDS["cs16"].index(kind))
    out = []
    for k in range(8):
        if kind.endswith("-noise"):
            out.append(_lsb_noise(fmt, rng, n, int(kind[3])))
            continue
        i = np.zeros(n)
        if kind == "lsb1-impulse":
            i[n // 3 + 1237 * k] = 1    # (mid-block: every block holds a whole response and nothing else)
        elif kind == "lsb1-every-977th":
            i[(k * n + np.arange(n)) % 977 == 0] = 1
        out.append(_iq(fmt, i, np.zeros(n)))
    return out


@functools.lru_cache(maxsize=None)
def _quiet_want(fmt, shape, kind):
    """The oracle's outputs [client][block], computed once for all arms."""
    blocks = _quiet_blocks(fmt, shape, kind)
    want = []
    for o in _oracles(shape):
        want.append([o.process(fmt, xb) for xb in blocks])
        o.close()
    return want


_QUIET_GOT = {}


def _quiet_got(monkeypatch, fmt, shape, arm, kind):
    """A fresh engine's outputs [client][block]: four one-block calls, then the other four blocks as one call (kept for the tests
    that compare arms)."""
    key = (fmt, shape, arm, kind)
    if key in _QUIET_GOT:
        return _QUIET_GOT[key]
    blocks = _quiet_blocks(fmt, shape, kind)
    eng, ids = _engine(monkeypatch, shape, fmt, arm, 4)
    got = [[] for _ in ids]
    for k in range(4):
        eng.process_host(blocks[k], "optimized")
        eng.fetch()
        for c, cid in enumerate(ids):
            got[c].append(eng.output(cid).copy())
    eng.process_host_group(np.concatenate(blocks[4:]), 4, "optimized")
    eng.fetch()
    for c, cid in enumerate(ids):
        y, off = eng.output(cid), 0
        for g in range(4):
            k = eng.output_len_block(cid, g)
            got[c].append(y[off:off + k].copy())
            off += k
        assert off == len(y), (cid, off, len(y))
    eng.close()
    _QUIET_GOT[key] = got
    return got


QUIET_CASES = [(fmt, shape, arm) for fmt in ("cs16", "cs8", "cu8") for shape in ("S42", "S21", "S100")
               for arm in (("halves", "halves-img", "f32") if shape != "S100" else ("halves", "f32"))]


@pytest.mark.parametrize("fmt,shape,arm", QUIET_CASES, ids=lambda v: str(v))
def test_quiet_streams_whole_calls(fmt, shape, arm, monkeypatch):
    """Streams that never hold more than an LSB or two (fresh engines: zero history, nothing louder anywhere): +-1 LSB noise, and for
    cs16 also +-2 LSB noise, a lone 1-LSB impulse per block, 1-LSB samples every 977th, and all zeros -- whose outputs are exact zeros,
    as the reference's.  Four one-block calls and one call of four blocks per kind; every client, every block, at 1e-5 of the block's
    own max|y| (which is asserted to be above zero), on the converting staging, the operand image (where the form exists: up to 8
    k-blocks) and the float32 mix as the control."""
    worst = {}
    for kind in QUIET_KINDS[fmt]:
        want = _quiet_want(fmt, shape, kind)
        got = _quiet_got(monkeypatch, fmt, shape, arm, kind)
        worst[kind] = 0.0
        for c in range(NCLIENTS):
            for k in range(8):
                g, w = got[c][k], want[c][k]
                assert len(g) == len(w) >= MIN_POLY_OUTPUTS, (kind, c, k, len(g), len(w))
                if kind == "zeros":
                    assert not w.any() and not g.any(), (kind, c, k, _err(g, w))
                    continue
                scale = float(np.abs(w).max())
                assert scale > 0.0, (kind, c, k)
                worst[kind] = max(worst[kind], _err(g, w) / scale)
        print("quiet_levels whole_calls %s %s %s %s worst %.3g" % (fmt, shape, arm, kind, worst[kind]))
    assert all(e <= REL_TOL for e in worst.values()), (fmt, shape, arm, worst)


@pytest.mark.parametrize("kind", ["lsb1-noise", "lsb1-impulse"])
@pytest.mark.parametrize("shape", ["S42", "S21"])
def test_operand_image_arm_is_bit_identical_on_quiet_input(shape, kind, monkeypatch):
    """The image the forward launch writes holds the halves the converting staging would make, subnormal ones included: same bits out
    (tests/test_mix_operand_image_gpu.py shows it on full-scale noise, where few halves are subnormal and none of them
    matters to the bar; here every second half is)."""
    old = _quiet_got(monkeypatch, "cs16", shape, "halves", kind)
    new = _quiet_got(monkeypatch, "cs16", shape, "halves-img", kind)
    for c in range(NCLIENTS):
        for k in range(8):
            assert np.abs(old[c][k]).max() > 0.0, (c, k)
            assert bits_equal(new[c][k], old[c][k]), (c, k, _err(new[c][k], old[c][k]))


# ---------------------------------------------------------------------------------------------------------------
# (c): level steps between the blocks of ONE call of an integer stream
STEP_KINDS = ["lsb2-noise", "full-scale-noise", "silence", "full-scale-impulse", "lsb1-noise", "full-scale-square", "lsb1-impulse",
              "noise-30dBFS"]


def _step_blocks(fmt, n):
    """A warm-up block of mid-level noise and the eight blocks of STEP_KINDS, in raw sample values.  A cu8 stream has no zero (its
    samples are (x - 127.5) / 128), so its silence -- the background of its impulses too -- is random 127 / 128, and its 1-LSB impulse
    one sample of 129."""
    rng = np.random.default_rng(2024)
    lo, hi = np.iinfo(_dtype(fmt)).min, np.iinfo(_dtype(fmt)).max
    zero = 127.5 if fmt == "cu8" else 0.0

    def uniform():
        return rng.integers(lo, hi + 1, n)

    def gauss(rms):  # rms as a fraction of full scale
        return np.clip(np.rint(zero + rng.standard_normal(n) * rms * (hi - zero)), lo, hi)

    def silence():
        return rng.integers(127, 129, n) if fmt == "cu8" else np.zeros(n)

    def impulse(level):
        i = silence()
        i[n // 3 + 77] = level
        return _iq(fmt, i, silence())

    square = np.where(np.arange(n) % 200 < 100, hi, lo if fmt == "cu8" else -hi)
    blocks = [_lsb_noise(fmt, rng, n, 2), _iq(fmt, uniform(), uniform()), _iq(fmt, silence(), silence()), impulse(hi),
              _lsb_noise(fmt, rng, n, 1), _iq(fmt, square, square), impulse(129 if fmt == "cu8" else 1),
              _iq(fmt, gauss(10.0 ** (-30 / 20.0)), gauss(10.0 ** (-30 / 20.0)))]
    return _iq(fmt, gauss(0.1), gauss(0.1)), blocks


@functools.lru_cache(maxsize=None)
def _step_want(fmt, shape):
    """-> (warm-up outputs [client], first pass [client][block], second pass [client][block]) of the oracle"""
    warm, blocks = _step_blocks(fmt, _shape(shape)[3])
    ww, w1, w2 = [], [], []
    for o in _oracles(shape):
        ww.append(o.process(fmt, warm))
        w1.append([o.process(fmt, xb) for xb in blocks])
        w2.append([o.process(fmt, xb) for xb in blocks])
        o.close()
    return ww, w1, w2


def _own_scale(scale, near):
    """The documented rule (test_cf32_two_half_mix_adversarial_levels_in_one_call): a block is held to 1e-5 of its own max|y|
    unless a neighbouring block's output scale is more than 100 x larger -- then to 1e-5 of that."""
    return near <= 100.0 * scale


@pytest.mark.parametrize("fmt,shape", [("cs16", "S42"), ("cu8", "S42"), ("cs8", "S42"), ("cs16", "S100")], ids=lambda v: str(v))
def test_integer_level_steps_in_one_call(fmt, shape, monkeypatch):
    """include/xlating_batch.h promises of a call of 8 blocks the results of 8 successive reference calls.  One such call whose blocks are
    +-2 LSB noise, full-scale noise, silence, a lone full-scale impulse, +-1 LSB noise, a full-scale square wave (period 200 samples),
    a lone 1-LSB impulse and noise at -30 dBFS, behind one warm-up block; every client PER BLOCK against the oracle under the rule of
    the cf32 test -- 1e-5 of the block's own max|y|, of the louder neighbour's where that is more than 100 x larger (an overlap-save
    segment spans the block end) --, with the two-half and with the float32 mix; then the same blocks one per call, where only the
    PREVIOUS block shares a segment.  At least five of the eight blocks are held to their own scale for every client (from the oracle
    alone: the block behind a loud one starts with that one's filter tail, which is its scale)."""
    n = _shape(shape)[3]
    warm, blocks = _step_blocks(fmt, n)
    want_warm, want, want2 = _step_want(fmt, shape)
    for c in range(NCLIENTS):
        sc = [float(np.abs(w).max()) for w in want[c]]
        assert min(len(w) for w in want[c]) >= MIN_POLY_OUTPUTS
        own = [_own_scale(sc[g], max(sc[max(g - 1, 0)], sc[min(g + 1, 7)])) for g in range(8)]
        assert sum(own) >= 5, (c, sc, own)
    for arm in ("halves", "f32"):
        eng, ids = _engine(monkeypatch, shape, fmt, arm, 8)
        eng.process_host(warm, "optimized")
        eng.fetch()
        for c in range(NCLIENTS):
            g = eng.output(ids[c])
            assert len(g) == len(want_warm[c]) and _err(g, want_warm[c]) <= REL_TOL * float(np.abs(want_warm[c]).max()), (arm, c)
        eng.process_host_group(np.concatenate(blocks), 8, "optimized")
        eng.fetch()
        worst = [0.0] * 8
        for c in range(NCLIENTS):
            got = eng.output(ids[c])
            lens = [eng.output_len_block(ids[c], g) for g in range(8)]
            assert lens == [len(w) for w in want[c]], (c, lens)
            scale = [float(np.abs(w).max()) for w in want[c]]
            off = 0
            for g in range(8):
                gb, wb = got[off:off + lens[g]], want[c][g]
                off += lens[g]
                near = max(scale[max(g - 1, 0)], scale[min(g + 1, 7)])
                ref = scale[g] if _own_scale(scale[g], near) else near
                assert ref > 0.0
                e = _err(gb, wb) / ref
                worst[g] = max(worst[g], e)
                assert e <= REL_TOL, (fmt, shape, arm, c, g, STEP_KINDS[g], e, "own scale" if ref == scale[g] else "neighbour's scale")
        print("quiet_levels level_steps %s %s %s one-call   %s" % (fmt, shape, arm, " ".join("%.2g" % e for e in worst)))
        worst = [0.0] * 8
        for g in range(8):  # the same blocks, one per call
            eng.process_host(blocks[g], "optimized")
            eng.fetch()
            for c in range(NCLIENTS):
                wb, gb = want2[c][g], eng.output(ids[c])
                assert len(gb) == len(wb)
                sc = [float(np.abs(w).max()) for w in want2[c]]
                prev = sc[g - 1] if g > 0 else float(np.abs(want[c][7]).max())
                ref = sc[g] if _own_scale(sc[g], prev) else prev
                e = _err(gb, wb) / ref
                worst[g] = max(worst[g], e)
                assert e <= REL_TOL, (fmt, shape, arm, c, g, STEP_KINDS[g], "one block per call", e)
        print("quiet_levels level_steps %s %s %s eight-calls %s" % (fmt, shape, arm, " ".join("%.2g" % e for e in worst)))
        eng.close()


# ---------------------------------------------------------------------------------------------------------------
# (d): cf32 streams far from unit level: the clamps of xlp_seg_exp and the powers xlp_seg_scale / xlp_seg_unscale build from it
@pytest.mark.parametrize("exponent", [-60, 60])
@pytest.mark.parametrize("shape", ["S100", "S42"])
def test_cf32_segment_scale_at_far_exponents(shape, exponent, monkeypatch):
    """A cf32 stream of noise at amplitude 2^-60, another at 2^+60 (test_cf32_two_half_mix_adversarial_levels_in_one_call spans 1e-6 ..
    3e4): fresh engines, three one-block calls, every client at 1e-5 of its own scale, two-half mix and float32 mix."""
    n = _shape(shape)[3]
    rng = np.random.default_rng(60 + exponent)
    blocks = [(rng.standard_normal(2 * n) * 0.3).astype(np.float32) * np.float32(2.0 ** exponent) for _ in range(3)]
    want = []
    for o in _oracles(shape):
        want.append([o.process("cf32", xb) for xb in blocks])
        o.close()
    for arm, opts in (("halves", ()), ("f32", ARMS["f32"][0])):
        fs, D, taps, _, plan = _shape(shape)
        monkeypatch.setenv("XL_EXP_POLY", "1")
        eng = xl.BatchEngine(fs, "cf32", 2 * n)
        for name, value in opts:
            eng.set_option(name, value)
        ids = [eng.add_client(D, taps, fc) for fc in _fcs(fs)]
        d = eng.describe() + " "
        assert plan in d and ARMS[arm][1] in d, d
        worst = 0.0
        for k, xb in enumerate(blocks):
            eng.process_host(xb, "optimized")
            eng.fetch()
            for c in range(NCLIENTS):
                g, w = eng.output(ids[c]), want[c][k]
                scale = float(np.abs(w).max())
                assert len(g) == len(w) >= MIN_POLY_OUTPUTS and np.isfinite(scale) and scale > 0.0, (arm, c, k, scale)
                worst = max(worst, _err(g, w) / scale)
        eng.close()
        print("quiet_levels far_exponents cf32 %s %s 2^%d worst %.3g" % (shape, arm, exponent, worst))
        assert worst <= REL_TOL, (shape, arm, exponent, worst)
