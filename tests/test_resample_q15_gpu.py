"""GPU tests (-m gpu) of the Q15 resampler bank (include/xlating_resample_q15.h).  The arithmetic is exact, so EVERY comparison is
np.array_equal against the integer restatement (tests/resample_q15_ref.py): no tolerance anywhere.  The index edges, the admitted
filters and the edges of the tiling (256-output tiles, a 4096-sample LDS span, 1024-sample carry slots, a 4096-entry LDS tap table)
under two splits of the input, saturation, the boundary between the 32-bit and the 64-bit sums, many streams in one feed, the bank's
housekeeping, the bank behind the batch engine's XL_MODE_Q15 rows, a cs16 spectrum bank fed from its device rows, and
tools/replay_iq.py --variant q15 --any-rate.
One stream here ("1/40", L = 1) reads its window in place.  The span limit itself, M % L != 0 in place, a tap table and a window both
in place, 64-bit sums over an in-place window and M = 2^31 - 1 are tests/test_resample_edges_gpu.py's (streams from
tests/resample_edges.py)."""
import errno
import functools
import importlib.util
import math
import os

import numpy as np
import pytest

import resample_q15_ref as QR
import resample_ref as RR
import sdr_server_amd as xl
from conftest import ROOT

pytestmark = pytest.mark.gpu

BAND_FREQ = 460100000


def admission(fs, fo, center=BAND_FREQ + 1000):
    """-> (request, admission, L, M, the second stage's taps) as xlating_wire_admit_any_rate and xlating_wire_resample_taps answer"""
    req = xl.WireRequest(center, fo, BAND_FREQ, 0)
    code, adm, rs, why = xl.wire_admit_any_rate(req, fs, 0, 5)
    assert code == 0, (fs, fo, why)
    if (rs.L, rs.M) == (1, 1):
        return req, adm, 1, 1, None  # no second stage
    code, taps = xl.wire_resample_taps(req, rs, 5)
    assert code == 0
    return req, adm, rs.L, rs.M, taps


def windowed_sinc(n, L, cutoff):
    """a float32 low-pass of n taps at `cutoff` (cycles per sample of the upsampled grid), gain L"""
    k = np.arange(n) - (n - 1) / 2
    h = np.sinc(2 * cutoff * k) * np.hamming(n)
    return (h * (L / h.sum())).astype(np.float32)


def full_range(n, seed):
    """int16 [n, 2], uniform over the whole range, -32768 and odd negative values among the first samples"""
    rng = np.random.default_rng(seed)
    x = rng.integers(-32768, 32768, (n, 2)).astype(np.int16)
    head = np.array([[-32768, -3], [-1, -32767], [32767, -32768], [1, 3], [-5, 0]], np.int16)
    x[:min(n, 5)] = head[:min(n, 5)]
    return x


def to_device(x, lead=0):
    """x (int16 [N, 2]) on the device behind `lead` complex samples of padding -> (tensor kept alive, address of x[0])"""
    import torch

    raw = np.concatenate([np.full(2 * lead, 77, np.int16), np.ascontiguousarray(x, dtype=np.int16).reshape(-1)])
    t = torch.from_numpy(raw).cuda()
    return t, t.data_ptr() + 4 * lead


def stream():
    import torch

    return torch.cuda.current_stream().cuda_stream


def feed_pieces(bank, sid, L, M, addr, pieces, start=0):
    """feed one stream piece by piece from stream position `start` (addr: the address of stream sample 0); the count of every feed is
    the formula's; -> all its outputs, int16 [n, 2]"""
    pos, outs = start, [np.zeros((0, 2), np.int16)]
    for c in pieces:
        c = int(c)
        before = bank.produced(sid)
        bank.feed([sid], [addr + 4 * pos], [c], stream())
        want = RR.counts(L, M, pos + c) - RR.counts(L, M, pos)
        assert bank.produced(sid) - before == want
        assert bank.output_device(sid)[1] == want
        bank.fetch()
        o = bank.output(sid)
        assert o.dtype == np.int16 and o.shape == (want, 2), (L, M, pos, c, o.shape, want)
        outs.append(o)
        pos += c
    return np.concatenate(outs)


def split(N, sizes):
    """N cut into the given sizes, the last piece taking what is left"""
    out, left = [], N
    for s in sizes:
        s = min(int(s), left)
        out.append(s)
        left -= s
    out.append(left)
    return out


def exact(y, L, M, taps, x, what=""):
    want = QR.restate(L, M, taps, x)
    assert y.dtype == np.int16 and y.shape == want.shape, (what, y.shape, want.shape)
    bad = np.nonzero((y != want).any(axis=1))[0]
    assert bad.size == 0, (what, L, M, bad.size, bad[:5], y[bad[:5]], want[bad[:5]])


# ------------------------------------------------------------------------------------------------------------ identity and index edges
def test_identity_and_index_edges():
    x = full_range(5000, 1)
    keep, addr = to_device(x)
    bank = xl.ResamplerBankQ15()
    half = np.full(1, 0.5, np.float32)  # c = 16384: y = x >> 1, the floor
    assert xl.resample_q15_quantize(half).tolist() == [16384]
    pieces = split(x.size // 2, [1, 255, 256, 257, 2000])
    a, b, c = bank.add(1, 1, half), bank.add(1, 3, half), bank.add(3, 1, half)
    ya = feed_pieces(bank, a, 1, 1, addr, pieces)
    assert np.array_equal(ya, x >> 1) and ya[0, 1] == -2  # (-3 >> 1 == -2)
    yb = feed_pieces(bank, b, 1, 3, addr, pieces)
    assert np.array_equal(yb, x[::3] >> 1)  # decimation by picking: n_m = 3 m
    yc = feed_pieces(bank, c, 3, 1, addr, pieces)
    want = np.zeros((3 * x.shape[0], 2), np.int16)
    want[::3] = x >> 1  # zero-stuffing: phase 0 holds the tap, phases 1 and 2 nothing
    assert np.array_equal(yc, want)
    for y, (L, M) in ((ya, (1, 1)), (yb, (1, 3)), (yc, (3, 1))):
        exact(y, L, M, half, x, f"identity {L}/{M}")
    bank.close()


# ------------------------------------------------------------------------------------------------------------ edges, exact
def edge_cases():
    yield "2/3", *admission(2400000, 1600000)[2:], 6000
    yield "7/8", *admission(2016000, 44100)[2:], 20000
    yield "3/5", *admission(10000000, 48000)[2:], 20000
    yield "147/160", *admission(2400000, 44100)[2:], 20000
    yield "624/625", 624, 625, windowed_sinc(7500, 624, 0.45 / 625), 20000
    rng = np.random.default_rng(3)
    yield "4096/4095", 4096, 4095, (rng.integers(-32768, 32768, 4096) / 32768.0).astype(np.float32), 20000
    yield "Q1024", 1, 2, windowed_sinc(1024, 1, 0.22), 20000
    yield "1/40", 1, 40, windowed_sinc(64, 1, 0.45 / 40), 30000


EDGES = list(edge_cases())
EDGE = {e[0]: e[1:] for e in EDGES}
NAMES = [e[0] for e in EDGES]


def edge_pieces(name):
    L, M, taps, N = EDGE[name]
    Q = -(-taps.size // L)
    return split(N, [Q - 1, 1, 300, 4097])


@functools.lru_cache(maxsize=None)
def edge_input(name):
    x = full_range(EDGE[name][3], 100 + EDGE[name][0])
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def edge_first_split(name):
    """the edge's outputs under its first split, computed once and shared by the tests that need them"""
    L, M, taps, N = EDGE[name]
    keep, addr = to_device(edge_input(name))
    bank = xl.ResamplerBankQ15()
    sid = bank.add(L, M, taps)
    y = feed_pieces(bank, sid, L, M, addr, edge_pieces(name))
    assert y.shape[0] == RR.counts(L, M, N) == bank.produced(sid)
    bank.close()
    y.setflags(write=False)
    return y


def test_edge_cases_are_what_they_are_meant_to_be():
    """conditions on the inputs: which path of the kernel each case takes"""
    facts = {}
    for name, (L, M, taps, N) in EDGE.items():
        assert math.gcd(L, M) == 1 and (name[0] == "Q" or name == f"{L}/{M}")
        Q = -(-taps.size // L)
        facts[name] = (Q, taps.size, int(np.abs(QR.quantize(taps)).max()), int(QR.phase_abs_sums(L, taps).max()))
    assert facts["2/3"][0] == 19 and facts["7/8"][0] == 14 and facts["3/5"][0] == 21
    assert facts["147/160"][:2] == (14, 1927) and 2048 < 147 * 14 <= 4096  # a 4 KB table, staged in LDS
    assert facts["624/625"][:3] == (13, 7500, 29420) and 624 * 13 > 4096  # a table read in place
    assert facts["4096/4095"][0] == 1 and facts["4096/4095"][1] == 4096  # the largest table LDS takes
    assert facts["Q1024"][0] == 1024 and facts["Q1024"][3] == 99580  # > 65535: the wide accumulator is forced
    assert 255 * 40 + 64 > 4096  # 1/40: the tile's window is read in place
    for name in ("2/3", "7/8", "3/5", "147/160", "624/625", "1/40"):
        assert facts[name][3] <= 65535, name  # the 32-bit path


@pytest.mark.parametrize("name", NAMES)
def test_edges_equal_the_restatement(name):
    L, M, taps, N = EDGE[name]
    exact(edge_first_split(name), L, M, taps, edge_input(name), name)


@pytest.mark.parametrize("name", NAMES)
def test_a_second_split_is_bit_identical(name):
    L, M, taps, N = EDGE[name]
    Q = -(-taps.size // L)
    x = edge_input(name)
    keep, addr = to_device(x, lead=3)  # an odd element offset: 4-byte aligned only
    rng = np.random.default_rng(300 + M)
    menu = [0, 1, 2, max(Q - 2, 0), Q - 1, Q, 255, 256, 257, 4096]
    sizes = list(menu) + [int(v) for v in rng.choice(menu, 30)]
    rng.shuffle(sizes)
    assert split(N, sizes) != edge_pieces(name)
    bank = xl.ResamplerBankQ15()
    sid = bank.add(L, M, taps)
    y = feed_pieces(bank, sid, L, M, addr, split(N, sizes))
    bank.close()
    assert np.array_equal(y, edge_first_split(name)), name


@pytest.mark.parametrize("knob", ["1", "2", "3"])
def test_the_measurement_knob_changes_no_bit(monkeypatch, knob):
    """XL_EXP_RSQ (tools/resample_bank_bench.py --q15: 1 = every sum in 64 bits, 2 = every tap table read in place) switches off
    what the kernel chose for a run; the sums are exact either way"""
    name = "147/160"  # by itself: 32-bit sums, the table in LDS
    L, M, taps, N = EDGE[name]
    keep, addr = to_device(edge_input(name))
    monkeypatch.setenv("XL_EXP_RSQ", knob)
    bank = xl.ResamplerBankQ15()
    monkeypatch.delenv("XL_EXP_RSQ")
    sid = bank.add(L, M, taps)
    y = feed_pieces(bank, sid, L, M, addr, split(N, [5000, 13]))
    bank.close()
    assert np.array_equal(y, edge_first_split(name))


# ------------------------------------------------------------------------------------------------------------ saturation, accumulators
def test_saturation_with_the_admitted_147_160_filter():
    _, _, L, M, taps = admission(2400000, 44100)
    assert (L, M) == (147, 160)
    N, Q = 3000, 14
    for re, im in ((-32768, 32767), (32767, -32768)):
        x = np.empty((N, 2), np.int16)
        x[:, 0], x[:, 1] = re, im
        s = QR.sums(L, M, taps, x)[Q:] >> 15  # past the start-up samples
        for k in range(2):  # a condition on the inputs: some outputs clip and some do not, in both components
            clipped = (s[:, k] > 32767) | (s[:, k] < -32768)
            assert clipped.any() and not clipped.all(), (re, im, k)
        keep, addr = to_device(x)
        bank = xl.ResamplerBankQ15()
        sid = bank.add(L, M, taps)
        y = feed_pieces(bank, sid, L, M, addr, split(N, [700, 1]))
        bank.close()
        exact(y, L, M, taps, x, f"saturation {re} {im}")
        assert (y[Q:, 0] == re).any() and (y[Q:, 0] != re).any()


def test_accumulator_boundary():
    """sum |c| = 65535 is the last table the 32-bit sums may take (largest sum 2^31 - 32768); 65536 reaches 2^31 exactly, where a
    wrapped 32-bit sum would give -32768"""
    N = 600
    x = np.full((N, 2), -32768, np.int16)
    keep, addr = to_device(x)
    bank = xl.ResamplerBankQ15()
    for c, total, largest in (((-32767, -32767, -1), 65535, 2 ** 31 - 32768), ((-32767, -32767, -2), 65536, 2 ** 31)):
        taps = (np.array(c, np.float64) / 32768.0).astype(np.float32)
        assert QR.quantize(taps).tolist() == list(c) and QR.phase_abs_sums(1, taps).tolist() == [total]
        assert QR.sums(1, 1, taps, x).max() == largest
        sid = bank.add(1, 1, taps)
        y = feed_pieces(bank, sid, 1, 1, addr, split(N, [1, 1, 300]))
        exact(y, 1, 1, taps, x, f"sum |c| {total}")
        assert (y[2:] == 32767).all(), total
    bank.close()


def test_wide_accumulator():
    Q, N = 1024, 3000
    rng = np.random.default_rng(64)
    taps = (rng.choice([-32767, 32767], Q) / 32768.0).astype(np.float32)
    x = rng.choice(np.array([-32768, 32767], np.int16), (N, 2))
    assert QR.phase_abs_sums(1, taps).tolist() == [Q * 32767]
    want = QR.restate(1, 1, taps, x)
    assert (want == 32767).any() and (want == -32768).any() and np.abs(QR.sums(1, 1, taps, x)).max() > 2 ** 32
    keep, addr = to_device(x)
    bank = xl.ResamplerBankQ15()
    sid = bank.add(1, 1, taps)
    y = feed_pieces(bank, sid, 1, 1, addr, split(N, [Q - 1, 1, 300]))
    bank.close()
    assert np.array_equal(y, want)


# ------------------------------------------------------------------------------------------------------------ many streams
def mixed_population(n):
    """n streams over seven ratios and tap sets -- 32-bit and 64-bit sums, tables in LDS, one and many taps per phase -- with two feeds
    of different counts each"""
    wide = np.array([0.99, -0.99, 0.99, 0.99, -0.99, 0.99, -0.99, 0.99], np.float32)
    kinds = [admission(2016000, 44100)[2:], admission(10000000, 48000)[2:], admission(2400000, 1600000)[2:],
             (1, 1, np.full(1, 0.5, np.float32)), (1, 3, windowed_sinc(40, 1, 0.15)), (3, 1, windowed_sinc(31, 3, 0.15)), (1, 2, wide)]
    assert QR.phase_abs_sums(1, wide)[0] > 65535
    rng = np.random.default_rng(n)
    out = []
    for i in range(n):
        L, M, taps = kinds[i % len(kinds)]
        c0, c1 = int(rng.integers(0, 900)), int(rng.integers(1, 900))
        if i % 17 == 3:
            c0 = 0
        if i % 19 == 5:
            c1 = 1
        out.append((L, M, taps, c0, c1, full_range(c0 + c1, 5000 + i)))
    return out


@pytest.mark.parametrize("n", [1, 8, 300])
def test_many_streams_equal_each_stream_alone(n):
    pop = mixed_population(n)
    dev = [to_device(p[5]) for p in pop]
    bank, alone = xl.ResamplerBankQ15(), xl.ResamplerBankQ15()
    sids = [bank.add(L, M, taps) for L, M, taps, *_ in pop]
    assert bank.stats()[:2] == (n, min(n, 7))
    got = [[] for _ in pop]
    for f in range(2):
        counts = [p[3 + f] for p in pop]
        ptrs = [d[1] + (4 * p[3] if f else 0) for d, p in zip(dev, pop)]
        bank.feed(sids, ptrs, counts, stream())
        if n > 1:
            assert bank.last_feed_ops() == (2, 1)
        bank.fetch()
        for i, sid in enumerate(sids):
            got[i].append(bank.output(sid))
    for i, (L, M, taps, c0, c1, x) in enumerate(pop):
        y = np.concatenate(got[i])
        sid = alone.add(L, M, taps)
        want = feed_pieces(alone, sid, L, M, dev[i][1], [c0, c1])
        alone.remove(sid)
        assert np.array_equal(y, want), (i, L, M)
        if i < 14:
            exact(y, L, M, taps, x, f"stream {i} of {n}")
    bank.close()
    alone.close()


def test_a_feed_of_single_tap_streams_is_one_launch():
    x = full_range(700, 12)
    keep, addr = to_device(x)
    bank = xl.ResamplerBankQ15()
    half = np.full(1, 0.5, np.float32)
    a, b, c = bank.add(1, 1, half), bank.add(3, 1, np.full(3, 0.25, np.float32)), bank.add(7, 8, windowed_sinc(97, 7, 0.4 / 8))
    bank.feed([a, b], [addr, addr], [700, 300], stream())
    assert bank.last_feed_ops() == (1, 1)  # no stream of the feed has Q > 1: no carry launch
    bank.feed([a, b, c], [addr, addr, addr], [0, 0, 0], stream())
    assert bank.last_feed_ops() == (0, 0)
    bank.feed([a, c], [addr, addr], [10, 10], stream())
    assert bank.last_feed_ops() == (2, 1)
    bank.close()


# ------------------------------------------------------------------------------------------------------------ the tables' and carries' lifetimes
def alone(bank, L, M, taps, addr, pieces):
    """the oracle of the three tests below: the stream by itself in `bank` (which holds nothing else), fed the same pieces with a
    fetch behind every feed -> its outputs per piece"""
    sid = bank.add(L, M, taps)
    outs, pos = [], 0
    for c in pieces:
        bank.feed([sid], [addr + 4 * pos], [c], stream())
        bank.fetch()
        outs.append(bank.output(sid))
        pos += c
    bank.remove(sid)
    return outs


def test_carry_array_grows_under_live_carries():
    """64 streams hold a carry (Q = 21) from a feed that nothing has waited for when the 65th is added: the array of carry slots is
    replaced by one of 128 and the carries move over"""
    _, _, L, M, taps = admission(10000000, 48000)
    assert (L, M) == (3, 5) and -(-taps.size // L) == 21
    first, second = [300 + i for i in range(65)], [200 + 2 * i for i in range(65)]
    dev = [to_device(full_range(first[i] + second[i], 7000 + i)) for i in range(65)]
    bank, ref = xl.ResamplerBankQ15(), xl.ResamplerBankQ15()
    sids = [bank.add(L, M, taps) for _ in range(64)]
    bank.feed(sids, [d[1] for d in dev[:64]], first[:64], stream())
    sids.append(bank.add(L, M, taps))
    assert sids == list(range(65))
    bank.feed(sids, [d[1] + 4 * c for d, c in zip(dev[:64], first)] + [dev[64][1]], second[:64] + [first[64] + second[64]], stream())
    bank.fetch()
    for i, sid in enumerate(sids):
        want = alone(ref, L, M, taps, dev[i][1], [first[i], second[i]])
        assert np.array_equal(bank.output(sid), want[1] if i < 64 else np.concatenate(want)), i
    bank.close()
    ref.close()


def test_six_feeds_in_a_row_reuse_the_pinned_tables():
    """the ring holds four pinned tables: the fifth and the sixth feed write tables that earlier feeds were uploaded from, and nothing
    on the host waits in between"""
    _, _, L, M, taps = admission(10000000, 48000)
    pieces = [300, 200, 257, 100, 333, 150]
    keep, addr = to_device(full_range(sum(pieces), 41))
    bank, ref = xl.ResamplerBankQ15(), xl.ResamplerBankQ15()
    sid = bank.add(L, M, taps)
    pos = 0
    for c in pieces:
        bank.feed([sid], [addr + 4 * pos], [c], stream())
        assert bank.last_feed_ops() == (2, 1)
        pos += c
    bank.fetch()
    assert bank.produced(sid) == RR.counts(L, M, pos)
    got, want = bank.output(sid), alone(ref, L, M, taps, addr, pieces)[-1]  # (which every earlier feed's carry has gone into)
    assert got.shape == want.shape and want.shape[0] > 0 and np.array_equal(got, want)
    bank.close()
    ref.close()


def test_device_table_grows_between_feeds():
    """a feed of 2 streams, then one that names 5 -- more than twice the table the first allocated -- while nothing has waited for
    the first, then a third"""
    _, _, L, M, taps = admission(10000000, 48000)
    counts = [[300, 310, 0, 0, 0], [200, 210, 220, 230, 240], [150, 160, 170, 180, 190]]
    dev = [to_device(full_range(sum(c[i] for c in counts), 43 + i)) for i in range(5)]
    bank, ref = xl.ResamplerBankQ15(), xl.ResamplerBankQ15()
    sids = [bank.add(L, M, taps) for _ in range(5)]
    want = [alone(ref, L, M, taps, dev[i][1], [c[i] for c in counts]) for i in range(5)]
    pos = [0] * 5
    for f, c in enumerate(counts):
        named = [i for i in range(5) if c[i] > 0]
        bank.feed([sids[i] for i in named], [dev[i][1] + 4 * pos[i] for i in named], [c[i] for i in named], stream())
        pos = [p + v for p, v in zip(pos, c)]
        if f > 0:
            bank.fetch()
            for i in named:
                got = bank.output(sids[i])
                assert got.shape == want[i][f].shape and got.shape[0] > 0 and np.array_equal(got, want[i][f]), (f, i)
    bank.close()
    ref.close()


# ------------------------------------------------------------------------------------------------------------ housekeeping
def test_equal_definitions_share_one_table():
    _, _, L, M, taps = admission(2016000, 44100)
    bank = xl.ResamplerBankQ15()
    sids = [bank.add(L, M, taps.copy()) for _ in range(300)]
    Q = -(-taps.size // L)
    assert bank.stats() == (300, 1, L * Q * 2)
    other = taps.copy()
    other.view(np.uint32)[-1] ^= 1  # one FLOAT tap differs in its last bit (the quantised taps need not): sharing is by the float taps
    extra = bank.add(L, M, other)
    assert bank.stats() == (301, 2, 2 * L * Q * 2)
    bank.remove(extra)
    assert bank.stats() == (300, 1, L * Q * 2)
    _, _, L3, M3, taps3 = admission(10000000, 48000)
    three = bank.add(L3, M3, taps3)
    assert bank.stats() == (301, 2, L * Q * 2 + 126)  # the admitted 3 / 5 table is 126 bytes
    bank.remove(three)
    for sid in sids:
        bank.remove(sid)
    assert bank.stats() == (0, 0, 0)
    bank.close()


def test_membership_and_refusals():
    _, _, L, M, taps = admission(2016000, 44100)
    x = full_range(3000, 9)
    keep, addr = to_device(x)
    bank, fbank = xl.ResamplerBankQ15(), xl.ResamplerBank()
    R = xl.resample_q15_lib()
    one = np.full(1, 0.5, np.float32)
    for args in [(0, 1, one), (1, 0, one), (2, 4, one), (6, 9, one), (4097, 4096, one), (1, 1 << 31, one), (1, 1, np.zeros(0, np.float32)),
                 (1, 2, np.full(1025, 0.5, np.float32)), (4, 3, np.full(4 * 1024 + 1, 0.5, np.float32))]:
        with pytest.raises(xl.XlatingError) as e:
            bank.add(*args)
        assert e.value.code == -errno.EINVAL, args[:2]
    assert R.xlating_resample_q15_bank_add(bank.h, 1, 1, None, 1) == -errno.EINVAL
    for bad in (np.ones(1, np.float32), np.array([0.5, np.nan], np.float32), np.array([np.inf], np.float32),
                np.array([0.25, -1.0001], np.float32)):
        with pytest.raises(xl.XlatingError) as e:
            bank.add(1, 1, bad)
        assert e.value.code == -errno.ERANGE, bad
    with pytest.raises(xl.XlatingError) as e:
        bank.add(2, 4, np.ones(1, np.float32))  # the arguments are judged first
    assert e.value.code == -errno.EINVAL
    assert bank.stats() == (0, 0, 0)
    assert bank.add(1, 1, np.array([-1.0], np.float32)) == 0  # h = -1.0 is accepted
    bank.remove(0)
    assert bank.add(4, 3, np.full(4 * 1024, 0.5, np.float32)) == 0  # Q = 1024, L M at their limits of the list above
    bank.remove(0)
    a, b = bank.add(L, M, taps), bank.add(L, M, taps)
    fa = fbank.add(L, M, taps)
    first = feed_pieces(bank, a, L, M, addr, [1000, 700])
    feed_pieces(bank, b, L, M, addr, [500])
    # refused calls consume nothing
    before = (bank.produced(a), bank.produced(b))
    for ids, counts in [([a, a], [10, 10]), ([a, b, a], [1, 1, 1]), ([a, 7], [10, 10]), ([-1], [10]), ([a, b], [10, (1 << 30) + 1])]:
        with pytest.raises(xl.XlatingError) as e:
            bank.feed(ids, [addr] * len(ids), counts, stream())
        assert e.value.code == -errno.EINVAL, (ids, counts)
        assert (bank.produced(a), bank.produced(b)) == before
    with pytest.raises(xl.XlatingError) as e:
        bank.add(L, M, np.ones(3, np.float32))
    assert e.value.code == -errno.ERANGE and (bank.produced(a), bank.produced(b)) == before and bank.stats()[:2] == (2, 1)
    # a handle of the other family is refused by every function, and nothing is consumed
    F = xl.resample_lib()
    ids_, ptrs_, counts_ = (np.array([v], t) for v, t in ((a, np.intc), (addr, np.uint64), (10, np.uint64)))
    import ctypes as C

    p, n, u = C.c_void_p(), C.c_size_t(0), C.c_uint(0)
    f32p, i16p = C.POINTER(C.c_float)(), C.POINTER(C.c_int16)()
    assert F.xlating_resample_bank_add(bank.h, L, M, taps.ctypes.data, taps.size) == -errno.EINVAL
    assert F.xlating_resample_bank_feed_device(bank.h, 1, ids_.ctypes.data, ptrs_.ctypes.data, counts_.ctypes.data, stream()) == -errno.EINVAL
    assert F.xlating_resample_bank_remove(bank.h, a) == -errno.EINVAL
    assert F.xlating_resample_bank_output_device(bank.h, a, C.byref(p), C.byref(n)) == -errno.EINVAL
    assert F.xlating_resample_bank_fetch(bank.h) == -errno.EINVAL
    assert F.xlating_resample_bank_output_host(bank.h, a, C.byref(f32p), C.byref(n)) == -errno.EINVAL
    assert F.xlating_resample_bank_produced(bank.h, a) == 0
    assert F.xlating_resample_bank_last_feed_ops(bank.h, C.byref(u), C.byref(u)) == -errno.EINVAL
    assert F.xlating_resample_bank_stats(bank.h, C.byref(u), C.byref(u), C.byref(n)) == -errno.EINVAL
    ids_[0] = fa
    assert R.xlating_resample_q15_bank_add(fbank.h, L, M, taps.ctypes.data, taps.size) == -errno.EINVAL
    assert R.xlating_resample_q15_bank_feed_device(fbank.h, 1, ids_.ctypes.data, ptrs_.ctypes.data, counts_.ctypes.data, stream()) == -errno.EINVAL
    assert R.xlating_resample_q15_bank_remove(fbank.h, fa) == -errno.EINVAL
    assert R.xlating_resample_q15_bank_output_device(fbank.h, fa, C.byref(p), C.byref(n)) == -errno.EINVAL
    assert R.xlating_resample_q15_bank_fetch(fbank.h) == -errno.EINVAL
    assert R.xlating_resample_q15_bank_output_host(fbank.h, fa, C.byref(i16p), C.byref(n)) == -errno.EINVAL
    assert R.xlating_resample_q15_bank_produced(fbank.h, fa) == 0
    assert R.xlating_resample_q15_bank_last_feed_ops(fbank.h, C.byref(u), C.byref(u)) == -errno.EINVAL
    assert R.xlating_resample_q15_bank_stats(fbank.h, C.byref(u), C.byref(u), C.byref(n)) == -errno.EINVAL
    assert (bank.produced(a), bank.produced(b)) == before and fbank.produced(fa) == 0
    assert bank.stats()[:2] == (2, 1) and fbank.stats()[:2] == (1, 1)
    fbank.close()
    bank.remove(b)
    with pytest.raises(xl.XlatingError) as e:
        bank.feed([b], [addr], [10], stream())  # a dead id
    assert e.value.code == -errno.EINVAL
    with pytest.raises(xl.XlatingError):
        bank.remove(b)
    # the stream that went on is untouched by all that
    rest = feed_pieces(bank, a, L, M, addr, [1300], start=1700)
    exact(np.concatenate([first, rest]), L, M, taps, x, "survivor")
    # a reused id starts at m = 0 with zero history
    bank.remove(a)
    again = bank.add(L, M, taps)
    assert again in (a, b) and bank.produced(again) == 0
    y = feed_pieces(bank, again, L, M, addr, [40, 2960])
    exact(y, L, M, taps, x, "reused id")
    bank.close()


def test_output_rows_and_arena_growth():
    _, _, L, M, taps = admission(10000000, 48000)
    x = full_range(18000, 21)
    keep, addr = to_device(x)
    bank, reader = xl.ResamplerBankQ15(), xl.ResamplerBankQ15()
    a, b = bank.add(L, M, taps), bank.add(L, M, taps)
    half = np.full(1, 0.5, np.float32)
    tap = reader.add(1, 1, half)  # reads a device row: a one-tap stream of another bank, y = row >> 1
    outs = {a: [], b: []}
    pos = 0
    for c in (300, 0, 15000, 2700):  # the third feed is 50 times the first: the arena grows
        bank.feed([a, b], [addr + 4 * pos, addr + 4 * pos], [c, c // 2], stream())
        rows = {}
        for sid in (a, b):
            p, n = bank.output_device(sid)
            assert (p is None) == (n == 0)
            reader.feed([tap], [p or 0], [n], stream())  # the row is readable until the bank's next feed
            reader.fetch()
            rows[sid] = reader.output(tap)
        bank.fetch()
        for sid in (a, b):
            assert np.array_equal(bank.output(sid) >> 1, rows[sid])
            assert np.array_equal(bank.output(sid) >> 1, rows[sid])  # (output_host may be asked again)
            outs[sid].append(bank.output(sid))
        pos += c
    exact(np.concatenate(outs[a]), L, M, taps, x, "row a")
    # a stream the latest feed did not name has no outputs of that feed
    bank.feed([a], [addr], [0], stream())
    assert bank.output_device(b) == (None, 0) and bank.output_device(a) == (None, 0)
    bank.fetch()
    assert bank.output(b).shape == (0, 2)
    bank.close()
    reader.close()


# ------------------------------------------------------------------------------------------------------------ behind the engine
def tones_u8(n, band_rate, freqs, seed):
    """a cu8 band of n samples: one tone per frequency (Hz from the band's centre), equal amplitudes, a little noise"""
    rng = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64) / band_rate
    z = np.exp(2j * np.pi * np.asarray(freqs, dtype=np.float64)[:, None] * t[None, :]).sum(axis=0) * (0.8 / len(freqs))
    z += 0.002 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    v = np.stack([z.real, z.imag], axis=1).reshape(-1)
    return np.clip(np.round(127.5 + 127 * v), 0, 255).astype(np.uint8)


class DeviceRow:
    """n int16 pairs at a device address, as torch.as_tensor reads foreign device memory"""

    def __init__(self, ptr, n):
        self.__cuda_array_interface__ = {"shape": (n, 2), "typestr": "<i2", "data": (ptr, False), "strides": None, "version": 2}


def device_bytes(ptr, n):
    """the int16 pairs at a device address -> int16 [n, 2] on the host (behind the current stream's work)"""
    import torch

    if not n:
        return np.zeros((0, 2), np.int16)
    return torch.as_tensor(DeviceRow(ptr, n), device="cuda").clone().cpu().numpy()


def test_behind_the_batch_engine():
    import torch

    band, nbytes, nblocks = 2016000, 8192, 6
    offsets = {"a": 100000, "int": -200000, "b": 300000}
    rates = {"a": 44100, "int": 48000, "b": 44100}
    x = tones_u8(nblocks * nbytes // 2, band, [off + 3000 for off in offsets.values()], 4)
    blocks = [torch.from_numpy(c).cuda() for c in np.split(x, nblocks)]
    eng = xl.BatchEngine(band, "cu8", nbytes)
    bank = xl.ResamplerBankQ15()
    clients = {}
    for k, fo in rates.items():
        req, adm, L, M, taps = admission(band, fo, center=BAND_FREQ + offsets[k])
        cid = xl.wire_add_client(eng, adm, band)
        assert cid >= 0
        clients[k] = dict(cid=cid, adm=adm, L=L, M=M, taps=taps, sid=None if (L, M) == (1, 1) else bank.add(L, M, taps), mid=[], out=[])
    assert all((clients[k]["adm"].decimation, clients[k]["L"], clients[k]["M"]) == (40, 7, 8) for k in "ab")
    assert (clients["int"]["adm"].decimation, clients["int"]["sid"]) == (42, None)
    assert bank.stats()[:2] == (2, 1)  # the two 44.1 kHz clients share one table
    second = {c["cid"]: c["sid"] for c in clients.values() if c["sid"] is not None}
    for d in blocks:
        eng.process_device(d.data_ptr(), nbytes, "q15", stream())
        bank.feed_engine(eng, second, stream())
        assert bank.last_feed_ops() == (2, 1)
        dev = {k: device_bytes(*eng.output_device(c["cid"])) for k, c in clients.items()}
        eng.fetch()
        bank.fetch()
        for k, c in clients.items():
            row = eng.output_cs16(c["cid"])
            # output_device after a Q15 call points at the int16 row output_cs16 returns: the same count, the same bytes
            assert eng.output_device(c["cid"])[1] == row.shape[0] == eng.output_len(c["cid"])
            assert dev[k].dtype == np.int16 and np.array_equal(dev[k], row), k
            c["mid"].append(row)
            if c["sid"] is not None:
                c["out"].append(bank.output(c["sid"]))
    for k, c in clients.items():
        mid = np.concatenate(c["mid"])
        assert mid.shape[0] > 0 and np.abs(mid.astype(np.int32)).max() > 1000
        if c["sid"] is None:
            continue
        y = np.concatenate(c["out"])
        assert y.shape[0] == RR.counts(7, 8, mid.shape[0]) == -(-mid.shape[0] * 7 // 8) == bank.produced(c["sid"])
        exact(y, c["L"], c["M"], c["taps"], mid, f"client {k}")  # the restatement applied to the engine's own cs16 outputs
    bank.close()
    eng.close()


# ------------------------------------------------------------------------------------------------------------ composition
def test_cs16_spectrum_bank_fed_from_the_resamplers_rows():
    _, _, L, M, taps = admission(2016000, 44100)
    W, rate = 64, 44100
    N = 2 * rate * M // L + 900  # two rows and a little at 44.1 kHz
    t = np.arange(N) / (rate * M / L)
    z = 9000 * np.exp(2j * np.pi * 5000 * t)
    rng = np.random.default_rng(33)
    x = np.round(np.stack([z.real, z.imag], axis=1) + rng.standard_normal((N, 2)) * 200).astype(np.int16)
    keep, addr = to_device(x)
    bank, sbank = xl.ResamplerBankQ15(), xl.SpectrumBank(W, "cs16")
    sid, wid = bank.add(L, M, taps), sbank.add(rate)
    outs, pos = [], 0
    for c in split(N, [20000, 1, 33000, 257, 20000]):
        bank.feed([sid], [addr + 4 * pos], [c], stream())
        p, n = bank.output_device(sid)
        sbank.feed([wid], [p or 0], [n], stream())
        bank.fetch()
        outs.append(bank.output(sid))
        pos += c
    y = np.concatenate(outs)
    exact(y, L, M, taps, x, "spectrum input")
    db, px = sbank.take_rows(wid)
    one = xl.Spectrum(rate, W, "cs16")
    one.feed(y.reshape(-1))
    want_db, want_px = one.take_rows()
    one.close()
    assert db.shape[0] == 2 and db.shape == want_db.shape
    assert np.array_equal(db.view(np.uint32), want_db.view(np.uint32)) and np.array_equal(px, want_px)
    bank.close()
    sbank.close()


# ------------------------------------------------------------------------------------------------------------ replay
def test_replay_q15_any_rate(tmp_path):
    spec = importlib.util.spec_from_file_location("replay_iq", os.path.join(ROOT, "tools", "replay_iq.py"))
    replay_iq = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(replay_iq)
    # --gzip is the sinks library's work: refused with q15, by the argument parser and by replay()
    with pytest.raises(SystemExit) as e:
        replay_iq.parse_args(["x.cu8", "--band-freq", "1", "--out", str(tmp_path), "--variant", "q15", "--gzip"])
    assert e.value.code == 2
    assert replay_iq.parse_args(["x.cu8", "--band-freq", "1", "--out", str(tmp_path), "--variant", "q15"]).variant == "q15"
    assert replay_iq.parse_args(["x.cu8", "--band-freq", "1", "--out", str(tmp_path), "--gzip"]).variant == "optimized"
    with pytest.raises(ValueError):
        replay_iq.replay("x.cu8", "cu8", 192000, BAND_FREQ, [], str(tmp_path / "no"), variant="q15", gzip=True)
    band_rate, buffer_size, W = 192000, 65536, 64
    reqs = [(BAND_FREQ + 12000, 44100), (BAND_FREQ - 20000, 48000)]
    nsamp = 2 * band_rate + 1234
    raw = tones_u8(nsamp, band_rate, [12000 + 3000, -20000 - 1500], 8)
    path = tmp_path / "capture.cu8"
    raw.tofile(path)
    adm, rej, st = replay_iq.replay(str(path), "cu8", band_rate, BAND_FREQ, reqs, str(tmp_path / "any"), buffer_size, 5, "q15",
                                    waterfall_width=W, any_rate=True)
    assert sorted(adm.values()) == sorted(reqs) and rej == [] and st["blocks_dropped"] == 0
    by_rate = {rate: cid for cid, (_, rate) in adm.items()}
    got = {rate: np.fromfile(tmp_path / "any" / f"{cid}.cs16", dtype=np.int16).reshape(-1, 2) for rate, cid in by_rate.items()}
    assert st["bytes_written"] == 4 * sum(g.shape[0] for g in got.values())
    assert not any(f.endswith((".cf32", ".gz")) for f in os.listdir(tmp_path / "any"))
    # the restated chain: the engine's own cs16 streams at D, then the restatement for the fractional client
    mids = {}
    eng = xl.BatchEngine(band_rate, "cu8", buffer_size)
    wadm = {}
    for center, rate in reqs:
        req, wadm[rate], L, M, taps = admission(band_rate, rate, center=center)
        mids[rate] = (xl.wire_add_client(eng, wadm[rate], band_rate), L, M, taps, [])
    assert (wadm[44100].decimation, mids[44100][1], mids[44100][2]) == (4, 147, 160) and mids[48000][1:3] == (1, 1)
    for off in range(0, raw.size, buffer_size):
        eng.process_host(raw[off:off + buffer_size], "q15")
        eng.fetch()
        for cid, L, M, taps, rows in mids.values():
            rows.append(eng.output_cs16(cid))
    eng.close()
    assert np.array_equal(got[48000], np.concatenate(mids[48000][4]))  # the integer client: the engine's samples as they are
    cid, L, M, taps, rows = mids[44100]
    exact(got[44100], L, M, taps, np.concatenate(rows), "replay")
    # the fractional client's waterfall is the spectrogram of its .cs16 at 44.1 kHz
    import spectrogram_ref as SR

    y = got[44100]
    H = y.shape[0] // 44100
    assert H >= 2
    px = SR.decode_png(str(tmp_path / "any" / f"{by_rate[44100]}.png"))
    one = xl.Spectrum(44100, W, "cs16")
    one.feed(y.reshape(-1))
    want = one.take_rows()[1]
    one.close()
    assert px.shape == (H, W) and np.array_equal(px, want[:H])
    assert os.path.exists(tmp_path / "any" / f"{by_rate[48000]}.png")
