"""GPU tests (-m gpu) of the resampler bank (include/xlating_resample.h): every output within the DERIVED bound of the float64
restatement (tests/resample_ref.py: |y32 - y64| <= gamma_Q S + Q 2^-126 per component, no measured tolerance), the output count per
feed, bit-identity under any split of the input and in any company of streams, table sharing, membership, the output rows, the
tables and the carries when their arrays grow and when the ring of pinned tables wraps, the bank behind the batch engine at the rates
the admission rule picks, a spectrum bank fed from its device rows, and tools/replay_iq.py --any-rate.
The streams here have M / L <= 3: every tile's window is staged in LDS.  The windows read in place, the span limit itself and the
splits that move a tile across it are tests/test_resample_edges_gpu.py's (streams from tests/resample_edges.py)."""
import errno
import importlib.util
import math
import os

import numpy as np
import pytest

import resample_ref as RR
import sdr_server_amd as xl
from conftest import ROOT, bits_equal

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


def noise(n, seed):
    rng = np.random.default_rng(seed)
    return (0.5 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64)


def to_device(x, lead=0):
    """x (complex64) on the device behind `lead` complex samples of padding -> (tensor kept alive, address of x[0])"""
    import torch

    raw = np.concatenate([np.full(2 * lead, 7.0, np.float32), np.ascontiguousarray(x).view(np.float32)])
    t = torch.from_numpy(raw).cuda()
    return t, t.data_ptr() + 8 * lead


def stream():
    import torch

    return torch.cuda.current_stream().cuda_stream


def feed_pieces(bank, sid, L, M, addr, pieces, start=0):
    """feed one stream piece by piece from stream position `start` (addr: the address of stream sample 0); the count of every feed is
    the formula's; -> all its outputs"""
    pos, outs = start, []
    for c in pieces:
        c = int(c)
        before = bank.produced(sid)
        bank.feed([sid], [addr + 8 * pos], [c], stream())
        want = RR.counts(L, M, pos + c) - RR.counts(L, M, pos)
        assert bank.produced(sid) - before == want
        assert bank.output_device(sid)[1] == want
        bank.fetch()
        o = bank.output(sid)
        assert o.size == want, (L, M, pos, c, o.size, want)
        outs.append(o)
        pos += c
    return np.concatenate(outs) if outs else np.zeros(0, np.complex64)


def split(N, sizes):
    """N cut into the given sizes, the last piece taking what is left"""
    out, left = [], N
    for s in sizes:
        s = min(int(s), left)
        out.append(s)
        left -= s
    out.append(left)
    return out


# ------------------------------------------------------------------------------------------------------------ identity and index edges
def test_identity_and_picking():
    x = noise(5000, 1)
    keep, addr = to_device(x)
    bank = xl.ResamplerBank()
    one = np.ones(1, np.float32)
    a, b, c = bank.add(1, 1, one), bank.add(1, 3, one), bank.add(3, 1, one)
    ya = feed_pieces(bank, a, 1, 1, addr, split(x.size, [1, 255, 256, 257, 2000]))
    assert bits_equal(ya, x)  # L = M = 1, one tap of 1.0: the input, bit for bit
    yb = feed_pieces(bank, b, 1, 3, addr, split(x.size, [1, 1, 1, 2, 1000]))
    assert bits_equal(yb, x[::3])  # decimation by picking: n_m = 3 m
    yc = feed_pieces(bank, c, 3, 1, addr, split(x.size, [1, 2, 700]))
    want = np.zeros(3 * x.size, np.complex64)
    want[::3] = x  # zero-stuffing: phase 0 holds the tap, phases 1 and 2 nothing
    assert yc.size == want.size and np.array_equal(yc, want)
    RR.check(yc, 3, 1, one, x, "zero-stuffing")
    bank.close()


def edge_cases():
    yield "2/3", *admission(2400000, 1600000)[2:], 6000
    yield "7/8", *admission(2016000, 44100)[2:], 20000
    yield "3/5", *admission(10000000, 48000)[2:], 20000
    yield "624/625", 624, 625, windowed_sinc(7500, 624, 0.45 / 625), 20000
    rng = np.random.default_rng(3)
    yield "4096/4095", 4096, 4095, rng.standard_normal(4096).astype(np.float32), 20000
    yield "Q1024", 1, 2, windowed_sinc(1024, 1, 0.22), 20000


EDGES = list(edge_cases())


@pytest.mark.parametrize("name,L,M,taps,N", EDGES, ids=[e[0] for e in EDGES])
def test_within_the_derived_bound(name, L, M, taps, N):
    assert math.gcd(L, M) == 1 and (name[0] == "Q" or name == f"{L}/{M}")
    Q = -(-taps.size // L)
    assert {"2/3": Q > 1, "624/625": taps.size == 7500 and Q == 13, "4096/4095": Q == 1, "Q1024": Q == 1024}.get(name, Q in (14, 21))
    x = noise(N, 100 + L)
    keep, addr = to_device(x)
    bank = xl.ResamplerBank()
    sid = bank.add(L, M, taps)
    y = feed_pieces(bank, sid, L, M, addr, split(N, [Q - 1, 1, 300, 4097]))
    assert y.size == RR.counts(L, M, N) == bank.produced(sid)
    RR.check(y, L, M, taps, x, name)
    bank.close()


def test_admitted_filters_meet_the_projects_bar():
    """for the admitted filters (Q <= 21) the derived bound is below 1e-5 of the stream's peak"""
    for fs, fo in [(10000000, 48000), (2016000, 44100), (2400000, 44100), (2048000, 48000), (2400000, 2000000)]:
        _, _, L, M, taps = admission(fs, fo)
        x = noise(4000, fo)
        y, sr, si = RR.restate(L, M, taps, x)
        Q = -(-taps.size // L)
        assert Q <= 21
        peak = max(np.abs(y.real).max(), np.abs(y.imag).max())
        assert max(RR.bound(Q, sr).max(), RR.bound(Q, si).max()) < 1e-5 * peak, (fs, fo)


# ------------------------------------------------------------------------------------------------------------ splits
@pytest.mark.parametrize("name,L,M,taps,N", EDGES, ids=[e[0] for e in EDGES])
def test_any_split_is_bit_identical(name, L, M, taps, N):
    N = min(N, 12000)
    Q = -(-taps.size // L)
    x = noise(N, 200 + L)
    keep0, addr0 = to_device(x)
    keep1, addr1 = to_device(x, lead=3)  # an odd element offset: 8-byte aligned only
    rng = np.random.default_rng(300 + M)
    menu = [0, 1, 2, max(Q - 2, 0), Q - 1, Q, 255, 256, 257, 4096]
    sizes = list(menu) + [int(v) for v in rng.choice(menu, 40)]
    rng.shuffle(sizes)
    bank = xl.ResamplerBank()
    s0, s1, s2 = (bank.add(L, M, taps) for _ in range(3))
    whole = feed_pieces(bank, s0, L, M, addr0, [N])
    pieces = feed_pieces(bank, s1, L, M, addr0, split(N, sizes))
    odd = feed_pieces(bank, s2, L, M, addr1, split(N, sizes[::-1]))
    assert whole.size == RR.counts(L, M, N)
    assert bits_equal(whole, pieces), name
    assert bits_equal(whole, odd), name
    bank.close()


# ------------------------------------------------------------------------------------------------------------ many streams
def mixed_population(n):
    """n streams over six ratios and tap sets, with two feeds of different counts each"""
    kinds = [admission(2016000, 44100)[2:], admission(10000000, 48000)[2:], admission(2400000, 1600000)[2:],
             (1, 1, np.ones(1, np.float32)), (1, 3, windowed_sinc(40, 1, 0.15)), (3, 1, windowed_sinc(31, 3, 0.15))]
    rng = np.random.default_rng(n)
    out = []
    for i in range(n):
        L, M, taps = kinds[i % len(kinds)]
        c0, c1 = int(rng.integers(0, 900)), int(rng.integers(1, 900))
        if i % 17 == 3:
            c0 = 0
        if i % 19 == 5:
            c1 = 1
        out.append((L, M, taps, c0, c1, noise(c0 + c1, 5000 + i)))
    return out


@pytest.mark.parametrize("n", [1, 8, 300])
def test_many_streams_equal_each_stream_alone(n):
    pop = mixed_population(n)
    dev = [to_device(p[5]) for p in pop]
    bank, alone = xl.ResamplerBank(), xl.ResamplerBank()
    sids = [bank.add(L, M, taps) for L, M, taps, *_ in pop]
    assert bank.stats()[:2] == (n, min(n, 6))
    got = [[] for _ in pop]
    for f in range(2):
        counts = [p[3 + f] for p in pop]
        ptrs = [d[1] + (8 * p[3] if f else 0) for d, p in zip(dev, pop)]
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
        assert bits_equal(y, want), (i, L, M)
        if i < 12:
            RR.check(y, L, M, taps, x, f"stream {i} of {n}")
    bank.close()
    alone.close()


def test_equal_definitions_share_one_table():
    _, _, L, M, taps = admission(2016000, 44100)
    bank = xl.ResamplerBank()
    sids = [bank.add(L, M, taps.copy()) for _ in range(300)]
    Q = -(-taps.size // L)
    assert bank.stats() == (300, 1, L * Q * 4)
    other = taps.copy()
    other.view(np.uint32)[-1] ^= 1  # one tap differs in its last bit
    extra = bank.add(L, M, other)
    assert bank.stats() == (301, 2, 2 * L * Q * 4)
    bank.remove(extra)
    assert bank.stats() == (300, 1, L * Q * 4)
    for sid in sids:
        bank.remove(sid)
    assert bank.stats() == (0, 0, 0)
    bank.close()


# ------------------------------------------------------------------------------------------------------------ membership
def test_membership_and_refusals():
    _, _, L, M, taps = admission(2016000, 44100)
    x = noise(3000, 9)
    keep, addr = to_device(x)
    bank = xl.ResamplerBank()
    R = xl.resample_lib()
    one = np.ones(1, np.float32)
    for args in [(0, 1, one), (1, 0, one), (2, 4, one), (6, 9, one), (4097, 4096, one), (1, 1 << 31, one), (1, 1, np.zeros(0, np.float32)),
                 (1, 2, np.ones(1025, np.float32)), (4, 3, np.ones(4 * 1024 + 1, np.float32))]:
        with pytest.raises(xl.XlatingError) as e:
            bank.add(*args)
        assert e.value.code == -errno.EINVAL, args[:2]
    assert R.xlating_resample_bank_add(bank.h, 1, 1, None, 1) == -errno.EINVAL
    assert bank.stats() == (0, 0, 0)
    assert bank.add(4, 3, np.ones(4 * 1024, np.float32)) == 0  # Q = 1024, L M at their limits of the list above
    bank.remove(0)
    a, b = bank.add(L, M, taps), bank.add(L, M, taps)
    first = feed_pieces(bank, a, L, M, addr, [1000, 700])
    feed_pieces(bank, b, L, M, addr, [500])
    # refused feeds consume nothing
    before = (bank.produced(a), bank.produced(b))
    for ids, counts in [([a, a], [10, 10]), ([a, b, a], [1, 1, 1]), ([a, 7], [10, 10]), ([-1], [10]), ([a, b], [10, (1 << 30) + 1])]:
        with pytest.raises(xl.XlatingError) as e:
            bank.feed(ids, [addr] * len(ids), counts, stream())
        assert e.value.code == -errno.EINVAL, (ids, counts)
        assert (bank.produced(a), bank.produced(b)) == before
    bank.remove(b)
    with pytest.raises(xl.XlatingError) as e:
        bank.feed([b], [addr], [10], stream())  # a dead id
    assert e.value.code == -errno.EINVAL
    with pytest.raises(xl.XlatingError):
        bank.remove(b)
    # the stream that went on is untouched by all that
    rest = feed_pieces(bank, a, L, M, addr, [1300], start=1700)
    RR.check(np.concatenate([first, rest]), L, M, taps, x, "survivor")
    # a reused id starts at m = 0 with zero history
    bank.remove(a)
    again = bank.add(L, M, taps)
    assert again in (a, b) and bank.produced(again) == 0
    y = feed_pieces(bank, again, L, M, addr, [40, 2960])
    RR.check(y, L, M, taps, x, "reused id")
    assert bits_equal(y[:first.size], first)
    bank.close()


# ------------------------------------------------------------------------------------------------------------ outputs
def test_output_rows_and_arena_growth():
    _, _, L, M, taps = admission(10000000, 48000)
    x = noise(18000, 21)
    keep, addr = to_device(x)
    bank, ident = xl.ResamplerBank(), xl.ResamplerBank()
    a, b = bank.add(L, M, taps), bank.add(L, M, taps)
    tap = ident.add(1, 1, np.ones(1, np.float32))  # reads a device row back: an identity stream of another bank
    outs = {a: [], b: []}
    pos = 0
    for c in (300, 0, 15000, 2700):  # the third feed is 50 times the first: the arena grows
        bank.feed([a, b], [addr + 8 * pos, addr + 8 * pos], [c, c // 2], stream())
        rows = {}
        for sid in (a, b):
            p, n = bank.output_device(sid)
            assert (p is None) == (n == 0)
            ident.feed([tap], [p or 0], [n], stream())  # the row is readable until the bank's next feed
            ident.fetch()
            rows[sid] = ident.output(tap)
        bank.fetch()
        for sid in (a, b):
            assert bits_equal(bank.output(sid), rows[sid])
            assert bits_equal(bank.output(sid), rows[sid])  # (output_host may be asked again)
            outs[sid].append(rows[sid])
        pos += c
    RR.check(np.concatenate(outs[a]), L, M, taps, x, "row a")
    # a stream the latest feed did not name has no outputs of that feed
    bank.feed([a], [addr], [0], stream())
    assert bank.output_device(b) == (None, 0) and bank.output_device(a) == (None, 0)
    bank.fetch()
    assert bank.output(b).size == 0
    bank.close()
    ident.close()


# ------------------------------------------------------------------------------------------------------------ the tables' and carries' lifetimes
def alone(bank, L, M, taps, addr, pieces):
    """the oracle of the three tests below: the stream by itself in `bank` (which holds nothing else), fed the same pieces with a
    fetch behind every feed -> its outputs per piece"""
    sid = bank.add(L, M, taps)
    outs, pos = [], 0
    for c in pieces:
        bank.feed([sid], [addr + 8 * pos], [c], stream())
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
    dev = [to_device(noise(first[i] + second[i], 7000 + i)) for i in range(65)]
    bank, ref = xl.ResamplerBank(), xl.ResamplerBank()
    sids = [bank.add(L, M, taps) for _ in range(64)]
    bank.feed(sids, [d[1] for d in dev[:64]], first[:64], stream())
    sids.append(bank.add(L, M, taps))
    assert sids == list(range(65))
    bank.feed(sids, [d[1] + 8 * c for d, c in zip(dev[:64], first)] + [dev[64][1]], second[:64] + [first[64] + second[64]], stream())
    bank.fetch()
    for i, sid in enumerate(sids):
        want = alone(ref, L, M, taps, dev[i][1], [first[i], second[i]])
        assert bits_equal(bank.output(sid), want[1] if i < 64 else np.concatenate(want)), i
    bank.close()
    ref.close()


def test_six_feeds_in_a_row_reuse_the_pinned_tables():
    """the ring holds four pinned tables: the fifth and the sixth feed write tables that earlier feeds were uploaded from, and nothing
    on the host waits in between"""
    _, _, L, M, taps = admission(10000000, 48000)
    pieces = [300, 200, 257, 100, 333, 150]
    keep, addr = to_device(noise(sum(pieces), 41))
    bank, ref = xl.ResamplerBank(), xl.ResamplerBank()
    sid = bank.add(L, M, taps)
    pos = 0
    for c in pieces:
        bank.feed([sid], [addr + 8 * pos], [c], stream())
        assert bank.last_feed_ops() == (2, 1)
        pos += c
    bank.fetch()
    assert bank.produced(sid) == RR.counts(L, M, pos)
    assert bits_equal(bank.output(sid), alone(ref, L, M, taps, addr, pieces)[-1])  # (which every earlier feed's carry has gone into)
    bank.close()
    ref.close()


def test_device_table_grows_between_feeds():
    """a feed of 2 streams, then one that names 5 -- more than twice the table the first allocated -- while nothing has waited for
    the first, then a third"""
    _, _, L, M, taps = admission(10000000, 48000)
    counts = [[300, 310, 0, 0, 0], [200, 210, 220, 230, 240], [150, 160, 170, 180, 190]]
    dev = [to_device(noise(sum(c[i] for c in counts), 43 + i)) for i in range(5)]
    bank, ref = xl.ResamplerBank(), xl.ResamplerBank()
    sids = [bank.add(L, M, taps) for _ in range(5)]
    want = [alone(ref, L, M, taps, dev[i][1], [c[i] for c in counts]) for i in range(5)]
    pos = [0] * 5
    for f, c in enumerate(counts):
        named = [i for i in range(5) if c[i] > 0]
        bank.feed([sids[i] for i in named], [dev[i][1] + 8 * pos[i] for i in named], [c[i] for i in named], stream())
        pos = [p + v for p, v in zip(pos, c)]
        if f > 0:
            bank.fetch()
            for i in named:
                assert bits_equal(bank.output(sids[i]), want[i][f]), (f, i)
    bank.close()
    ref.close()


# ------------------------------------------------------------------------------------------------------------ behind the engine
def tones_u8(n, band_rate, freqs, seed):
    """a cu8 band of n samples: one tone per frequency (Hz from the band's centre), equal amplitudes, a little noise"""
    rng = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64) / band_rate
    z = np.exp(2j * np.pi * np.asarray(freqs, dtype=np.float64)[:, None] * t[None, :]).sum(axis=0) * (0.8 / len(freqs))
    z += 0.002 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    v = np.stack([z.real, z.imag], axis=1).reshape(-1)
    return np.clip(np.round(127.5 + 127 * v), 0, 255).astype(np.uint8)


def test_behind_the_batch_engine():
    import torch

    band, nbytes, G, ncalls = 2016000, 100002, 2, 4
    rates = {44100: 100000, 48000: -200000, 25000: 400000}  # rate -> centre offset
    x = tones_u8(ncalls * G * nbytes // 2, band, [off + 3000 for off in rates.values()], 4)
    calls = [torch.from_numpy(c).cuda() for c in np.split(x, ncalls)]
    eng = xl.BatchEngine(band, "cu8", nbytes, group_blocks=G)
    bank = xl.ResamplerBank()
    clients = {}
    for fo, off in rates.items():
        req, adm, L, M, taps = admission(band, fo, center=BAND_FREQ + off)
        cid = xl.wire_add_client(eng, adm, band)
        assert cid >= 0
        clients[fo] = dict(cid=cid, adm=adm, L=L, M=M, taps=taps, sid=None if (L, M) == (1, 1) else bank.add(L, M, taps), mid=[], out=[])
    assert (clients[44100]["adm"].decimation, clients[44100]["L"], clients[44100]["M"]) == (40, 7, 8)
    assert (clients[48000]["adm"].decimation, clients[48000]["sid"]) == (42, None)
    assert (clients[25000]["adm"].decimation, clients[25000]["L"], clients[25000]["M"]) == (72, 25, 28)
    second = {c["cid"]: c["sid"] for c in clients.values() if c["sid"] is not None}
    for d in calls:
        eng.process_device_group(d.data_ptr(), nbytes, G, "native", stream())
        bank.feed_engine(eng, second, stream())
        assert bank.last_feed_ops() == (2, 1)
        eng.fetch()
        bank.fetch()
        for c in clients.values():
            c["mid"].append(eng.output(c["cid"]))
            if c["sid"] is not None:
                c["out"].append(bank.output(c["sid"]))
    for fo, c in clients.items():
        mid = np.concatenate(c["mid"])
        y = mid if c["sid"] is None else np.concatenate(c["out"])
        if c["sid"] is not None:
            assert y.size == RR.counts(c["L"], c["M"], mid.size) == bank.produced(c["sid"])
            RR.check(y, c["L"], c["M"], c["taps"], mid, f"client {fo}")  # the restatement applied to the engine's own outputs
        assert y.size >= 4096
        spec = np.abs(np.fft.fft(y[-4096:].astype(np.complex128) * np.hanning(4096)))
        k = int(spec.argmax())
        assert abs(k - 3000 * 4096 / fo) <= 1.0, (fo, k, 3000 * 4096 / fo)  # 3 kHz at rate fo, +- one bin
    bank.close()
    eng.close()


# ------------------------------------------------------------------------------------------------------------ composition
def test_spectrum_bank_fed_from_the_resamplers_rows():
    _, _, L, M, taps = admission(2016000, 44100)
    W, rate = 64, 44100
    N = 2 * rate * M // L + 900  # two rows and a little at 44.1 kHz
    t = np.arange(N) / (rate * M / L)
    x = (0.4 * np.exp(2j * np.pi * 5000 * t) + noise(N, 33) * 0.01).astype(np.complex64)
    keep, addr = to_device(x)
    bank, sbank = xl.ResamplerBank(), xl.SpectrumBank(W, "cf32")
    sid, wid = bank.add(L, M, taps), sbank.add(rate)
    outs, pos = [], 0
    for c in split(N, [20000, 1, 33000, 257, 20000]):
        bank.feed([sid], [addr + 8 * pos], [c], stream())
        p, n = bank.output_device(sid)
        sbank.feed([wid], [p or 0], [n], stream())
        bank.fetch()
        outs.append(bank.output(sid))
        pos += c
    y = np.concatenate(outs)
    db, px = sbank.take_rows(wid)
    one = xl.Spectrum(rate, W, "cf32")
    one.feed(y.view(np.float32))
    want_db, want_px = one.take_rows()
    one.close()
    assert db.shape[0] == 2 and db.shape == want_db.shape
    assert np.array_equal(db.view(np.uint32), want_db.view(np.uint32)) and np.array_equal(px, want_px)
    bank.close()
    sbank.close()


# ------------------------------------------------------------------------------------------------------------ replay
def test_replay_any_rate(tmp_path):
    spec = importlib.util.spec_from_file_location("replay_iq", os.path.join(ROOT, "tools", "replay_iq.py"))
    replay_iq = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(replay_iq)
    band_rate, buffer_size, W = 192000, 65536, 64
    reqs = [(BAND_FREQ + 12000, 44100), (BAND_FREQ - 20000, 48000)]
    nsamp = 2 * band_rate + 1234
    raw = tones_u8(nsamp, band_rate, [12000 + 3000, -20000 - 1500], 8)
    path = tmp_path / "capture.cu8"
    raw.tofile(path)
    # without the flag the fractional request is rejected as before
    adm, rej, st = replay_iq.replay(str(path), "cu8", band_rate, BAND_FREQ, reqs, str(tmp_path / "plain"), buffer_size, 5, "native")
    assert sorted(adm.values()) == [reqs[1]] and rej == [(reqs[0][0], reqs[0][1], 1)]
    plain = np.fromfile(tmp_path / "plain" / f"{list(adm)[0]}.cf32", dtype=np.complex64)
    adm, rej, st = replay_iq.replay(str(path), "cu8", band_rate, BAND_FREQ, reqs, str(tmp_path / "any"), buffer_size, 5, "native",
                                    waterfall_width=W, any_rate=True)
    assert sorted(adm.values()) == sorted(reqs) and rej == [] and st["blocks_dropped"] == 0
    by_rate = {rate: cid for cid, (_, rate) in adm.items()}
    # the integer client is served as before
    assert bits_equal(np.fromfile(tmp_path / "any" / f"{by_rate[48000]}.cf32", dtype=np.complex64), plain)
    # the fractional client: the engine's own stream at D (native: the same numbers in any company), then the restatement
    req, wadm, L, M, taps = admission(band_rate, 44100, center=reqs[0][0])
    assert (wadm.decimation, L, M) == (4, 147, 160)
    eng = xl.BatchEngine(band_rate, "cu8", buffer_size)
    cid = xl.wire_add_client(eng, wadm, band_rate)
    mid = []
    for off in range(0, raw.size, buffer_size):
        eng.process_host(raw[off:off + buffer_size], "native")
        eng.fetch()
        mid.append(eng.output(cid))
    eng.close()
    mid = np.concatenate(mid)
    y = np.fromfile(tmp_path / "any" / f"{by_rate[44100]}.cf32", dtype=np.complex64)
    assert y.size == RR.counts(L, M, mid.size)
    RR.check(y, L, M, taps, mid, "replay")
    # its waterfall is the spectrogram of its .cf32 at 44.1 kHz
    import spectrogram_ref as SR

    H = y.size // 44100
    assert H >= 2
    px = SR.decode_png(str(tmp_path / "any" / f"{by_rate[44100]}.png"))
    one = xl.Spectrum(44100, W, "cf32")
    one.feed(y.view(np.float32))
    want = one.take_rows()[1]
    one.close()
    assert px.shape == (H, W) and np.array_equal(px, want[:H])
