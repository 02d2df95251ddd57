"""GPU tests (-m gpu) of the spectrum bank's widths above 8192 (xlating_spectrum_bank_create_wide, SpectrumBank(wide=True)): every
stream's rows bit for bit the single wide object's (xl.Spectrum(..., wide=True), itself held to the float64 restatement by
tests/test_spectrogram_wide_gpu.py) in company and under ragged feeds, at every transform length, with any scratch size, through
rounds, across membership changes; the float64 restatement directly; the same bank below the cap; a launch count that depends on the
transforms and the scratch, not on the streams; behind the batch engine; tools/replay_iq.py's waterfalls above 8192."""
import importlib.util
import os

import numpy as np
import pytest

import sdr_server_amd as xl
import siggen
import spectrogram_ref as R
from conftest import ROOT
from spectrogram_ref import signal

pytestmark = pytest.mark.gpu

SSZ = {"cu8": 2, "cs16": 4, "cf32": 8}


def single(raw, fmt, sr, W, wide=True):
    """the rows of one single object fed the whole signal at once"""
    s = xl.Spectrum(sr, W, fmt, wide=wide)
    s.feed(raw)
    rows = s.take_rows()
    s.close()
    return rows


def same(a, b):
    return a[0].shape == b[0].shape and np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1], b[1])


def cat(parts, W):
    db = np.concatenate([p[0] for p in parts]) if parts else np.zeros((0, W), np.float32)
    px = np.concatenate([p[1] for p in parts]) if parts else np.zeros((0, W), np.uint8)
    return db, px


def run_bank(W, fmt, streams, wide=True, take_between=True, ops=None):
    """streams: [(sampling_rate, raw, counts)]: feed f gives stream i its counts[f] next samples (0 once its list has ended; what the
    counts leave over goes in a last feed), all streams in one call from device memory; rows are taken between feeds from every other
    stream and at the end from all.  ops: a list that gets every feed's last_feed_ops().  -> [(db, px)] per stream"""
    import torch

    st = torch.cuda.current_stream().cuda_stream
    bank = xl.SpectrumBank(W, fmt, wide=wide)
    S = []
    for k, (sr, raw, counts) in enumerate(streams):
        n = raw.size // 2
        counts = [int(c) for c in counts]
        assert sum(counts) <= n
        if sum(counts) < n:
            counts.append(n - sum(counts))
        S.append(dict(id=bank.add(sr), dev=torch.from_numpy(raw).cuda(), counts=counts, pos=0, parts=[], early=take_between and k % 2 == 0))
    for f in range(max(len(s["counts"]) for s in S)):
        ids, ptrs, cnts = [], [], []
        for s in S:
            c = s["counts"][f] if f < len(s["counts"]) else 0
            ids.append(s["id"])
            ptrs.append(s["dev"].data_ptr() + s["pos"] * SSZ[fmt])
            cnts.append(c)
            s["pos"] += c
        bank.feed(ids, ptrs, cnts, st)
        if ops is not None:
            ops.append(bank.last_feed_ops())
        for s in S:
            if s["early"] and f % 3 == 0:
                s["parts"].append(bank.take_rows(s["id"]))
    out = []
    for s in S:
        s["parts"].append(bank.take_rows(s["id"]))
        assert bank.rows_pending(s["id"]) == 0
        out.append(cat(s["parts"], W))
    bank.close()
    return out


# ------------------------------------------------------------------------------------------------------------ 1. in company
@pytest.mark.parametrize("fmt", ["cu8", "cs16", "cf32"])
@pytest.mark.parametrize("W", [16384, 8193, 20000])
def test_rows_equal_the_single_wide_object_in_company(W, fmt):
    """three streams of one bank -- F = 1; F = 2 with a skip; F = 3 with a skip -- about 2.3 rows each, fed in ragged pieces that differ
    per stream: pieces of 1000 samples (the carry is appended to many times), seeded random pieces below W // 2, one piece spanning two
    rows.  Not within a tolerance: equal"""
    rng = np.random.default_rng(31 * W + SSZ[fmt])
    rates = [W, 2 * W + W // 3, 3 * W + W // 2 + 1]
    n = [2 * sr + sr * 3 // 10 for sr in rates]
    raws = [signal(fmt, n[k], W, seed=(977 * W + k) % (1 << 32)) for k in range(3)]
    pieces = [[1000] * (n[0] // 1000),
              [int(v) for v in rng.integers(1, W // 2, 2 * n[1] // (W // 2))],
              [777, 2 * rates[2] + 5]]
    pieces[1] = pieces[1][:int(np.searchsorted(np.cumsum(pieces[1]), n[1]))]
    got = run_bank(W, fmt, list(zip(rates, raws, pieces)))
    for sr, raw, rows in zip(rates, raws, got):
        want = single(raw, fmt, sr, W)
        assert want[0].shape == (2, W)
        assert same(rows, want), (W, fmt, sr)


# ------------------------------------------------------------------------------------------------------------ 2. every length
LENGTHS = [1 << e for e in range(14, 21)] + [8193, 16385, 50000, 100000, 200000, 262145, 1048575]


@pytest.mark.parametrize("W", LENGTHS)
def test_every_transform_length(W):
    """plain 2^14 .. 2^20 and Bluestein 2^15 .. 2^21 (all three splits N1 = 64, 128, 256), cf32, two streams of different rates.  The two
    largest lengths (N = 2^20 and 2^21: the widths 262145, 1048576 and 1048575) run with F = 1 and one row per stream"""
    fmt = "cf32"
    N = W if W & (W - 1) == 0 else 1 << (2 * W - 2).bit_length()  # (the power of two >= 2 W - 1)
    if N >= 1 << 20:
        rates, n = [W, W + 3], [W + 1000, W + 1500]
    else:
        rates, n = [W, 2 * W + 3], [2 * W + 100, 2 * W + 3 + 500]
    raws = [signal(fmt, n[k], W, seed=(13 * W + k) % (1 << 32)) for k in range(2)]
    got = run_bank(W, fmt, [(rates[0], raws[0], [W // 2 + 1]), (rates[1], raws[1], [n[1] - 7])])
    for sr, raw, rows in zip(rates, raws, got):
        want = single(raw, fmt, sr, W)
        assert want[0].shape[0] in (1, 2)
        assert same(rows, want), (W, sr)


# ------------------------------------------------------------------------------------------------------------ 3. the restatement
@pytest.mark.parametrize("fmt,W", [("cu8", 16384), ("cf32", 50000)])
def test_rows_against_float64(fmt, W):
    """directly against tests/spectrogram_ref.py, its criteria unchanged, with the signals of test_spectrogram_wide_gpu.py's parity
    cases (which meet the criteria's condition on the inputs for the single object): so that equality with the single object cannot
    pass by both being wrong together"""
    sr = W
    raw = signal(fmt, sr * 2 + sr // 3, W, seed=(1000 * W + 0) % (1 << 32))
    other = signal(fmt, 3 * W + 10, W, seed=4)
    (db, px), _ = run_bank(W, fmt, [(sr, raw, [W // 3, W]), (W + 7, other, [W + W // 2])])
    assert db.shape == (2, W)
    total, equal = R.check_parity(db, px, raw, fmt, sr, W)
    print(f"wide bank parity {fmt} W={W}: {total - equal} of {total} pixels differ")


# ------------------------------------------------------------------------------------------------------------ 4. scratch chunking
@pytest.mark.parametrize("W,N", [(16384, 16384), (8193, 32768)])
def test_scratch_chunking(W, N, monkeypatch):
    """three streams with F = 7, each fed a row at a time: 21 transforms per round.  A scratch that holds 5, 3 and 1 transforms (chunk
    ends inside a run, and exactly between two streams' runs) gives the rows of the default scratch, which are the single object's"""
    fmt, sr = "cf32", 7 * W
    raws = [signal(fmt, 2 * sr, W, seed=40 + k) for k in range(3)]
    streams = [(sr, raw, [sr, sr]) for raw in raws]
    whole = run_bank(W, fmt, streams)
    for raw, rows in zip(raws, whole):
        assert rows[0].shape == (2, W)
    assert same(whole[1], single(raws[1], fmt, sr, W))
    monkeypatch.setenv("XL_TESTING", "1")
    for held in (5, 3, 1):
        monkeypatch.setenv("XL_EXP_SPEC_SCRATCH", str(held * 8 * N))
        got = run_bank(W, fmt, streams)
        for k in range(3):
            assert same(got[k], whole[k]), (held, k)


# ------------------------------------------------------------------------------------------------------------ 5. rounds
def test_rounds_give_the_same_rows(monkeypatch):
    """one feed takes a stream through five rows with two row slots, beside a slower stream, with a staging that holds one row (every
    completed row ends a round): the rows of five one-row feeds.  That the staging did cut the feed shows in its copies: each of the
    seven rows then has a round of its own, which is a table and a pair of row copies"""
    W, fmt = 16384, "cu8"
    rates = [W + 5, 2 * W + 100]
    n = [5 * rates[0] + 100, 2 * rates[1] + W]
    raws = [signal(fmt, n[k], W, seed=70 + k) for k in range(2)]
    by_rows = run_bank(W, fmt, [(rates[0], raws[0], [rates[0]] * 5), (rates[1], raws[1], [rates[1] // 2] * 4)])
    assert by_rows[0][0].shape == (5, W) and by_rows[1][0].shape == (2, W)
    ops_default, ops_tiny = [], []
    at_once = run_bank(W, fmt, [(rates[0], raws[0], [n[0]]), (rates[1], raws[1], [n[1]])], take_between=False, ops=ops_default)
    assert same(at_once[0], by_rows[0]) and same(at_once[1], by_rows[1])
    monkeypatch.setenv("XL_TESTING", "1")
    monkeypatch.setenv("XL_EXP_SPEC_BANK_STAGE", "1")
    tiny = run_bank(W, fmt, [(rates[0], raws[0], [n[0]]), (rates[1], raws[1], [n[1]])], take_between=False, ops=ops_tiny)
    assert same(tiny[0], by_rows[0]) and same(tiny[1], by_rows[1])
    print("five rows and two in one feed, (launches, copies): default staging", ops_default, "one-row staging", ops_tiny)
    assert len(ops_default) == len(ops_tiny) == 1
    assert ops_tiny[0][1] >= 3 * 7 and ops_tiny[0][1] > ops_default[0][1] and ops_tiny[0][0] > ops_default[0][0], (ops_default, ops_tiny)
    assert same(tiny[0], single(raws[0], fmt, rates[0], W))


# ------------------------------------------------------------------------------------------------------------ 6. membership
def test_membership():
    """add, feed half a row, remove, add again (the id is reused), feed: the new stream's rows are a fresh single object's -- nothing of
    the removed stream's half row is in them -- and a stream fed throughout is undisturbed"""
    import torch

    W, fmt = 8193, "cs16"
    st = torch.cuda.current_stream().cuda_stream
    rate = {"a": 2 * W + 11, "b": 2 * W + 100, "d": W + 3}
    sigs = {"a": signal(fmt, 2 * rate["a"] + 500, W, 1), "b": signal(fmt, rate["b"], W, 2), "d": signal(fmt, 2 * rate["d"] + 9, W, 3)}
    dev = {k: torch.from_numpy(v).cuda() for k, v in sigs.items()}
    pos = dict.fromkeys(sigs, 0)
    ids = {}
    bank = xl.SpectrumBank(W, fmt, wide=True)

    def feed(pairs):
        bank.feed([ids[n] for n, _ in pairs], [dev[n].data_ptr() + 4 * pos[n] for n, _ in pairs], [c for _, c in pairs], st)
        for n, c in pairs:
            pos[n] += c

    ids["a"] = bank.add(rate["a"])
    ids["b"] = bank.add(rate["b"])
    feed([("a", 3000), ("b", W // 2)])  # b: a carry is left behind
    feed([("b", rate["b"] // 2 - W // 2), ("a", W)])  # b: half a row; its first transform is in, so its row slot holds maxima
    assert W < pos["b"] < 2 * W and bank.rows_pending(ids["b"]) == 0
    bank.remove(ids["b"])
    ids["d"] = bank.add(rate["d"])
    assert ids["d"] == ids["b"]
    assert bank.rows_pending(ids["d"]) == 0
    feed([("d", rate["d"] + 17), ("a", rate["a"])])
    feed([("d", sigs["d"].size // 2 - pos["d"])])
    feed([("a", sigs["a"].size // 2 - pos["a"])])
    for n in ("a", "d"):
        want = single(sigs[n], fmt, rate[n], W)
        assert want[0].shape[0] == 2
        assert same(bank.take_rows(ids[n]), want), n
    bank.close()


# ------------------------------------------------------------------------------------------------------------ 7. below the cap
@pytest.mark.parametrize("W", [100, 8191, 8192])
def test_same_bank_below_the_cap(W):
    fmt = "cs16"
    rates = [W, 2 * W + 3]
    raws = [signal(fmt, 3 * sr + 11, W, seed=W + k) for k, sr in enumerate(rates)]
    streams = [(rates[0], raws[0], [W // 2, W + 1]), (rates[1], raws[1], [1, 2 * rates[1]])]
    wide, narrow = run_bank(W, fmt, streams, wide=True), run_bank(W, fmt, streams, wide=False)
    for k in range(2):
        assert narrow[k][0].shape[0] == 3
        assert same(wide[k], narrow[k]), (W, k)
    assert same(wide[0], single(raws[0], fmt, rates[0], W, wide=False))


# ------------------------------------------------------------------------------------------------------------ 8. launch count
def test_launch_count_depends_on_transforms_and_scratch_not_on_streams(monkeypatch):
    """8 transforms as one stream x 8 and as 8 streams x 1, at the same width and scratch, report the same last_feed_ops(); a scratch
    twice as large does not increase it"""
    import torch

    W, fmt = 16384, "cf32"
    raw = signal(fmt, 8 * W, W, 5)
    d = torch.from_numpy(raw).cuda()
    st = torch.cuda.current_stream().cuda_stream
    monkeypatch.setenv("XL_TESTING", "1")
    ops = {}
    for held in (4, 8):
        monkeypatch.setenv("XL_EXP_SPEC_SCRATCH", str(held * 8 * W))
        for n in (1, 8):
            bank = xl.SpectrumBank(W, fmt, wide=True)
            ids = [bank.add(8 * W // n) for _ in range(n)]
            bank.feed(ids, [d.data_ptr() + 8 * i * (8 * W // n) for i in range(n)], [8 * W // n] * n, st)
            ops[(held, n)] = bank.last_feed_ops()
            assert all(bank.rows_pending(i) == 1 for i in ids)
            if n == 1:
                assert same(bank.take_rows(ids[0]), single(raw, fmt, 8 * W, W))
            bank.close()
        print(f"scratch of {held} transforms: (launches, copies) one stream x 8 {ops[(held, 1)]}, 8 streams x 1 {ops[(held, 8)]}")
        assert ops[(held, 1)] == ops[(held, 8)], ops
    assert ops[(8, 1)][0] <= ops[(4, 1)][0] and ops[(8, 1)][1] <= ops[(4, 1)][1], ops
    assert ops[(4, 1)][0] == 2 * 2 + 1 and ops[(8, 1)][0] == 2 + 1, ops  # two passes per chunk of a plain width, one finishing launch


# ------------------------------------------------------------------------------------------------------------ 9. behind the engine
def test_device_feed_behind_the_engine():
    """2.016 Msps cu8, eight 48 kHz clients at D = 42 (101 taps), two optimized calls of 8 blocks, feed_engine after each into a wide bank
    of W = 16000 (F = 3): every client's completed row is the single wide object's from that client's fetched outputs"""
    import torch

    band, W, nbytes, G = 2016000, 16000, 262144, 8
    taps = siggen.hamming_sinc(101, 0.01)
    eng = xl.BatchEngine(band, "cu8", nbytes, group_blocks=G)
    ids = [eng.add_client(42, taps, -700000 + 200000 * c) for c in range(8)]
    bank = xl.SpectrumBank(W, "cf32", wide=True)
    sid = {cid: bank.add(48000) for cid in ids}
    st = torch.cuda.current_stream()
    ev = torch.cuda.Event()
    ev.record(st)  # (creates the event)
    outs = {cid: [] for cid in ids}
    for call in range(2):
        x = siggen.xs_u8(777 + call, G * nbytes)
        d = torch.from_numpy(x).cuda()
        torch.cuda.synchronize()  # (the engine's stream is not torch's)
        eng.process_device_group(d.data_ptr(), nbytes, G, "optimized", "engine")
        eng.record_event(ev.cuda_event)
        st.wait_event(ev)
        bank.feed_engine(eng, sid, st.cuda_stream)
        print("wide bank behind the engine, feed (launches, copies):", bank.last_feed_ops())
        st.synchronize()  # (the next call reuses the device rows)
        eng.fetch()
        for cid in ids:
            outs[cid].append(eng.output(cid))
    for cid in ids:
        raw = np.concatenate(outs[cid]).view(np.float32)
        assert 48000 <= raw.size // 2 < 2 * 48000
        rows = bank.take_rows(sid[cid])
        assert rows[0].shape == (1, W)
        assert same(rows, single(raw, "cf32", 48000, W)), cid
    bank.close()
    eng.close()


# ------------------------------------------------------------------------------------------------------------ 10. replay
def test_replay_writes_wide_waterfalls(tmp_path):
    """tools/replay_iq.py --waterfall-width 9000 on a short generated capture with two 48 kHz clients: each <id>.png has the pixels
    spectrogram_main(..., wide=True) makes from that client's .cf32"""
    spec = importlib.util.spec_from_file_location("replay_iq", os.path.join(ROOT, "tools", "replay_iq.py"))
    replay_iq = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(replay_iq)
    band_rate, band_freq, W = 192000, 460100000, 9000
    rng = np.random.default_rng(8)
    n = int(2.3 * band_rate)
    t = np.arange(n) / band_rate
    z = 0.4 * np.exp(2j * np.pi * 15000 * t) + 0.3 * np.exp(-2j * np.pi * 41500 * t) + 0.01 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    raw = np.clip(np.round(127.5 + 127 * np.stack([z.real, z.imag], axis=1).reshape(-1)), 0, 255).astype(np.uint8)
    path, out = tmp_path / "capture.cu8", tmp_path / "out"
    raw.tofile(path)
    assert raw.size < 1 << 20
    replay_iq.main([str(path), "--format", "cu8", "--band-rate", str(band_rate), "--band-freq", str(band_freq), "--out", str(out),
                    "--client", "460112000:48000", "--client", "460060000:48000", "--variant", "native", "--waterfall-width", str(W)])
    pngs = sorted(f for f in os.listdir(out) if f.endswith(".png"))
    assert len(pngs) == 2
    for f in pngs:
        cf32 = str(out / f.replace(".png", ".cf32"))
        H = (os.path.getsize(cf32) // 8) // 48000
        assert H == 2
        want = str(tmp_path / ("want_" + f))
        assert xl.spectrogram_main(cf32, want, W, 48000, "cf32", wide=True) == 0
        got_px, want_px = R.decode_png(str(out / f)), R.decode_png(want)
        assert got_px.shape == (H, W) and np.array_equal(got_px, want_px), f
