"""GPU tests (-m gpu) of the spectrum bank (include/xlating_spectrum.h, xlating_spectrum_bank_*): every stream's rows bit-identical
to the single-stream object's over widths, formats, row shapes and ragged feeds; parity with the float64 restatement
(tests/spectrogram_ref.py); membership changes; a launch count that does not depend on the number of streams; behind the batch engine
(mixed clients, the headline population, no interference); tools/replay_iq.py's waterfalls."""
import errno
import importlib.util
import os

import numpy as np
import pytest

import sdr_server_amd as xl
import siggen
import spectrogram_ref as R
from conftest import ROOT
from spectrogram_ref import check_parity, signal

pytestmark = pytest.mark.gpu

SSZ = {"cu8": 2, "cs16": 4, "cf32": 8}


def single(raw, fmt, sr, W):
    """the rows of one xl.Spectrum fed the whole signal at once"""
    s = xl.Spectrum(sr, W, fmt)
    s.feed(raw)
    db, px = s.take_rows()
    s.close()
    return db, px


def assert_same_rows(got, want, what):
    assert got[0].shape == want[0].shape and got[1].shape == want[1].shape, (what, got[0].shape, want[0].shape)
    assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)), what
    assert np.array_equal(got[1], want[1]), what


def cat(parts, W):
    db = np.concatenate([p[0] for p in parts]) if parts else np.zeros((0, W), np.float32)
    px = np.concatenate([p[1] for p in parts]) if parts else np.zeros((0, W), np.uint8)
    return db, px


# ------------------------------------------------------------------------------------------------------------ (1), (2) plain buffers
def rates_of(W):
    """F = 1 without skip (a rate equal to W), F = 3 with a skip of W // 2 + 1 where that stays below W, a multiple of W, F = 2 with a
    skip of one sample, and for W <= 1024 an F in the hundreds with a skip"""
    skip = W // 2 + 1 if W // 2 + 1 < W else 0
    rates = [W, 3 * W + skip, 5 * W, 2 * W + (1 if W > 1 else 0), 7 * W + W // 3]
    if W <= 1024:
        rates.append(150 * W + W // 3)
    return rates


def feed_counts(rng, sr, W, nfeeds):
    """nfeeds counts of one stream: 0, 1, W - 1, W + 1 and one spanning more than a row among them, the others random; their sum is
    the stream's length: at least three rows and a third"""
    special = [0, 1, W - 1, W + 1, sr + sr // 2 + 1]
    total = max(3 * sr + sr // 3, sum(special) + 2 * sr)
    rest = total - sum(special)
    cuts = np.sort(rng.integers(0, rest + 1, nfeeds - len(special) - 1))
    parts = np.diff(np.concatenate([[0], cuts, [rest]]))
    counts = np.concatenate([special, parts]).astype(np.int64)
    rng.shuffle(counts)
    assert counts.size == nfeeds and counts.sum() == total
    return counts, total


_BANK_RUNS = {}


def run_bank_case(W, fmt):
    """(1)'s run, once per (W, fmt): -> [(sr, raw, db, px)] per stream"""
    import torch

    if (W, fmt) in _BANK_RUNS:
        return _BANK_RUNS[(W, fmt)]
    rng = np.random.default_rng(10007 * W + SSZ[fmt])
    nfeeds = 24
    st = torch.cuda.current_stream()
    bank = xl.SpectrumBank(W, fmt)
    streams = []
    for k, sr in enumerate(rates_of(W)):
        counts, total = feed_counts(rng, sr, W, nfeeds)
        raw = signal(fmt, total, W, seed=977 * W + k)
        streams.append(dict(sr=sr, raw=raw, dev=torch.from_numpy(raw).cuda(), counts=counts, pos=0, id=bank.add(sr), parts=[],
                            early=(k % 2 == 0)))
    for f in range(nfeeds):
        ids, ptrs, cnts = [], [], []
        for s in streams:
            ids.append(s["id"])
            ptrs.append(s["dev"].data_ptr() + s["pos"] * SSZ[fmt])
            cnts.append(int(s["counts"][f]))
            s["pos"] += int(s["counts"][f])
        bank.feed(ids, ptrs, cnts, st.cuda_stream)
        for s in streams:
            if s["early"] and (f % 3 == 0):  # rows taken between feeds for some streams, only at the end for the others
                s["parts"].append(bank.take_rows(s["id"]))
    out = []
    for s in streams:
        assert s["pos"] * 2 == s["raw"].size
        s["parts"].append(bank.take_rows(s["id"]))
        assert bank.rows_pending(s["id"]) == 0
        out.append((s["sr"], s["raw"], *cat(s["parts"], W)))
    bank.close()
    _BANK_RUNS.clear()  # (one case is kept: (2) follows (1) of the same width and format)
    _BANK_RUNS[(W, fmt)] = out
    return out


WIDTHS = [1, 3, 64, 100, 256, 1000, 1024, 8191, 8192]


@pytest.mark.parametrize("fmt", ["cu8", "cs16", "cf32"])
@pytest.mark.parametrize("W", WIDTHS)
def test_bank_rows_equal_single_object(W, fmt):
    """(1): not within a tolerance -- equal: both run the same transform code on the same samples, and a maximum is exact"""
    for sr, raw, db, px in run_bank_case(W, fmt):
        want = single(raw, fmt, sr, W)
        assert want[0].shape[0] >= 3
        assert_same_rows((db, px), want, (W, fmt, sr))


@pytest.mark.parametrize("W,fmt", [(100, "cu8"), (256, "cs16"), (8191, "cf32"), (256, "cf32"), (1000, "cu8"), (64, "cs16")])
def test_bank_rows_against_float64(W, fmt):
    """(2): the same streams against the float64 restatement, so that (1) cannot pass by both sides being wrong together"""
    for sr, raw, db, px in run_bank_case(W, fmt):
        H = (raw.size // 2) // sr  # (the restatement's height; a stream also completes a last row whose skipped tail is missing)
        assert db.shape[0] in (H, H + 1)
        check_parity(db[:H], px[:H], raw, fmt, sr, W)


def test_rounds_give_the_same_rows(monkeypatch):
    """one row slot per stream: every feed that crosses a row is cut into rounds; the rows do not change"""
    monkeypatch.setenv("XL_EXP_SPEC_BANK_SLOTS", "1")
    _BANK_RUNS.clear()
    for sr, raw, db, px in run_bank_case(64, "cf32"):
        assert_same_rows((db, px), single(raw, "cf32", sr, 64), sr)
    _BANK_RUNS.clear()


def test_six_feeds_in_a_row_reuse_the_pinned_tables():
    """the ring holds four pinned tables: the fifth and the sixth feed write tables that earlier feeds were uploaded from, and nothing
    on the host waits in between (the per-stream arrays growing under rows in progress and the device table growing between feeds:
    test_membership)"""
    import torch

    W, sr, fmt = 64, 64 * 3 + 33, "cf32"
    counts = [300, 200, 257, 150, 333, 150]  # every feed completes a row and leaves a straddling transform
    raw = signal(fmt, sum(counts), W, seed=61)
    d = torch.from_numpy(raw).cuda()
    st = torch.cuda.current_stream().cuda_stream
    bank = xl.SpectrumBank(W, fmt)
    sid = bank.add(sr)
    pos = 0
    for c in counts:
        assert pos // sr < (pos + c) // sr and (pos + c) % sr % W != 0
        bank.feed([sid], [d.data_ptr() + 8 * pos], [c], st)
        pos += c
    rows = bank.take_rows(sid)
    assert rows[0].shape[0] == pos // sr == 6
    assert_same_rows(rows, single(raw, fmt, sr, W), "six feeds")
    bank.close()


# ------------------------------------------------------------------------------------------------------------ (3) membership
def test_membership():
    import torch

    W, fmt = 100, "cs16"
    st = torch.cuda.current_stream().cuda_stream
    bank = xl.SpectrumBank(W, fmt)
    sigs = {name: signal(fmt, n, W, seed) for name, n, seed in [("a", 5000, 1), ("b", 5000, 2), ("c", 4000, 3), ("d", 3000, 4)]}
    dev = {k: torch.from_numpy(v).cuda() for k, v in sigs.items()}
    rate = {"a": 730, "b": 415, "c": 100, "d": 250}
    pos = dict.fromkeys(sigs, 0)
    ids = {}

    def feed(pairs):
        """pairs: [(name, count)]"""
        bank.feed([ids[n] for n, _ in pairs], [dev[n].data_ptr() + 4 * pos[n] for n, _ in pairs], [c for _, c in pairs], st)
        for n, c in pairs:
            pos[n] += c

    ids["a"] = bank.add(rate["a"])
    ids["b"] = bank.add(rate["b"])
    feed([("a", 1234), ("b", 777)])
    ids["c"] = bank.add(rate["c"])  # added after others have consumed samples
    feed([("c", 150), ("a", 901)])  # a subset
    assert bank.rows_pending(ids["b"]) == 777 // 415 + (1 if 777 % 415 >= 400 else 0)
    # b is removed mid-row, its id reused at another rate
    old_b = ids["b"]
    bank.remove(old_b)
    with pytest.raises(xl.XlatingError) as e:
        bank.take_rows(old_b)
    assert e.value.code == -errno.EINVAL
    with pytest.raises(xl.XlatingError) as e:  # a removed id is refused, and nothing is consumed
        bank.feed([ids["a"], old_b], [dev["a"].data_ptr(), dev["b"].data_ptr()], [10, 10], st)
    assert e.value.code == -errno.EINVAL
    with pytest.raises(xl.XlatingError) as e:
        bank.remove(old_b)
    assert e.value.code == -errno.EINVAL
    ids["d"] = bank.add(rate["d"])
    assert ids["d"] == old_b
    with pytest.raises(xl.XlatingError) as e:  # a duplicate id: -EINVAL, nothing consumed
        bank.feed([ids["a"], ids["d"], ids["a"]], [dev["a"].data_ptr()] * 3, [50, 50, 50], st)
    assert e.value.code == -errno.EINVAL
    with pytest.raises(xl.XlatingError) as e:
        bank.add(W - 1)
    assert e.value.code == -errno.EINVAL
    feed([("d", 1111), ("a", 5000 - pos["a"]), ("c", 4000 - pos["c"])])
    feed([("d", 3000 - pos["d"])])
    for n in ("a", "c", "d"):
        assert pos[n] * 2 == sigs[n].size
        assert_same_rows(bank.take_rows(ids[n]), single(sigs[n], fmt, rate[n], W), n)
    # many streams: the per-stream state grows past its first allocation while streams hold rows in progress
    more = [bank.add(333) for _ in range(200)]
    assert len(set(more) | set(ids.values())) == 200 + 3
    feed2 = signal(fmt, 1000, W, 9)
    d2 = torch.from_numpy(feed2).cuda()
    bank.feed(more, [d2.data_ptr()] * 200, [500] * 200, st)
    more2 = [bank.add(333) for _ in range(300)]  # (grows again, mid-row)
    bank.feed(more + more2, [d2.data_ptr() + 4 * 500] * 200 + [d2.data_ptr()] * 300, [500] * 200 + [1000] * 300, st)
    want = single(feed2, fmt, 333, W)
    for sid in (more[0], more[77], more[199], more2[0], more2[299]):
        assert_same_rows(bank.take_rows(sid), want, sid)
    bank.close()


# ------------------------------------------------------------------------------------------------------------ (4) launch count
def test_launch_count_does_not_depend_on_the_number_of_streams():
    import torch

    W, sr, fmt = 64, 64 * 4 + 9, "cf32"
    raw = signal(fmt, 4 * sr, W, 5)
    d = torch.from_numpy(raw).cuda()
    st = torch.cuda.current_stream().cuda_stream
    ops = {}
    for n in (8, 1024):
        bank = xl.SpectrumBank(W, fmt)
        ids = [bank.add(sr) for _ in range(n)]
        bank.feed(ids, [d.data_ptr()] * n, [W + 3] * n, st)  # completes no row, leaves a carry
        quiet = bank.last_feed_ops()
        bank.feed(ids, [d.data_ptr() + 8 * (W + 3)] * n, [2 * sr] * n, st)  # completes rows, continues and leaves a carry
        busy = bank.last_feed_ops()
        assert all(bank.rows_pending(i) == 2 for i in ids)
        rows = bank.take_rows(ids[-1])
        assert_same_rows(rows, tuple(a[:2] for a in single(raw[:2 * (W + 3 + 2 * sr)], fmt, sr, W)), n)
        bank.close()
        ops[n] = (quiet, busy)
        print(f"streams {n}: (launches, copies) without rows {quiet}, with rows {busy}")
    assert ops[8] == ops[1024], ops
    (ql, qc), (bl, bc) = ops[8]
    assert ql >= 1 and qc >= 1 and bl > ql and bc == qc + 2  # the finishing launch and its pair of copies


# ------------------------------------------------------------------------------------------------------------ (5) behind the engine
def tones_u8(n, band_rate, freqs, seed):
    """a cu8 band of n samples: one tone per frequency (Hz from the band's centre), equal amplitudes, a little noise"""
    rng = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64) / band_rate
    z = np.zeros(n, np.complex128)
    for f0 in range(0, len(freqs), 16):  # (in slabs: bounded memory)
        z += np.exp(2j * np.pi * np.asarray(freqs[f0:f0 + 16])[:, None] * t[None, :]).sum(axis=0)
    z *= 0.8 / len(freqs)
    z += 0.002 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    v = np.stack([z.real, z.imag], axis=1).reshape(-1)
    return np.clip(np.round(127.5 + 127 * v), 0, 255).astype(np.uint8)


@pytest.mark.parametrize("variant", ["optimized", "native"])
def test_behind_the_batch_engine_mixed_clients(variant):
    import torch

    band, W, nbytes, ncalls = 2016000, 64, 100002, 4
    code, taps = xl.create_low_pass_filter(1.0, band, 4000, 9600)
    assert code == 0
    clients = []  # (D, centre, k)
    for c in range(80):
        D = 42 if c % 2 == 0 else 21
        k = (c // 2) % 7 - 3 if D == 42 else (c // 2) % 5 - 2
        clients.append((D, -880000 + 22000 * c, k))
    freqs = [fc + k * (band / D) / W for D, fc, k in clients]
    x = tones_u8(ncalls * nbytes // 2, band, freqs, 3)
    blocks = [torch.from_numpy(b).cuda() for b in np.split(x, ncalls)]
    st = torch.cuda.current_stream()
    eng = xl.BatchEngine(band, "cu8", nbytes)
    ids = [eng.add_client(D, taps, fc) for D, fc, _ in clients]
    bank = xl.SpectrumBank(W, "cf32")
    sr = {42: 64 * 17 + 5, 21: 64 * 35 + 21}  # (shorter than the true rates: rows complete within a call or two)
    sid = {cid: bank.add(sr[D]) for cid, (D, _, _) in zip(ids, clients)}
    outs = {cid: [] for cid in ids}
    for d in blocks:
        eng.process_device(d.data_ptr(), nbytes, variant, st.cuda_stream)
        bank.feed_engine(eng, sid, st.cuda_stream)
        eng.fetch()
        for cid in ids:
            outs[cid].append(eng.output(cid))
            assert outs[cid][-1].size % W != 0
    if variant == "optimized":
        desc = eng.describe()
        poly = desc.split("| polyphase:")[1].split("|")[0]
        assert " D42 " in poly and " D21 " in poly and "cols40" in poly, desc
    for cid, (D, _, k) in zip(ids, clients):
        raw = np.concatenate(outs[cid]).view(np.float32)
        db, px = bank.take_rows(sid[cid])
        assert db.shape[0] >= 3
        assert_same_rows((db, px), single(raw, "cf32", sr[D], W), cid)  # (a)
        H = (raw.size // 2) // sr[D]
        check_parity(db[:H], px[:H], raw, "cf32", sr[D], W)  # (b)
        assert np.all(db.argmax(axis=1) == W // 2 + k), (cid, D, k, db.argmax(axis=1))  # (c)
    bank.close()
    eng.close()


# ------------------------------------------------------------------------------------------------------------ (6) headline
def test_headline_population():
    """1024 clients x 48 kHz (D = 42, 505 taps), two calls of 8 blocks on the engine's own stream, ordered by record_event: one row of
    F = 187 at W = 256 per client"""
    import torch

    band, W, nbytes, G = 2016000, 256, 262144, 8
    code, taps = xl.create_low_pass_filter(1.0, band, 24000, 9600)
    assert code == 0 and taps.size == 505
    eng = xl.BatchEngine(band, "cu8", nbytes, group_blocks=G)
    ids = [eng.add_client(42, taps, -900000 + 1758 * c) for c in range(1024)]
    bank = xl.SpectrumBank(W, "cf32")
    sid = {cid: bank.add(48000) for cid in ids}
    st = torch.cuda.current_stream()
    ev = torch.cuda.Event()
    ev.record(st)  # (creates the event)
    outs = {cid: [] for cid in ids}
    for call in range(2):
        x = siggen.xs_u8(4242 + call, G * nbytes)
        d = torch.from_numpy(x).cuda()
        torch.cuda.synchronize()  # (the engine's stream is not torch's)
        eng.process_device_group(d.data_ptr(), nbytes, G, "optimized", "engine")
        eng.record_event(ev.cuda_event)
        st.wait_event(ev)
        bank.feed_engine(eng, sid, st.cuda_stream)
        print("headline feed (launches, copies):", bank.last_feed_ops())
        st.synchronize()  # (the next call reuses the device rows)
        eng.fetch()
        for cid in ids:
            outs[cid].append(eng.output(cid))
    assert "polyphase: cls0 D42 T505 cols1024" in eng.describe(), eng.describe()
    sample = set(ids[::32])
    assert len(sample) == 32
    for cid in ids:
        raw = np.concatenate(outs[cid]).view(np.float32)
        assert 47872 <= raw.size // 2 < 2 * 48000
        db, px = bank.take_rows(sid[cid])
        assert db.shape[0] == 1
        H = (raw.size // 2) // 48000
        assert H == 1
        check_parity(db, px, raw, "cf32", 48000, W)
        if cid in sample:
            assert_same_rows((db, px), single(raw, "cf32", 48000, W), cid)
    bank.close()
    eng.close()


# ------------------------------------------------------------------------------------------------------------ (7) interference
def test_bank_beside_the_batch_engine():
    """config 5's engine (cf32, D = 100, 257 taps, 64 clients: the two-half matrix-core mix) with and without a bank fed from its
    outputs on the same stream: the engine's outputs do not change, and the bank's rows are those of a bank fed the same recorded
    outputs with no engine alive"""
    import torch

    taps = siggen.hamming_sinc(257, 0.004)
    nsamp, W, sr = 131072, 64, 64 * 9 + 7
    fcs = [-4900000 + (9800000 // 64) * c for c in range(64)]
    blocks = [signal("cf32", nsamp, 64, seed=50 + k) for k in range(3)]
    dev = [torch.from_numpy(b).cuda() for b in blocks]
    st = torch.cuda.current_stream()

    def run(with_bank):
        eng = xl.BatchEngine(10000000, "cf32", 2 * nsamp)
        ids = [eng.add_client(100, taps, fc) for fc in fcs]
        bank = sid = None
        if with_bank:
            bank = xl.SpectrumBank(W, "cf32")
            sid = {cid: bank.add(sr) for cid in ids}
        outs = []
        for d in dev:
            eng.process_device(d.data_ptr(), 2 * nsamp, "optimized", st.cuda_stream)
            if bank:
                bank.feed_engine(eng, sid, st.cuda_stream)
            eng.fetch()
            outs.append([eng.output(c).copy() for c in ids])
        assert "mix=mfma" in eng.describe(), eng.describe()
        rows = [bank.take_rows(sid[c]) for c in ids] if bank else None
        eng.close()
        if bank:
            bank.close()
        return outs, rows

    outs_alone, _ = run(False)
    outs_both, rows_both = run(True)
    for a, b in zip(outs_alone, outs_both):
        for x, y in zip(a, b):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    # the same recorded outputs into a bank with no engine alive
    bank = xl.SpectrumBank(W, "cf32")
    sids = [bank.add(sr) for _ in fcs]
    for call in outs_both:
        d = [torch.from_numpy(o.view(np.float32)).cuda() for o in call]
        bank.feed(sids, [t.data_ptr() for t in d], [o.size for o in call], st.cuda_stream)
        st.synchronize()
    for c, s in enumerate(sids):
        rows = bank.take_rows(s)
        assert rows[0].shape[0] >= 3
        assert_same_rows(rows_both[c], rows, c)
    bank.close()


# ------------------------------------------------------------------------------------------------------------ (8) replay
def test_replay_writes_each_clients_waterfall(tmp_path):
    spec = importlib.util.spec_from_file_location("replay_iq", os.path.join(ROOT, "tools", "replay_iq.py"))
    replay_iq = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(replay_iq)
    band_rate, band_freq, buffer_size, W = 192000, 460100000, 262144, 256
    reqs = [(460112000, 48000), (460080000, 24000), (460140000, 32000), (460100000 + 2000000, 48000)]
    nsamp = int(3.3 * band_rate)  # at least three rows (seconds) of every client
    raw = tones_u8(nsamp, band_rate, [12000 + 3000, -20000 - 1500, 40000 + 2500, -60000], 8)
    path = tmp_path / "capture.cu8"
    raw.tofile(path)
    assert raw.size < 4 << 20
    adm, rej, st = replay_iq.replay(str(path), "cu8", band_rate, band_freq, reqs, str(tmp_path / "out"), buffer_size, 5, "native",
                                    waterfall_width=W)
    assert sorted(adm.values()) == sorted(reqs[:3]) and rej == [(reqs[3][0], reqs[3][1], 1)]
    assert st["blocks_dropped"] == 0
    for cid, (center, rate) in adm.items():
        out = np.fromfile(tmp_path / "out" / f"{cid}.cf32", dtype=np.float32)
        H = (out.size // 2) // rate
        assert H >= 3
        px = R.decode_png(str(tmp_path / "out" / f"{cid}.png"))
        assert px.shape == (H, W)
        assert np.array_equal(px, single(out, "cf32", rate, W)[1][:H]), cid
