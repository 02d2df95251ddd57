"""GPU tests of the serve object's gain and level meter (family XL_SERVE_CF32_AS_CS16: xlating_serve_set_gain, _set_auto_gain,
_enable_levels, _levels, _gain_log) on small engines: blocks of 65536 elements, four clients, one and two blocks a call, overlap 0 and
1.  The cf32 rows of every call are read from the device (xlating_serve_outputs_device, moved by a plain pack of a Delivery of the
test's own) and every file is held to the numpy restatement of those rows under the gain in force (tests/delivery_gain_ref.py), bit for
bit; the levels to the restatement's integers."""
import errno
import os

import numpy as np
import pytest
import torch

import delivery_gain_ref as GR
import sdr_server_amd as xl
import test_serve_gpu as SG

pytestmark = pytest.mark.gpu

BAND_FREQ, BUFFER = SG.BAND_FREQ, 65536
MODES = [(1, False), (1, True), (2, False), (2, True)]  # (blocks a call, overlap)


def join(s, center, rate):
    code, resp, cid = s.request(xl.wire_build_request(center, rate, BAND_FREQ, 0))
    assert code == 0 and resp == xl.wire_build_response(0, cid)
    return cid


def device_rows(reader, s, ids):
    """the latest call's final cf32 rows -> ({id: complex64 array}, pointers, lengths)"""
    torch.cuda.synchronize()
    ptrs, lens = s.outputs_device(ids)
    t = reader.pack(ids, ptrs, 8 * lens)
    reader.wait(t)
    rows = {i: reader.row(t, i).view(np.complex64).copy() for i in ids}
    reader.release(t)
    return rows, ptrs.tolist(), lens.tolist()


def image_bytes(ptrs, lens):
    end = 0
    for p, n in zip(ptrs, lens):
        if n == 0:
            continue
        at = (end & ~15) + ((p & 31) >> 1)
        end = (at + 16 if at < end else at) + 4 * n
    return end


def stated_bytes(ptrs, lens):
    rows = sum(1 for n in lens if n)
    return (image_bytes(ptrs, lens) + 15) // 16 * 16 + 12 * rows if rows else 0


def read(tmp, cid):
    return open(os.path.join(str(tmp), f"{cid}.cs16"), "rb").read()


# ------------------------------------------------------------------------------------------------------------ a cf32 band
CF_RATE = 1000000
CF_CLIENTS = [(BAND_FREQ + 100000, 100000), (BAND_FREQ - 250000, 100000), (BAND_FREQ + 300, 50000), (BAND_FREQ - 250000, 48000)]


def cf32_band(nblocks, seed=41):
    """cf32 at 1 Msps in +-1: tones at the clients' centres and a little noise; peaks near 0.9"""
    n = nblocks * BUFFER // 2
    rng = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64) / CF_RATE
    z = sum(a * np.exp(2j * np.pi * f * t) for a, f in ((0.35, 101000.0), (0.3, -249500.0), (0.2, 1300.0)))
    z = z + 0.01 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    return np.stack([z.real, z.imag], axis=1).reshape(-1).astype(np.float32)


def run_cf32(tmp, x, group, overlap, gain=None, levels=False, nblocks=4):
    """the band x through a family-2 object with every client at `gain` -> ({client index: file bytes}, per-call records, clipped totals)"""
    os.makedirs(str(tmp), exist_ok=True)
    s = xl.Serve(CF_RATE, "cf32", BUFFER, str(tmp), family="cf32-cs16", native=True, any_rate=True, overlap=overlap, group_blocks=group,
                 queue_bytes=1 << 20)
    reader = xl.Delivery(2)
    ids = [join(s, c, r) for c, r in CF_CLIENTS]
    assert ids == sorted(ids)
    for cid in ids:
        if gain is not None:
            s.set_gain(cid, gain)
    if levels:
        s.enable_levels(True)
    calls = []
    for part in np.split(x, nblocks // group):
        s.blocks_host(part, group)
        rows, ptrs, lens = device_rows(reader, s, ids)
        calls.append({"rows": rows, "ops": s.last_ops(), "ptrs": ptrs, "lens": lens, "levels": s.levels(ids)})
    s.flush()
    final = s.levels(ids)
    assert s.dropped() == []
    s.close()
    reader.close()
    return {k: read(tmp, cid) for k, cid in enumerate(ids)}, calls, final, ids


@pytest.mark.parametrize("group,overlap", [(1, False), (2, True)])
def test_a_scaled_cf32_band_under_gain_minus_12_is_the_unit_band(group, overlap, tmp_path):
    """a cf32 recording scaled by 2^12 with every client at gain -12 against the same recording in +-1 at gain 0: the engine's
    arithmetic commutes with a power of two, so the files are identical; the same scaled band at gain 0 saturates, is counted, and its
    files are the restatement of its rows"""
    x = cf32_band(4)
    unit, calls1, _, _ = run_cf32(tmp_path / "unit", x, group, overlap)
    scaled, calls12, final12, ids = run_cf32(tmp_path / "scaled", x * np.float32(4096.0), group, overlap, gain=-12)
    assert all(len(unit[k]) > 4000 for k in unit) and scaled == unit
    assert all(c["ops"][:2] == (3, 3) and c["ops"][2] == image_bytes(c["ptrs"], c["lens"]) for c in calls1)  # nothing enabled: the parent's call
    assert all(c["ops"][:2] == (3, 4) and c["ops"][2] == stated_bytes(c["ptrs"], c["lens"]) for c in calls12)
    assert final12["clipped_total"].tolist() == [0] * 4 and final12["gain_log2"].tolist() == [-12] * 4
    for k in range(4):  # the files are the restatement of the device rows under the gain
        assert scaled[k] == b"".join(GR.narrow_bytes(c["rows"][ids[k]], -12) for c in calls12)
    hot, calls0, final0, ids0 = run_cf32(tmp_path / "hot", x * np.float32(4096.0), group, overlap, gain=0, levels=True)
    for k in range(4):
        want = b"".join(GR.narrow_bytes(c["rows"][ids0[k]], 0) for c in calls0)
        assert hot[k] == want
        v = np.frombuffer(hot[k], np.int16)
        y = np.concatenate([c["rows"][ids0[k]] for c in calls0]).view(np.float32)
        sat = (v == 32767) | (v == -32768)
        assert np.array_equal(sat, (np.rint(y.astype(np.float64) * 32768.0) >= 32767) | (np.rint(y.astype(np.float64) * 32768.0) <= -32768))
        clipped = sum(GR.level(c["rows"][ids0[k]], 0)[1] for c in calls0)
        assert int(final0["clipped_total"][k]) == clipped
    assert int(final0["clipped_total"][0]) > 0 and int(final0["clipped_total"][1]) > 0  # (the clients on the tones)
    # the levels of a call are those of its rows: of the latest call with overlap 0, of the call before with overlap 1
    for j, c in enumerate(calls0):
        src = j - 1 if overlap else j
        if src < 0:
            assert c["levels"]["peak_bits"].tolist() == [0] * 4
            continue
        want = [GR.level(calls0[src]["rows"][cid], 0) for cid in ids0]
        got = list(zip(c["levels"]["peak_bits"].tolist(), c["levels"]["clipped"].tolist(), c["levels"]["nans"].tolist()))
        assert got == want, (j, got, want)
    want = [GR.level(calls0[-1]["rows"][cid], 0) for cid in ids0]  # after the flush: the last call's
    assert list(zip(final0["peak_bits"].tolist(), final0["clipped"].tolist(), final0["nans"].tolist())) == want


# ------------------------------------------------------------------------------------------------------------ a cu8 band
CU_RATE = 200000
CU_CLIENTS = [(BAND_FREQ + 12000, 50000), (BAND_FREQ - 20000, 48000), (BAND_FREQ + 30000, 25000), (BAND_FREQ + 12000, 48000)]
# per client, the gain of each of the six blocks' calls (a call of two blocks takes the first block's)
SCHEDULE = [[0, 3, 3, -2, -2, 7], [1, 1, -4, -4, 0, 0], [0, 0, 0, 0, 0, 0], [-48, 48, 48, 5, 5, 5]]


def cu8_band():
    return SG.tones_u8(6 * BUFFER // 2, CU_RATE, [12000 + 3000, -20000 - 1500, 30000 + 500], 9)


@pytest.mark.parametrize("group,overlap", MODES)
def test_gain_changed_between_calls_on_a_cu8_band(group, overlap, tmp_path):
    """an integer-rate client (50 kHz of 200 kHz), a fractional one (48 kHz through the float bank) and two more: every file equals
    narrow(row, g) of the rows of xlating_serve_outputs_device, call by call, with the gains changed between calls by set_gain; the
    gain log's first_sample is the file offset (in samples) where the bytes change scale"""
    s = xl.Serve(CU_RATE, "cu8", BUFFER, str(tmp_path), family="cf32-cs16", native=True, any_rate=True, overlap=overlap,
                 group_blocks=group, queue_bytes=1 << 20)
    reader = xl.Delivery(2)
    ids = [join(s, c, r) for c, r in CU_CLIENTS]
    x = cu8_band()
    want = {cid: [] for cid in ids}
    log = {cid: [] for cid in ids}
    samples = {cid: 0 for cid in ids}
    now = {cid: 0 for cid in ids}
    for b in range(0, 6, group):
        for k, cid in enumerate(ids):
            g = SCHEDULE[k][b]
            if g != now[cid]:
                log[cid].append((samples[cid], g))
            s.set_gain(cid, g)  # (also when it does not change: no entry then)
            now[cid] = g
        s.blocks_host(x[b * BUFFER:(b + group) * BUFFER], group)
        rows, ptrs, lens = device_rows(reader, s, ids)
        gained = any(now[c] != 0 for c in ids)
        launches, copies, d2h = s.last_ops()
        assert (launches, copies, d2h) == ((3, 4, stated_bytes(ptrs, lens)) if gained else (3, 3, image_bytes(ptrs, lens)))
        for cid in ids:
            want[cid].append(GR.narrow_bytes(rows[cid], now[cid]))
            samples[cid] += rows[cid].size
    s.flush()
    assert s.dropped() == []
    lv = s.levels(ids)
    for k, cid in enumerate(ids):
        assert s.gain_log(cid) == log[cid], (cid, s.gain_log(cid), log[cid])
        assert int(lv["gain_log2"][k]) == SCHEDULE[k][5 if group == 1 else 4]
        assert (int(lv["peak_bits"][k]), int(lv["clipped"][k]), int(lv["nans"][k])) == GR.level(rows[cid], now[cid])
    assert s.gain_log(ids[0], 1) == log[ids[0]][-1:]
    s.close()
    reader.close()
    for cid in ids:
        data = read(tmp_path, cid)
        assert data == b"".join(want[cid]) and len(data) == 4 * samples[cid] > 0, cid
    assert len(os.listdir(str(tmp_path))) == 4


# ------------------------------------------------------------------------------------------------------------ automatic gain
@pytest.mark.parametrize("overlap", [False, True])
def test_auto_gain_answers_a_step_of_64_in_level(overlap, tmp_path):
    """three calls at a level the policy leaves alone (peaks in [1/8, 1)), then the band 2^6 louder: the log shows ONE drop, by the
    step's top, within the lag the header documents (from the call after the step with overlap 0, from the second call after it with
    overlap 1); no clipped sample from there on; the stream undone per the log is within half a delivered LSB of the cf32 rows
    wherever it did not clip"""
    nblocks, step_at = 8, 3
    x = cf32_band(nblocks, seed=43)
    x[step_at * BUFFER:] *= np.float32(64.0)
    s = xl.Serve(CF_RATE, "cf32", BUFFER, str(tmp_path), family="cf32-cs16", native=True, any_rate=True, overlap=overlap, queue_bytes=1 << 20)
    reader = xl.Delivery(2)
    ids = [join(s, c, r) for c, r in CF_CLIENTS[:2]] + [join(s, *CF_CLIENTS[3])]  # the two on the tones, and the fractional one on a tone
    for cid in ids:
        s.set_auto_gain(cid, True)
    rows, before = {cid: [] for cid in ids}, {cid: [] for cid in ids}
    for j, part in enumerate(np.split(x, nblocks)):
        for cid in ids:
            before[cid].append(sum(r.size for r in rows[cid]))
        s.blocks_host(part)
        assert s.last_ops()[:2] == (3, 4)  # (automatic gain packs through the gain call from the first call on)
        got, _, _ = device_rows(reader, s, ids)
        for cid in ids:
            rows[cid].append(got[cid])
    s.flush()
    lag = 2 if overlap else 1
    lv = s.levels(ids)
    logs = {cid: s.gain_log(cid) for cid in ids}
    s.close()
    reader.close()
    for k, cid in enumerate(ids):
        y = [r.view(np.float32) for r in rows[cid]]
        peaks = [float(np.abs(v).max()) for v in y]
        assert all(0.125 <= p < 1.0 for p in peaks[:step_at]), peaks  # the policy leaves these alone
        top = int(np.frexp(peaks[step_at])[1])  # |peak| in [2^(top - 1), 2^top) at gain 0
        assert 5 <= top <= 7 and all(np.frexp(p)[1] <= top for p in peaks[step_at:]), peaks
        assert logs[cid] == [(before[cid][step_at + lag], -top)], (logs[cid], before[cid], top)
        gains = [0] * (step_at + lag) + [-top] * (nblocks - step_at - lag)
        data = np.frombuffer(read(tmp_path, cid), np.int16)
        assert data.tobytes() == b"".join(GR.narrow_bytes(r, g) for r, g in zip(rows[cid], gains))
        clipped = [GR.level(r, g)[1] for r, g in zip(rows[cid], gains)]
        assert sum(clipped[:step_at]) == 0 and all(c > 0 for c in clipped[step_at:step_at + lag]) and sum(clipped[step_at + lag:]) == 0
        assert int(lv["clipped_total"][k]) == sum(clipped) and int(lv["gain_log2"][k]) == -top and int(lv["clipped"][k]) == 0
        at = 0
        for v, g in zip(y, gains):  # undone per the log
            out = data[at:at + v.size]
            at += v.size
            ok = (out > -32768) & (out < 32767)  # (a value the clamp may have made)
            err = np.abs(GR.undo(out, g) - v.astype(np.float64))
            assert float(err[ok].max()) <= 2.0 ** -(15 + g) / 2, (cid, g)
        assert at == data.size


# ------------------------------------------------------------------------------------------------------------ nothing enabled; refusals
def test_with_nothing_enabled_the_call_is_the_parents_and_refusals(tmp_path):
    """a family-2 object nobody asked a gain or a level of: its files and operation counts are those of pack_device_cs16 driven by hand
    on the same rows; enabling levels changes the counts as the header says and not one byte; the calls are refused on families 0 and 1,
    on a dead id and for a gain outside -48 .. 48"""
    x = cu8_band()
    os.makedirs(str(tmp_path / "f2"))
    s = xl.Serve(CU_RATE, "cu8", BUFFER, str(tmp_path / "f2"), family="cf32-cs16", native=True, any_rate=True, queue_bytes=1 << 20)
    hand = xl.Delivery(2)
    ids = [join(s, c, r) for c, r in CU_CLIENTS]
    want = {cid: [] for cid in ids}
    for b in range(6):
        if b == 3:
            s.enable_levels(True)
        if b == 5:
            s.enable_levels(False)
        s.blocks_host(x[b * BUFFER:(b + 1) * BUFFER])
        torch.cuda.synchronize()
        ptrs, lens = s.outputs_device(ids)
        t = hand.pack_cs16(ids, ptrs, lens)
        hand_ops = hand.last_ops()
        hand.wait(t)
        for cid in ids:
            want[cid].append(hand.row(t, cid).tobytes())
        hand.release(t)
        launches, copies, d2h = s.last_ops()
        if 3 <= b < 5:
            assert (launches, copies, d2h) == (2 + hand_ops[0], 1 + hand_ops[1] + 1, stated_bytes(ptrs.tolist(), lens.tolist()))
            lv = s.levels(ids)
            assert lv["gain_log2"].tolist() == [0] * 4 and all(int(p) > 0 for p in lv["peak_bits"])
        else:
            assert (launches, copies, d2h) == (2 + hand_ops[0], 1 + hand_ops[1], hand_ops[2])  # the bank's feed, and the parent's pack
    for cid in ids:
        assert s.gain_log(cid) == []
    # refusals
    for bad in (49, -49, 1000):
        with pytest.raises(xl.XlatingError) as e:
            s.set_gain(ids[0], bad)
        assert e.value.code == -errno.EINVAL
    dead = max(ids) + 17
    for call in (lambda: s.set_gain(dead, 1), lambda: s.set_auto_gain(dead, True), lambda: s.levels([ids[0], dead]), lambda: s.gain_log(dead)):
        with pytest.raises(xl.XlatingError) as e:
            call()
        assert e.value.code == -errno.EINVAL
    s.flush()
    s.close()
    hand.close()
    for cid in ids:
        assert read(tmp_path / "f2", cid) == b"".join(want[cid])
    for family in ("cf32", "cs16"):
        os.makedirs(str(tmp_path / family))
        o = xl.Serve(CU_RATE, "cu8", BUFFER, str(tmp_path / family), family=family, any_rate=True, queue_bytes=1 << 20)
        cid = join(o, *CU_CLIENTS[0])
        for call in (lambda: o.set_gain(cid, 1), lambda: o.set_auto_gain(cid, True), lambda: o.enable_levels(True), lambda: o.levels([cid]),
                     lambda: o.gain_log(cid)):
            with pytest.raises(xl.XlatingError) as e:
                call()
            assert e.value.code == -errno.EINVAL
        o.close()


def test_serve_iq_writes_the_gain_files(tmp_path):
    """tools/serve_iq.py --cs16-out --gain G / --auto-gain: the samples are the object's, and <id>.gain holds the gain log's lines and
    the final clipped_total"""
    serve_iq = SG._tool("serve_iq")
    path = tmp_path / "band.cu8"
    cu8_band().tofile(path)
    clients = CU_CLIENTS[:2]
    args = (str(path), "cu8", CU_RATE, BAND_FREQ, clients)
    plain, _, _ = serve_iq.replay(*args, str(tmp_path / "plain"), BUFFER, 5, "native", any_rate=True, cs16_out=True)
    fixed, _, _ = serve_iq.replay(*args, str(tmp_path / "fixed"), BUFFER, 5, "native", any_rate=True, cs16_out=True, gain=-3)
    auto, _, _ = serve_iq.replay(*args, str(tmp_path / "auto"), BUFFER, 5, "native", any_rate=True, cs16_out=True, auto_gain=True)
    assert plain == fixed == auto and len(plain) == 2 and not [f for f in os.listdir(str(tmp_path / "plain")) if f.endswith(".gain")]
    for cid in plain:
        base = np.frombuffer(read(tmp_path / "plain", cid), np.int16).astype(np.int64)
        lines = open(tmp_path / "fixed" / f"{cid}.gain").read().split("\n")
        assert lines[0] == "0 -3" and lines[1].startswith("clipped_total ") and lines[2:] == [""]
        got = np.frombuffer(read(tmp_path / "fixed", cid), np.int16).astype(np.int64)
        assert got.size == base.size > 0 and int(np.abs(8 * got - base).max()) <= 4  # (8 x the rounded y * 2^12 against the rounded y * 2^15)
        lines = open(tmp_path / "auto" / f"{cid}.gain").read().split("\n")
        assert lines[-2].startswith("clipped_total ") and all(len(l.split()) == 2 for l in lines[:-1])
    with pytest.raises(ValueError):
        serve_iq.replay(*args, str(tmp_path / "bad"), BUFFER, 5, "native", any_rate=True, gain=3)
    a = serve_iq.parse_args([str(path), "--band-freq", str(BAND_FREQ), "--out", str(tmp_path), "--cs16-out", "--gain", "-5", "--auto-gain"])
    assert a.gain == -5 and a.auto_gain and a.cs16_out
