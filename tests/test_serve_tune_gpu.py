"""GPU tests of tuning a running client of the serve object (xlating_serve_set_tune, include/xlating_serve.h) on a small band: cu8 at
2.016 Msps, 4 calls of 2 blocks of 65536 bytes.  Four FILE clients: twins of one request at 48000 Hz (the rate divides: D = 42) and twins
of one request at 44100 Hz (a fractional client), the second of each pair tuned with a shift and a ramp before call 0 and retuned before
call 2.  The tuned twin's file is, bit for bit, the restatement's rotation (tests/tune_ref.py) of the other's -- in family 0 as it is, in
family 2 narrowed by tests/delivery_narrow_ref.py (by tests/delivery_gain_ref.py under a gain) -- with overlap 0 and 1; the log names
the samples where the rule changes; outputs_device gives the tuned rows; a spectrum sees the shift; an object never tuned is what it
was; a tuned client that leaves disturbs nobody."""
import functools
import os
import tempfile

import numpy as np
import pytest

import delivery_gain_ref as GR
import delivery_narrow_ref as NR
import sdr_server_amd as xl
import tune_ref as TR
from pyoracle import Oracle

pytestmark = pytest.mark.gpu

BAND_FREQ = 437000000
BAND_RATE, BUFFER, GROUP, CALLS = 2016000, 65536, 2, 4
# (centre, rate): A and its twin A', B and its twin B'
CLIENTS = [(BAND_FREQ + 100000, 48000), (BAND_FREQ + 100000, 48000), (BAND_FREQ - 200000, 44100), (BAND_FREQ - 200000, 44100)]
TONES = [100000 + 6000, -200000 + 6000]  # Hz from the band's centre: 6 kHz above each pair's centre
# client index: [(before call, shift_hz, ramp_hz_per_s)]
TUNES = {1: [(0, 1234.5, 250.0), (2, -3000.0, 0.0)], 3: [(0, -2000.25, 40000.0), (2, 777.0, -1500.0)]}
EXT = {"cf32": "cf32", "cf32-cs16": "cs16"}


@functools.lru_cache(maxsize=None)
def capture():
    n = CALLS * GROUP * (BUFFER // 2)
    rng = np.random.default_rng(8)
    t = np.arange(n, dtype=np.float64) / BAND_RATE
    z = np.exp(2j * np.pi * np.asarray(TONES, dtype=np.float64)[:, None] * t[None, :]).sum(axis=0) * 0.4
    z += 0.002 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    v = np.stack([z.real, z.imag], axis=1).reshape(-1)
    raw = np.clip(np.round(127.5 + 127 * v), 0, 255).astype(np.uint8)
    raw.setflags(write=False)
    return raw


def admission(center, rate):
    req = xl.WireRequest(center, rate, BAND_FREQ, 0)
    code, adm, rs, why = xl.wire_admit_any_rate(req, BAND_RATE, 0, 5)
    assert code == 0
    return adm, rs.L, rs.M


def final_rate(center, rate):
    """the stated expression: (double)band_rate * L / ((double)D * M)"""
    adm, L, M = admission(center, rate)
    return float(BAND_RATE) * L / (float(adm.decimation) * M)


class Reader:
    """device rows to the host: one plain delivery pack of them, waited for"""

    def __init__(self):
        self.dlv = xl.Delivery(2)

    def rows(self, ptrs, lens):
        import torch

        torch.cuda.synchronize()
        t = self.dlv.pack(list(range(len(ptrs))), [int(p) for p in ptrs], [8 * int(n) for n in lens], torch.cuda.current_stream().cuda_stream)
        self.dlv.wait(t)
        out = [self.dlv.row(t, k).view(np.complex64) for k in range(len(ptrs))]
        self.dlv.release(t)
        return out


@functools.lru_cache(maxsize=None)
def run(family, overlap, tuned=True, gains=(), leave=None):
    """the capture through a Serve with the four clients -> dict: files (bytes per client index), lens (per call, per client), ops (per
    call), logs (tune_log per client index at the end), rows (the device rows per call, per client, read back)
    gains: ((client index, gain_log2), ..) set before call 0; leave: (client index, before call) removes that client"""
    tmp = tempfile.mkdtemp(prefix="serve_tune_")
    s = xl.Serve(BAND_RATE, "cu8", BUFFER, tmp, family=family, native=True, any_rate=True, overlap=overlap, group_blocks=GROUP,
                 queue_bytes=1 << 20)
    ids = []
    for center, rate in CLIENTS:
        code, resp, cid = s.request(xl.wire_build_request(center, rate, BAND_FREQ, 0))
        assert code == 0
        ids.append(cid)
    for i, g in gains:
        s.set_gain(ids[i], g)
    reader = Reader()
    raw = capture()
    per = GROUP * BUFFER
    res = {"lens": [], "ops": [], "rows": [], "logs": {}, "ids": ids}
    live = list(range(len(ids)))
    for k in range(CALLS):
        if leave is not None and leave[1] == k:
            s.remove(ids[leave[0]])
            live.remove(leave[0])
        for i, changes in TUNES.items():
            for kk, sh, ra in changes:
                if tuned and kk == k and i in live:
                    s.set_tune(ids[i], sh, ra)
        s.blocks_host(raw[k * per:(k + 1) * per], GROUP)
        res["ops"].append(s.last_ops()[:2])
        ptrs, lens = s.outputs_device([ids[i] for i in live])
        got = reader.rows(ptrs, lens)
        res["lens"].append({i: int(n) for i, n in zip(live, lens)})
        res["rows"].append({i: r for i, r in zip(live, got)})
    for i in live:
        res["logs"][i] = s.tune_log(ids[i])
    s.flush()
    assert s.dropped() == []
    s.close()
    reader.dlv.close()
    res["files"] = {i: open(os.path.join(tmp, f"{cid}.{EXT[family]}"), "rb").read() for i, cid in enumerate(ids)}
    for f in os.listdir(tmp):
        os.remove(os.path.join(tmp, f))
    os.rmdir(tmp)
    return res


@functools.lru_cache(maxsize=None)
def expected(i):
    """client i's tuned stream from its twin's cf32 file of the plain family-0 run: the restatement, call by call -> (complex64, the
    log it must leave)"""
    base = run("cf32", False)
    x = np.frombuffer(base["files"][i - 1], np.complex64)
    rate = final_rate(*CLIENTS[i])
    st, pos, out, log = None, 0, [], []
    for k in range(CALLS):
        for kk, sh, ra in TUNES[i]:
            if kk == k:
                F, R = TR.from_hz(sh, ra, rate)
                st = (st[0] if st else 0, F, R)
                log.append((pos, F, R))
        n = base["lens"][k][i]
        y, st = TR.rotate(x[pos:pos + n], *st)
        out.append(y)
        pos += n
    assert pos == x.size
    return np.concatenate(out), log


@pytest.mark.parametrize("overlap", [False, True])
def test_twins_in_family_0(overlap):
    r = run("cf32", overlap)
    assert len(r["files"][0]) > 0 and len(r["files"][2]) > 0
    for i in (1, 3):  # the integer-rate twins, the fractional twins
        want, log = expected(i)
        twin = np.frombuffer(r["files"][i - 1], np.complex64)
        got = np.frombuffer(r["files"][i], np.complex64)
        assert got.size == twin.size == want.size
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (i, np.nonzero(got.view(np.uint32) != want.view(np.uint32))[0][:8])
        assert not np.array_equal(got, twin)
        # the log names the samples where the file changes rule
        assert r["logs"][i] == log and log[0][0] == 0 and log[1][0] == r["lens"][0][i] + r["lens"][1][i]
        assert r["logs"][i - 1] == []
    # the untuned clients' files do not depend on the way of running, nor on who else is tuned
    assert r["files"][0] == run("cf32", False)["files"][0] and r["files"][2] == run("cf32", False)["files"][2]
    # the rates: 48000 exactly, and 44100 through the stated expression
    assert final_rate(*CLIENTS[0]) == 48000.0 and abs(final_rate(*CLIENTS[2]) - 44100.0) < 1e-6
    adm, L, M = admission(*CLIENTS[2])
    assert (L, M) != (1, 1)
    # one tuner feed per call: a launch and a copy more than the untuned call's feed, carry and pack
    assert r["ops"] == [(4, 4)] * CALLS


@pytest.mark.parametrize("overlap", [False, True])
@pytest.mark.parametrize("gains", [(), ((1, -3), (3, 1), (0, -3))], ids=["g0", "gains"])
def test_twins_in_family_2(overlap, gains):
    r = run("cf32-cs16", overlap, True, gains)
    g = dict(gains)
    base = run("cf32", False)
    for i in (1, 3):
        want, log = expected(i)
        narrow = NR.narrow_bytes(want) if g.get(i, 0) == 0 else GR.narrow_bytes(want, g[i])
        assert r["files"][i] == narrow, i
        assert r["logs"][i] == log
    # the untuned twins: their cf32 stream narrowed, as ever
    for i in (0, 2):
        x = np.frombuffer(base["files"][i], np.complex64)
        assert r["files"][i] == (NR.narrow_bytes(x) if g.get(i, 0) == 0 else GR.narrow_bytes(x, g[i])), i
    if gains:  # the same rule under the same gain: the gain acts on the tuned row
        assert r["files"][1] != r["files"][0] and GR.narrow_bytes(expected(1)[0], -3) == r["files"][1]


@pytest.mark.parametrize("family", ["cf32", "cf32-cs16"])
def test_outputs_device_gives_the_tuned_rows(family):
    r = run(family, True)
    for i in (1, 3):
        want, _ = expected(i)
        got = np.concatenate([r["rows"][k][i] for k in range(CALLS)])
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), i
    for i in (0, 2):
        got = np.concatenate([r["rows"][k][i] for k in range(CALLS)])
        assert got.tobytes() == run("cf32", False)["files"][i]


def test_integer_rate_stream_is_the_oracle_rotated():
    """the chain to the reference: the untuned twin's file is the oracle's stream (as the existing serve tests hold), so the tuned
    file is the restatement's rotation of the oracle's stream"""
    adm, L, M = admission(*CLIENTS[0])
    assert (adm.decimation, L, M) == (42, 1, 1)
    code, taps = xl.create_low_pass_filter(1.0, BAND_RATE, adm.lpf_cutoff, adm.lpf_transition)
    assert code == 0
    o = Oracle(adm.decimation, taps, adm.center_offset, BAND_RATE, BUFFER)
    raw = capture()
    want = np.concatenate([o.process("cu8", raw[off:off + BUFFER], "cf32") for off in range(0, raw.size, BUFFER)])
    o.close()
    assert run("cf32", False)["files"][0] == want.tobytes()


def test_spectrum_sees_the_shift():
    """a tone through a client tuned by -3000 Hz peaks 3000 Hz lower in a Spectrum row than through its twin: 64 bins of 46.875 Hz"""
    r = run("cf32", False)
    W = 1024
    start = r["lens"][0][1] + r["lens"][1][1]  # from call 2 on client A' is tuned by -3000 Hz, no ramp
    peaks = {}
    for i in (0, 1):
        x = np.frombuffer(r["files"][i], np.complex64)[start:]
        assert x.size >= 2 * W
        sp = xl.Spectrum(W, W, "cf32")  # (a row per transform)
        sp.feed(x.view(np.float32))
        db, _ = sp.take_rows()
        sp.close()
        assert db.shape[0] >= 2
        peaks[i] = [int(np.argmax(row)) for row in db]
    assert len(set(peaks[0])) == 1 and len(set(peaks[1])) == 1, peaks
    assert (peaks[0][0] - peaks[1][0]) % W == 3000 * W // 48000 == 64, peaks


def test_an_object_never_tuned_is_what_it_was():
    """the same last_ops as the existing serve tests expect of a call with a fractional client (feed, carry, pack; two tables up, the
    rows down), the same bytes as the untuned clients of every other run, twins equal, no log"""
    r = run("cf32", False, False)
    assert r["ops"] == [(3, 3)] * CALLS
    assert r["files"][0] == r["files"][1] and r["files"][2] == r["files"][3]
    base = run("cf32", False)
    assert r["files"][0] == base["files"][0] and r["files"][2] == base["files"][2]
    assert all(r["logs"][i] == [] for i in range(4))
    n = run("cf32-cs16", False, False)
    assert n["ops"] == [(3, 3)] * CALLS and n["files"][0] == NR.narrow_bytes(np.frombuffer(base["files"][0], np.complex64))


@pytest.mark.parametrize("overlap", [False, True])
def test_a_tuned_client_leaves_mid_run(overlap):
    r = run("cf32", overlap, True, (), (1, 2))  # A' leaves before call 2
    base = run("cf32", False)
    for i in (0, 2, 3):
        assert r["files"][i] == base["files"][i], i
    n01 = 8 * (base["lens"][0][1] + base["lens"][1][1])
    assert r["files"][1] == base["files"][1][:n01]
    assert r["ops"] == [(4, 4)] * CALLS  # B' is still tuned


def test_serve_iq_tunes_from_a_file(tmp_path):
    """tools/serve_iq.py --tune FILE: each line applied before the first call whose first band sample is at or after its time (one
    block per call there: the streams do not depend on the split); <id>.tune holds the log's lines"""
    import importlib.util

    from conftest import ROOT

    spec = importlib.util.spec_from_file_location("serve_iq_tool", os.path.join(ROOT, "tools", "serve_iq.py"))
    serve_iq = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(serve_iq)
    path = tmp_path / "band.cu8"
    capture().tofile(path)
    t2 = (2 * GROUP * (BUFFER // 2) - 0.5) / BAND_RATE  # (inside the last band sample before call 2 of the runs above)
    lines = ["# client_index seconds shift_hz ramp_hz_per_s"]
    for i, changes in TUNES.items():
        for kk, sh, ra in changes:
            lines.append(f"{i} {0.0 if kk == 0 else t2!r} {sh!r} {ra!r}  # before call {kk}")
    (tmp_path / "tune.txt").write_text("\n".join(reversed(lines)) + "\n")  # (any order: sorted by time)
    a = serve_iq.parse_args([str(path), "--band-freq", str(BAND_FREQ), "--out", str(tmp_path / "o"), "--tune", str(tmp_path / "tune.txt")])
    assert a.tune == str(tmp_path / "tune.txt")
    adm, rej, st = serve_iq.replay(str(path), "cu8", BAND_RATE, BAND_FREQ, CLIENTS, str(tmp_path / "o"), BUFFER, 5, "native", any_rate=True,
                                   tune=serve_iq.read_tune_file(a.tune))
    assert rej == [] and len(adm) == 4 and st["blocks"] == CALLS * GROUP
    ids = sorted(adm)
    base = run("cf32", False)
    for i, cid in enumerate(ids):
        assert open(tmp_path / "o" / f"{cid}.cf32", "rb").read() == base["files"][i], i
        if i in TUNES:
            got = [tuple(int(v) for v in line.split()) for line in open(tmp_path / "o" / f"{cid}.tune")]
            assert got == expected(i)[1]
        else:
            assert not os.path.exists(tmp_path / "o" / f"{cid}.tune")
    with pytest.raises(ValueError):
        serve_iq.replay(str(path), "cu8", BAND_RATE, BAND_FREQ, CLIENTS[:1], str(tmp_path / "q"), BUFFER, 5, "q15", tune=[(0, 0.0, 1.0, 0.0)])


def test_refusals(tmp_path):
    s = xl.Serve(BAND_RATE, "cu8", BUFFER, tmp_path, family="cs16", native=True, any_rate=True)
    code, resp, cid = s.request(xl.wire_build_request(*CLIENTS[0], BAND_FREQ, 0))
    assert code == 0
    for fn in (lambda: s.set_tune(cid, 100.0, 0.0), lambda: s.tune_log(cid)):
        with pytest.raises(xl.XlatingError) as e:
            fn()
        assert e.value.code == -22  # a Q15 rotator does not exist
    s.close()
    s = xl.Serve(BAND_RATE, "cu8", BUFFER, tmp_path, family="cf32", native=True, any_rate=True)
    code, resp, cid = s.request(xl.wire_build_request(*CLIENTS[0], BAND_FREQ, 0))
    for args in ((cid + 1, 100.0, 0.0), (cid, 24000.0, 0.0), (cid, float("nan"), 0.0), (cid, 0.0, 0.5 * 48000.0 ** 2)):
        with pytest.raises(xl.XlatingError) as e:
            s.set_tune(*args)
        assert e.value.code == -22
    assert s.tune_log(cid) == []
    s.set_tune(cid, 100.0, 0.0)
    s.set_tune(cid, 200.0, 1.0)  # two changes before any sample between them: the later one stands
    assert s.tune_log(cid) == [(0,) + TR.from_hz(200.0, 1.0, 48000.0)]
    s.close()
