"""GPU tests of the squelch of the serve object (xlating_serve_set_squelch, include/xlating_serve.h) on the scenario of
tests/squelch_cases.py: cu8 at 2.016 Msps, 8 calls of 2 blocks of 65536 bytes, twins at 48000 Hz and twins at 44100 Hz whose tones are
switched per call; the second of each pair is squelched.  In the families cf32, cs16 and cf32-cs16, with overlap 0 and 1 and hang_calls
0 and 1, the squelched twin's file is, byte for byte, its unsquelched twin's rows of exactly the calls the Python policy
(tests/meter_ref.py) opens on the restated powers of those rows; squelch_state and the log are the restatement's; the operations and
the bytes that cross fall on closed calls; a call with every client closed issues no pack.  Then squelch with set_tune, with gains and
levels, clear_squelch, a squelched client that leaves, and an object on which no squelch was ever set."""
import functools
import os
import tempfile

import numpy as np
import pytest

import meter_ref as MR
import sdr_server_amd as xl
import squelch_cases as SC

pytestmark = pytest.mark.gpu

EXT = {"cf32": "cf32", "cs16": "cs16", "cf32-cs16": "cs16"}
ESZ = {"cf32": 8, "cs16": 4, "cf32-cs16": 4}
TUNE = (1234.5, 250.0)  # shift_hz, ramp_hz_per_s of pair A in the variant "tune"
GAIN = -2               # of pair A in the variant "gain"
CLEAR_BEFORE, LEAVE_BEFORE = 4, 3


@functools.lru_cache(maxsize=None)
def run(family, overlap, hang, variant):
    """the capture through a Serve with the four clients.  variant: "base" no squelch ever; "sq" clients 1 and 3 squelched; "all" all
    four; "tune" sq + pair A tuned; "gain" sq + levels and a gain on pair A; "clear" sq, client 1 cleared before call CLEAR_BEFORE;
    "leave" sq, client 3 removed before call LEAVE_BEFORE
    -> dict: files, lens (per call, per client: outputs_device), ops (per call), state (per call: squelch_state of the live clients),
    logs (squelch_log at the end), levels / gain_logs (variant gain, per call)"""
    tmp = tempfile.mkdtemp(prefix="serve_squelch_")
    s = xl.Serve(SC.BAND_RATE, "cu8", SC.BUFFER, tmp, family=family, native=True, any_rate=True, overlap=overlap, group_blocks=SC.GROUP,
                 queue_bytes=1 << 20)
    ids = []
    for center, rate in SC.CLIENTS:
        code, resp, cid = s.request(xl.wire_build_request(center, rate, SC.BAND_FREQ, 0))
        assert code == 0
        ids.append(cid)
    squelched = () if variant == "base" else (0, 1, 2, 3) if variant == "all" else SC.SQUELCHED
    for i in squelched:
        s.set_squelch(ids[i], SC.OPEN_POWER, SC.CLOSE_POWER, hang)
    if variant == "tune":
        for i in (0, 1):
            s.set_tune(ids[i], *TUNE)
    if variant == "gain":
        s.enable_levels(True)
        for i in (0, 1):
            s.set_gain(ids[i], GAIN)
    raw = SC.capture()
    per = SC.GROUP * SC.BUFFER
    res = {"lens": [], "ops": [], "state": [], "logs": {}, "levels": [], "gain_logs": [], "tune_logs": {}, "ids": ids}
    live = list(range(4))
    for k in range(SC.CALLS):
        if variant == "clear" and k == CLEAR_BEFORE:
            s.clear_squelch(ids[1])
        if variant == "leave" and k == LEAVE_BEFORE:
            s.remove(ids[3])
            live.remove(3)
        s.blocks_host(raw[k * per:(k + 1) * per], SC.GROUP)
        res["ops"].append(s.last_ops())
        ptrs, lens = s.outputs_device([ids[i] for i in live])
        assert all(int(p) != 0 for p in ptrs), "outputs_device still gives every row"
        res["lens"].append({i: int(n) for i, n in zip(live, lens)})
        st = s.squelch_state([ids[i] for i in live])
        res["state"].append({i: (float(st["power"][j]), int(st["open"][j]), int(st["withheld_samples"][j])) for j, i in enumerate(live)})
        if variant == "gain":
            lv = s.levels([ids[0], ids[1]])
            res["levels"].append([(int(lv["peak_bits"][j]), int(lv["clipped"][j]), int(lv["nans"][j]), int(lv["gain_log2"][j])) for j in (0, 1)])
            res["gain_logs"].append(s.gain_log(ids[1]))
    for i in live:
        res["logs"][i] = s.squelch_log(ids[i])
        if variant == "tune":
            res["tune_logs"][i] = s.tune_log(ids[i])
    s.flush()
    assert s.dropped() == []
    s.close()
    res["files"] = {i: open(os.path.join(tmp, f"{cid}.{EXT[family]}"), "rb").read() for i, cid in enumerate(ids)}
    for f in os.listdir(tmp):
        os.remove(os.path.join(tmp, f))
    os.rmdir(tmp)
    return res


def split(data, lens, esz):
    out, pos = [], 0
    for n in lens:
        out.append(data[pos:pos + n * esz])
        pos += n * esz
    assert pos == len(data)
    return out


@functools.lru_cache(maxsize=None)
def restated(family, i, variant):
    """squelched client i's per-call (powers, lens): the restatement on the FINAL rows its unsquelched twin delivered -- cf32 rows in
    families 0 and 2 (the twin's file of the family-0 run), int16 pairs in family 1"""
    src_family = "cs16" if family == "cs16" else "cf32"
    src = run(src_family, False, 0, "tune" if variant == "tune" else "base")
    twin = i - 1 if i in SC.SQUELCHED else i
    lens = [src["lens"][k][twin] for k in range(SC.CALLS)]
    rows = split(src["files"][twin], lens, ESZ[src_family])
    if src_family == "cf32":
        powers = [MR.power_cf32(np.frombuffer(r, np.complex64)) for r in rows]
    else:
        powers = [MR.power_cs16(np.frombuffer(r, np.int16).reshape(-1, 2)) for r in rows]
    return powers, lens


NOMINAL = {"full": 10 * SC.OPEN_POWER, "half": (SC.OPEN_POWER * SC.CLOSE_POWER) ** 0.5, "off": 0.0}


@pytest.mark.parametrize("hang", [0, 1])
@pytest.mark.parametrize("overlap", [False, True])
@pytest.mark.parametrize("family", ["cf32", "cs16", "cf32-cs16"])
def test_twins(family, overlap, hang):
    r = run(family, overlap, hang, "sq")
    base = run(family, overlap, 0, "base")
    esz = ESZ[family]
    for i in SC.SQUELCHED:
        powers, lens = restated(family, i, "base")
        gates, log, withheld = SC.expected_gates(powers, lens, hang)
        assert gates == SC.expected_gates([NOMINAL[w] for w in SC.envelope(i)], lens, hang)[0], "the restated powers walk the envelope"
        # the twin is what it is without any squelch; the squelched file is its rows of the open calls, byte for byte
        assert r["files"][i - 1] == base["files"][i - 1] and len(base["files"][i - 1]) == esz * sum(lens)
        assert r["files"][i] == b"".join(seg for seg, g in zip(split(r["files"][i - 1], lens, esz), gates) if g), (i, gates)
        assert 0 < len(r["files"][i]) < len(r["files"][i - 1])
        assert r["logs"][i] == log and r["logs"][i - 1] == []
        acc = 0
        for k in range(SC.CALLS):
            assert r["lens"][k][i] == lens[k], "outputs_device gives the quiet rows too"
            acc += 0 if gates[k] else lens[k]
            assert r["state"][k][i] == (powers[k], int(gates[k]), acc), (i, k, r["state"][k][i], powers[k])
            assert r["state"][k][i - 1] == (0.0, 1, 0)
        assert acc == withheld == sum(lens) - len(r["files"][i]) // esz
    # the operations and the bytes: the meter's launch and two copies more than the call without a squelch, and the closed rows' bytes
    # fewer (an image places a row within 12 bytes of its predecessor's end)
    for k in range(SC.CALLS):
        bl, bc, bb = base["ops"][k]
        l, c, b = r["ops"][k]
        assert (l, c) == (bl + 1, bc + 2), (k, r["ops"][k], base["ops"][k])
        open_bytes = esz * sum(r["lens"][k][i] for i in range(4) if r["state"][k][i][1])
        all_bytes = esz * sum(r["lens"][k].values())
        assert open_bytes <= b <= open_bytes + 12 * 4 and all_bytes <= bb <= all_bytes + 12 * 4
        if open_bytes < all_bytes:
            assert b < bb
    assert any(r["ops"][k][2] < base["ops"][k][2] for k in range(SC.CALLS))


@pytest.mark.parametrize("family", ["cf32", "cs16", "cf32-cs16"])
def test_a_call_with_every_client_closed_issues_no_pack(family):
    r = run(family, True, 0, "all")
    base = run(family, True, 0, "base")
    for pair in (0, 2):
        powers, lens = restated(family, pair, "base")
        gates, log, withheld = SC.expected_gates(powers, lens, 0)
        want = b"".join(seg for seg, g in zip(split(base["files"][pair], lens, ESZ[family]), gates) if g)
        assert r["files"][pair] == r["files"][pair + 1] == want
        assert r["logs"][pair] == r["logs"][pair + 1] == log
    closed = [k for k in range(SC.CALLS) if not any(r["state"][k][i][1] for i in range(4))]
    assert 0 in closed and SC.CALLS - 1 in closed
    for k in range(SC.CALLS):
        bl, bc, bb = base["ops"][k]
        if k in closed:  # no pack launch, no table copy, no copy to the host: the feed, its carry and the meter remain
            assert r["ops"][k] == (bl - 1 + 1, bc - 2 + 2, 0), (k, r["ops"][k], base["ops"][k])
        else:
            assert r["ops"][k][:2] == (bl + 1, bc + 2) and 0 < r["ops"][k][2] <= bb


@pytest.mark.parametrize("family", ["cf32", "cf32-cs16"])
@pytest.mark.parametrize("overlap", [False, True])
def test_squelch_and_tune(family, overlap):
    """both twins of pair A tuned alike, the second squelched: its file is the tuned twin's rows of the open calls -- the phase has
    run on through the withheld ones -- and the tune log counts delivered samples"""
    r = run(family, overlap, 0, "tune")
    powers, lens = restated(family, 1, "tune")
    gates, log, withheld = SC.expected_gates(powers, lens, 0)
    assert gates == SC.expected_gates(*restated(family, 1, "base"), 0)[0], "a rotation moves no power across a mark"
    assert r["files"][0] != run(family, overlap, 0, "base")["files"][0]
    assert r["files"][1] == b"".join(seg for seg, g in zip(split(r["files"][0], lens, ESZ[family]), gates) if g)
    assert r["logs"][1] == log and [st[1][0] for st in r["state"]] == powers
    assert r["tune_logs"][0] == r["tune_logs"][1] and len(r["tune_logs"][1]) == 1 and r["tune_logs"][1][0][0] == 0
    # one tuner feed and one meter measurement a call
    base = run(family, overlap, 0, "base")
    assert [o[:2] for o in r["ops"]] == [(o[0] + 2, o[1] + 3) for o in base["ops"]]


def test_squelch_gain_and_levels():
    """family 2 with levels on and a gain on pair A: a closed call changes neither the levels nor the gain log of the squelched twin;
    an open call's levels are its twin's"""
    r = run("cf32-cs16", False, 0, "gain")
    powers, lens = restated("cf32-cs16", 1, "base")
    gates, log, withheld = SC.expected_gates(powers, lens, 0)
    assert r["files"][0] != run("cf32-cs16", False, 0, "base")["files"][0], "the gain acts"
    assert r["files"][1] == b"".join(seg for seg, g in zip(split(r["files"][0], lens, 4), gates) if g)
    assert r["logs"][1] == log
    prev = (0, 0, 0, 0)
    for k in range(SC.CALLS):
        twin, mine = r["levels"][k]
        assert twin[0] != 0 and twin[3] == GAIN
        assert mine == (twin if gates[k] else prev), (k, mine, twin, prev)
        prev = mine
        assert r["gain_logs"][k] == [(0, GAIN)]
    assert not gates[0] and r["levels"][0][1] == (0, 0, 0, 0), "zeros until a call was delivered"


@pytest.mark.parametrize("family", ["cf32", "cs16"])
def test_clear_squelch_reopens_from_the_next_call(family):
    r = run(family, True, 0, "clear")
    powers, lens = restated(family, 1, "base")
    q, lg = MR.Squelch(SC.OPEN_POWER, SC.CLOSE_POWER, 0), MR.SquelchLog()
    gates, produced, delivered = [], 0, 0
    for k in range(SC.CALLS):
        if k == CLEAR_BEFORE:
            lg.note(produced, delivered, True)
        g = True if k >= CLEAR_BEFORE else q.step(powers[k])
        if k < CLEAR_BEFORE:
            lg.note(produced, delivered, g)
        gates.append(g)
        produced += lens[k]
        delivered += lens[k] if g else 0
    assert not gates[CLEAR_BEFORE - 1] and SC.envelope(1)[CLEAR_BEFORE] == "off", "the call after the clear is a quiet one, and delivered"
    assert r["files"][1] == b"".join(seg for seg, g in zip(split(r["files"][0], lens, ESZ[family]), gates) if g)
    assert r["logs"][1] == lg.entries and lg.entries[-1][2] == 1
    assert [r["state"][k][1][1] for k in range(SC.CALLS)] == [int(g) for g in gates]
    assert r["state"][SC.CALLS - 1][1][0] == 0.0, "not measured any more"
    # client 3 goes on as in the plain run
    assert r["files"][3] == run(family, True, 0, "sq")["files"][3]


@pytest.mark.parametrize("overlap", [False, True])
def test_a_squelched_client_leaves(overlap):
    r = run("cf32", overlap, 1, "leave")
    sq = run("cf32", overlap, 1, "sq")
    for i in (0, 1, 2):
        assert r["files"][i] == sq["files"][i], i
    powers, lens = restated("cf32", 3, "base")
    gates, _, _ = SC.expected_gates(powers, lens, 1)
    want = b"".join(seg for seg, g in zip(split(sq["files"][2], lens, 8)[:LEAVE_BEFORE], gates) if g)
    assert r["files"][3] == want and len(want) > 0
    assert r["logs"][1] == sq["logs"][1]


@pytest.mark.parametrize("family", ["cf32", "cs16", "cf32-cs16"])
def test_an_object_never_squelched_is_what_it_was(family):
    """the operations of a call with a fractional client as the existing serve tests pin them (feed, carry, pack; two tables up, the
    rows down), twins equal, no log, nothing withheld"""
    r = run(family, False, 0, "base")
    assert [o[:2] for o in r["ops"]] == [(3, 3)] * SC.CALLS
    assert r["files"][0] == r["files"][1] and r["files"][2] == r["files"][3] and len(r["files"][0]) > 0
    assert all(r["logs"][i] == [] for i in range(4))
    assert all(st[i] == (0.0, 1, 0) for st in r["state"] for i in range(4))


def test_serve_iq_squelches_and_writes_the_log(tmp_path):
    """tools/serve_iq.py --squelch: every client squelched, one block per call there; <id>.squelch holds the log's lines, and with its
    two counts the file is rebuilt from the unsquelched stream: the samples of the stretches the log calls open, nothing else"""
    import importlib.util

    from conftest import ROOT

    spec = importlib.util.spec_from_file_location("serve_iq_tool", os.path.join(ROOT, "tools", "serve_iq.py"))
    serve_iq = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(serve_iq)
    path = tmp_path / "band.cu8"
    SC.capture().tofile(path)
    db = "%r:%r:1" % (float(10 * np.log10(SC.OPEN_POWER)), float(10 * np.log10(SC.CLOSE_POWER)))
    a = serve_iq.parse_args([str(path), "--band-freq", str(SC.BAND_FREQ), "--out", str(tmp_path / "o"), "--squelch=" + db])
    sq = serve_iq.parse_squelch(a.squelch)
    assert sq[2] == 1 and abs(sq[0] / SC.OPEN_POWER - 1) < 1e-12 and abs(sq[1] / SC.CLOSE_POWER - 1) < 1e-12
    adm, rej, st = serve_iq.replay(str(path), "cu8", SC.BAND_RATE, SC.BAND_FREQ, SC.CLIENTS, str(tmp_path / "o"), SC.BUFFER, 5, "native",
                                   any_rate=True, squelch=sq)
    assert rej == [] and len(adm) == 4 and st["blocks"] == SC.CALLS * SC.GROUP
    base = run("cf32", False, 0, "base")  # (the streams do not depend on the split into calls)
    for i, cid in enumerate(sorted(adm)):
        stream = base["files"][i]
        lines = [line.split() for line in open(tmp_path / "o" / f"{cid}.squelch")]
        assert lines[-1][0] == "withheld_samples"
        log = [tuple(int(v) for v in f) for f in lines[:-1]]
        assert [e[2] for e in log] == [k % 2 for k in range(len(log))] and log[0][:2] == (0, 0) and len(log) >= 4
        want, pos, is_open, delivered = b"", 0, True, 0
        for stream_sample, delivered_sample, o in log + [(len(stream) // 8, None, None)]:
            if is_open:
                want += stream[8 * pos:8 * stream_sample]
                delivered += stream_sample - pos
            assert delivered_sample is None or delivered_sample == delivered
            pos, is_open = stream_sample, bool(o)
        got = open(tmp_path / "o" / f"{cid}.cf32", "rb").read()
        assert got == want and 0 < len(got) < len(stream)
        assert int(lines[-1][1]) == (len(stream) - len(got)) // 8
    with pytest.raises(ValueError):
        serve_iq.parse_squelch("-40:-20")


def test_refusals(tmp_path):
    s = xl.Serve(SC.BAND_RATE, "cu8", SC.BUFFER, tmp_path, family="cf32", native=True, any_rate=True)
    code, resp, cid = s.request(xl.wire_build_request(*SC.CLIENTS[0], SC.BAND_FREQ, 0))
    assert code == 0
    for args in ((cid + 1, 1.0, 0.5, 0), (cid, 0.5, 1.0, 0), (cid, float("nan"), 0.0, 0), (cid, 1.0, float("nan"), 0), (cid, float("inf"), 0.0, 0),
                 (cid, 1.0, -0.5, 0), (cid, -1.0, -2.0, 0)):
        with pytest.raises(xl.XlatingError) as e:
            s.set_squelch(*args)
        assert e.value.code == -22
    for fn in (lambda: s.clear_squelch(cid + 1), lambda: s.squelch_state([cid + 1]), lambda: s.squelch_log(cid + 1)):
        with pytest.raises(xl.XlatingError) as e:
            fn()
        assert e.value.code == -22
    s.clear_squelch(cid)  # (a client that has none)
    assert s.squelch_log(cid) == []
    s.set_squelch(cid, 0.0, 0.0, 0)  # never closes: a level meter
    s.blocks_host(SC.capture()[:SC.BUFFER], 1)
    st = s.squelch_state([cid])
    assert st["open"][0] == 1 and st["power"][0] > 0.0 and st["withheld_samples"][0] == 0 and s.squelch_log(cid) == []
    s.close()
