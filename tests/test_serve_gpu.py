"""GPU tests of the serve object (include/xlating_serve.h) on the shape of test_replay_any_rate: band 192000 Hz, blocks of 65536 bytes,
one client at 48000 Hz (the rate divides: D = 4) and one at 44100 Hz (D = 4, then 147 / 160), about two seconds of tones.  The files the
object writes are compared with three references computed once per family: the oracle's stream (integer-rate client, bit for bit), the
restatements of the second stage (tests/resample_ref.py's own bound for cf32, tests/resample_q15_ref.py bit for bit for cs16), and the
streams obtained by driving the engine and the bank by hand on the same blocks (byte for byte: delivery adds no arithmetic).  Then the
pins (overlap, the cs16 file that xlating_sinks_submit leaves empty, the bytes that cross, the operation counts), the wire answers,
sockets, joins and leaves, tools/serve_iq.py against tools/replay_iq.py, and the C demo."""
import errno
import functools
import gzip
import importlib.util
import os
import socket
import subprocess
import threading

import numpy as np
import pytest

import resample_q15_ref as QR
import resample_ref as RR
import sdr_server_amd as xl
from conftest import ROOT
from pyoracle import Oracle

pytestmark = pytest.mark.gpu

BAND_FREQ = 460100000
BAND_RATE, BUFFER = 192000, 65536
REQS = [(BAND_FREQ + 12000, 44100), (BAND_FREQ - 20000, 48000)]
FAMILIES = {"cf32": ("native", 8, np.complex64), "cs16": ("q15", 4, np.int16)}


def tones_u8(n, band_rate, freqs, seed):
    """a cu8 band of n samples: one tone per frequency (Hz from the band's centre), equal amplitudes, a little noise"""
    rng = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64) / band_rate
    z = np.exp(2j * np.pi * np.asarray(freqs, dtype=np.float64)[:, None] * t[None, :]).sum(axis=0) * (0.8 / len(freqs))
    z += 0.002 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    v = np.stack([z.real, z.imag], axis=1).reshape(-1)
    return np.clip(np.round(127.5 + 127 * v), 0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def capture():
    raw = tones_u8(2 * BAND_RATE + 1234, BAND_RATE, [12000 + 3000, -20000 - 1500], 8)
    raw.setflags(write=False)
    return raw


def blocks():
    raw = capture()
    return [raw[off:off + BUFFER] for off in range(0, raw.size, BUFFER)]


def calls(group):
    """the capture as (array, nblocks) calls: runs of up to `group` full blocks, the short last block alone"""
    bl, out = blocks(), []
    full = [b for b in bl if b.size == BUFFER]
    for i in range(0, len(full), group):
        out.append((np.concatenate(full[i:i + group]), len(full[i:i + group])))
    out += [(b, 1) for b in bl if b.size != BUFFER]
    return out


def admission(center, rate):
    req = xl.WireRequest(center, rate, BAND_FREQ, 0)
    code, adm, rs, why = xl.wire_admit_any_rate(req, BAND_RATE, 0, 5)
    assert code == 0
    taps = None
    if (rs.L, rs.M) != (1, 1):
        code, taps = xl.wire_resample_taps(req, rs, 5)
        assert code == 0
    return req, adm, rs.L, rs.M, taps


@functools.lru_cache(maxsize=None)
def by_hand(family):
    """the engine and the bank driven by hand, one block per call: {rate: the client's final stream as bytes}, and the engine's own
    stream of the fractional client (the second stage's input)"""
    variant, esz, dt = FAMILIES[family]
    eng = xl.BatchEngine(BAND_RATE, "cu8", BUFFER)
    bank = xl.ResamplerBankQ15() if family == "cs16" else xl.ResamplerBank()
    cids, final, mid = {}, {r: [] for _, r in REQS}, []
    for center, rate in REQS:
        req, adm, L, M, taps = admission(center, rate)
        cids[rate] = xl.wire_add_client(eng, adm, BAND_RATE)
    req, adm, L, M, taps = admission(*REQS[0])
    assert (adm.decimation, L, M) == (4, 147, 160)  # (admission picks D = 4 and 147 / 160)
    sid = bank.add(L, M, taps)
    out = eng.output_cs16 if family == "cs16" else eng.output
    for b in blocks():
        eng.process_host(b, variant)
        eng.fetch()
        final[48000].append(out(cids[48000]))
        mid.append(out(cids[44100]))
        bank.feed_engine(eng, {cids[44100]: sid})
        bank.fetch()
        final[44100].append(bank.output(sid))
    bank.close()
    eng.close()
    return {r: np.concatenate(v).tobytes() for r, v in final.items()}, np.concatenate(mid)


@functools.lru_cache(maxsize=None)
def oracle_stream(family, center, nrepeat=1, first=0, last=None, rate=48000):
    """the oracle's stream of an integer-rate client over blocks()[first:last], repeated, as bytes"""
    req, adm, L, M, _ = admission(center, rate)
    assert (L, M) == (1, 1)
    code, taps = xl.create_low_pass_filter(1.0, BAND_RATE, adm.lpf_cutoff, adm.lpf_transition)
    assert code == 0
    o = Oracle(adm.decimation, taps, adm.center_offset, BAND_RATE, BUFFER)
    parts = [o.process("cu8", b, family) for _ in range(nrepeat) for b in blocks()[first:last]]
    o.close()
    return np.concatenate(parts).tobytes()


def serve_files(tmp, family, gz=False, overlap=False, group=1, **kw):
    """the capture through a Serve with the two FILE clients -> ({rate: file bytes}, {rate: id}, per-call (last_ops, rows)).  The queues
    hold the whole capture (a D = 4 client's stream is 770 KB): no writer thread, however late, can lose a client here"""
    os.makedirs(tmp, exist_ok=True)
    kw.setdefault("queue_bytes", 1 << 20)
    s = xl.Serve(BAND_RATE, "cu8", BUFFER, tmp, family=family, native=True, any_rate=True, gzip=gz, overlap=overlap, group_blocks=group, **kw)
    ids = {}
    for center, rate in REQS:
        code, resp, cid = s.request(xl.wire_build_request(center, rate, BAND_FREQ, 0))
        assert code == 0 and resp == xl.wire_build_response(0, cid)
        ids[rate] = cid
    log = []
    for x, n in calls(group):
        s.blocks_host(x, n)
        log.append((s.last_ops(), s.outputs_device(list(ids.values()))))
    s.flush()
    assert s.dropped() == []
    s.close()
    ext = family + (".gz" if gz else "")
    rd = (lambda p: gzip.open(p, "rb").read()) if gz else (lambda p: open(p, "rb").read())
    return {rate: rd(os.path.join(tmp, f"{cid}.{ext}")) for rate, cid in ids.items()}, ids, log


# ------------------------------------------------------------------------------------------------------------ the streams
@pytest.mark.parametrize("family", ["cf32", "cs16"])
def test_files_against_the_oracle_and_the_restatements(family, tmp_path):
    variant, esz, dt = FAMILIES[family]
    files, ids, log = serve_files(str(tmp_path), family)
    hand, mid = by_hand(family)
    # the integer-rate client: bit for bit the oracle's stream.  For cs16 this is the file xlating_sinks_submit leaves empty today
    assert len(files[48000]) > 0 and files[48000] == oracle_stream(family, REQS[1][0])
    # the fractional client against the restatement of the second stage applied to the engine's stream
    req, adm, L, M, taps = admission(*REQS[0])
    if family == "cf32":
        y = np.frombuffer(files[44100], np.complex64)
        assert y.size == RR.counts(L, M, mid.size)
        RR.check(y, L, M, taps, mid, "serve")
    else:
        y = np.frombuffer(files[44100], np.int16).reshape(-1, 2)
        want = QR.restate(L, M, taps, mid)
        assert y.shape == want.shape and np.array_equal(y, want)
    # and byte for byte the engine and the bank driven by hand
    assert files[48000] == hand[48000] and files[44100] == hand[44100]
    # what crossed to the host per call: exactly the delivered samples, each row behind at most 12 bytes of padding -- not the arena
    for (launches, copies, d2h), (ptrs, lens) in log:
        assert (launches, copies) == (3, 3)  # the bank's feed and carry + the pack; two tables up, the rows down
        end = 0
        for p, n in zip(ptrs.tolist(), lens.tolist()):
            at = (end & ~15) + (p & 15)
            end = (at + 16 if at < end else at) + n * esz
        assert d2h == end and esz * int(lens.sum()) <= d2h <= esz * int(lens.sum()) + 12 * len(lens)
    total = sum(int(lens.sum()) for _, (_, lens) in log)
    assert esz * total == len(files[48000]) + len(files[44100])


@pytest.mark.parametrize("group", [1, 4])
@pytest.mark.parametrize("overlap", [False, True])
@pytest.mark.parametrize("gz", [False, True])
@pytest.mark.parametrize("family", ["cf32", "cs16"])
def test_every_way_of_running_writes_the_same_files(family, gz, overlap, group, tmp_path):
    """FILE with and without gzip, overlap 0 and 1, one block per call and four: the streams of the engine and the bank driven by hand"""
    files, ids, log = serve_files(str(tmp_path), family, gz, overlap, group)
    hand, _ = by_hand(family)
    assert files[48000] == hand[48000] and files[44100] == hand[44100]
    assert sorted(os.listdir(tmp_path)) == sorted(f"{cid}.{family}{'.gz' if gz else ''}" for cid in ids.values())


def test_operation_counts_do_not_grow_with_the_clients(tmp_path):
    counts = {}
    for n in (2, 64):
        s = xl.Serve(BAND_RATE, "cu8", BUFFER, tmp_path / str(n), family="cf32", native=True, any_rate=True)
        os.makedirs(tmp_path / str(n))
        for i in range(n):
            code, resp, cid = s.request(xl.wire_build_request(BAND_FREQ - 40000 + 1000 * i, 44100 if i % 2 else 48000, BAND_FREQ, 0))
            assert code == 0
        assert s.engine().num_clients == n
        for b in blocks()[:2]:
            s.blocks_host(b)
            counts.setdefault(n, []).append(s.last_ops()[:2])
        s.flush()
        s.close()
        assert len(os.listdir(tmp_path / str(n))) == n
    assert counts[2] == counts[64] == [(3, 3), (3, 3)]


# ------------------------------------------------------------------------------------------------------------ the wire
def test_wire_answers(tmp_path):
    s = xl.Serve(BAND_RATE, "cu8", BUFFER, tmp_path, family="cf32", native=True, any_rate=True)
    eng = s.engine()
    msg = xl.wire_build_request(REQS[1][0], 48000, BAND_FREQ, 0)
    # what the parsers say about short and foreign messages comes back as it is
    for bad, code in ((msg[:1], -errno.EAGAIN), (msg[:9], -errno.EAGAIN), (b"\x01" + msg[1:], -errno.EPROTO), (xl.wire_build_header(3), -errno.EPROTO)):
        with pytest.raises(xl.XlatingError) as e:
            s.request(bad)
        assert e.value.code == code
    # invalid requests (a rate of zero, a client band outside the server's): INVALID_REQUEST, the server's answer for them
    for center, rate, details in ((REQS[1][0], 0, 1), (BAND_FREQ + 500000, 48000, 1)):
        req = xl.WireRequest(center, rate, BAND_FREQ, 0)
        assert xl.wire_admit_any_rate(req, BAND_RATE, 0, 5)[3] == details
        code, resp, cid = s.request(xl.wire_build_request(center, rate, BAND_FREQ, 0))
        assert code == 1 and cid is None and resp == xl.wire_build_response(1, details)
    assert eng.num_clients == 0
    code, resp, a = s.request(msg)
    assert code == 0 and resp == xl.wire_build_response(0, a)
    # a second band is refused while clients run, with OUT_OF_BAND_FREQ ...
    other = xl.wire_build_request(REQS[1][0] + 1000000, 48000, BAND_FREQ + 1000000, 0)
    req = xl.WireRequest(REQS[1][0] + 1000000, 48000, BAND_FREQ + 1000000, 0)
    c0, _, _, why = xl.wire_admit_any_rate(req, BAND_RATE, BAND_FREQ, 5)
    assert c0 != 0 and why == 2
    code, resp, cid = s.request(other)
    assert code == 1 and resp == xl.wire_build_response(1, why) and eng.num_clients == 1
    # ... and admitted after they have all left
    s.remove(a)
    assert eng.num_clients == 0
    code, resp, b = s.request(other)
    assert code == 0 and resp == xl.wire_build_response(0, b) and eng.num_clients == 1
    with pytest.raises(xl.XlatingError):
        s.remove(b + 7)  # not a client
    s.close()
    # a sink that cannot be opened: INTERNAL_ERROR, and what had been added is undone
    s = xl.Serve(BAND_RATE, "cu8", BUFFER, tmp_path / "missing", family="cs16", any_rate=True)
    for center, rate in REQS:  # (with and without a second stage)
        code, resp, cid = s.request(xl.wire_build_request(center, rate, BAND_FREQ, 0))
        assert code == 1 and resp == xl.wire_build_response(1, 3) and s.engine().num_clients == 0
    code, resp, cid = s.request(xl.wire_build_request(REQS[1][0], 48000, BAND_FREQ, 1), socket_fd=-1)  # SOCKET without a socket
    assert code == 1 and resp == xl.wire_build_response(1, 3) and s.engine().num_clients == 0
    s.blocks_host(blocks()[0])  # (no clients: nothing to do)
    assert s.last_ops() == (0, 0, 0)
    s.close()
    # ... and the counts of a call without clients are that call's, not the one's before it
    s = xl.Serve(BAND_RATE, "cu8", BUFFER, tmp_path, family="cf32", native=True, any_rate=True)
    code, resp, a = s.request(msg)
    assert code == 0
    s.blocks_host(blocks()[0])
    assert s.last_ops()[:2] == (1, 2) and s.last_ops()[2] > 0
    s.remove(a)
    s.blocks_host(blocks()[1])
    assert s.last_ops() == (0, 0, 0)
    s.close()


# ------------------------------------------------------------------------------------------------------------ sockets
class Reader(threading.Thread):
    """reads a socket until `want` bytes have come or the peer closes"""

    def __init__(self, sock, want):
        super().__init__(daemon=True)
        self.sock, self.want, self.data = sock, want, bytearray()
        self.sock.settimeout(20)
        self.start()

    def run(self):
        try:
            while len(self.data) < self.want:
                part = self.sock.recv(1 << 16)
                if not part:
                    break
                self.data += part
        except OSError:
            pass


@pytest.mark.parametrize("family", ["cf32", "cs16"])
def test_socket_peer_reads_the_exact_stream(family, tmp_path):
    hand, _ = by_hand(family)
    s = xl.Serve(BAND_RATE, "cu8", BUFFER, tmp_path, family=family, native=True, any_rate=True, overlap=True, queue_bytes=1 << 20)
    pairs, readers = {}, {}
    for center, rate in REQS:
        a, b = socket.socketpair()
        code, resp, cid = s.request(xl.wire_build_request(center, rate, BAND_FREQ, 1), socket_fd=a.fileno())
        assert code == 0
        pairs[rate], readers[rate] = (a, b), Reader(b, len(hand[rate]))
    for b in blocks():
        s.blocks_host(b)
    s.flush()
    for rate, r in readers.items():
        r.join(30)
        assert not r.is_alive() and bytes(r.data) == hand[rate], rate
    assert s.dropped() == [] and os.listdir(tmp_path) == []
    s.close()
    for a, b in pairs.values():
        assert a.fileno() >= 0  # (the descriptors stay the caller's)
        a.close(), b.close()


def test_peer_that_never_reads_is_dropped_and_nobody_else_loses_a_byte(tmp_path):
    """queue_bytes = 1 MiB.  The stalled socket's client (48000 Hz: 64 KiB a call) overflows its queue after about twenty calls: it is
    removed from the engine and reported once.  The other client (12000 Hz: 16 KiB a call, 528 KiB over the 33 calls, which its queue
    holds whatever its writer does) keeps every byte: its file is the oracle's stream over all the calls"""
    s = xl.Serve(BAND_RATE, "cu8", BUFFER, tmp_path, family="cf32", native=True, any_rate=True, queue_bytes=1 << 20)
    a, b = socket.socketpair()
    a.setsockopt(socket.SOL_SOCKET, socket.SO_SNDBUF, 4096)
    code, _, stalled = s.request(xl.wire_build_request(REQS[1][0], 48000, BAND_FREQ, 1), socket_fd=a.fileno())
    assert code == 0
    code, _, good = s.request(xl.wire_build_request(REQS[0][0], 12000, BAND_FREQ, 0))
    assert code == 0
    full = blocks()[:11]
    seen = []
    for rep in range(3):
        for blk in full:
            s.blocks_host(blk)
            seen += s.dropped()
    assert seen == [stalled] and s.engine().num_clients == 1
    s.flush()
    assert s.dropped() == []
    s.close()
    assert open(tmp_path / f"{good}.cf32", "rb").read() == oracle_stream("cf32", REQS[0][0], 3, 0, 11, 12000)
    a.close(), b.close()


def test_dropped_clients_id_is_reused_and_the_newcomer_starts_with_its_first_block(tmp_path):
    """overlap = 1: a client is dropped (its peer never reads, its queue overflows) while the latest call's ticket still holds a row
    under its id; the engine gives that id to the next request.  The newcomer's file is the oracle's stream from the first block after
    its request: nothing of the old client's row reaches it"""
    s = xl.Serve(BAND_RATE, "cu8", BUFFER, tmp_path, family="cf32", native=True, any_rate=True, overlap=True, queue_bytes=1 << 20)
    a, b = socket.socketpair()
    a.setsockopt(socket.SOL_SOCKET, socket.SO_SNDBUF, 4096)
    code, _, old = s.request(xl.wire_build_request(REQS[1][0], 48000, BAND_FREQ, 1), socket_fd=a.fileno())
    assert code == 0
    full = blocks()[:11]
    k, gone = 0, []
    while not gone and k < 60:  # (64 KiB a call into a queue of 1 MiB that nobody drains)
        s.blocks_host(full[k % 11])
        k += 1
        gone = s.dropped()
    assert gone == [old] and s.engine().num_clients == 0
    code, _, new = s.request(xl.wire_build_request(REQS[0][0], 48000, BAND_FREQ, 0))  # another centre: another stream
    assert code == 0 and new == old
    fed = [full[(k + i) % 11] for i in range(3)]
    for blk in fed:
        s.blocks_host(blk)
    s.flush()
    assert s.dropped() == []
    s.close()
    req, adm, L, M, _ = admission(REQS[0][0], 48000)
    code, taps = xl.create_low_pass_filter(1.0, BAND_RATE, adm.lpf_cutoff, adm.lpf_transition)
    o = Oracle(adm.decimation, taps, adm.center_offset, BAND_RATE, BUFFER)
    want = np.concatenate([o.process("cu8", blk) for blk in fed]).tobytes()
    o.close()
    assert open(tmp_path / f"{new}.cf32", "rb").read() == want
    a.close(), b.close()


def test_join_and_leave_between_calls_with_overlap(tmp_path):
    """overlap = 1: the leaver is still owed its last block when it leaves, and gets it; the newcomer's stream starts with the first
    block after its request"""
    s = xl.Serve(BAND_RATE, "cu8", BUFFER, tmp_path, family="cf32", native=True, any_rate=True, overlap=True)
    want_a = oracle_stream("cf32", REQS[1][0], 1, 0, 3)
    want_b = oracle_stream("cf32", REQS[0][0], 1, 3, 5)
    sa, sb = socket.socketpair()
    code, _, a = s.request(xl.wire_build_request(REQS[1][0], 48000, BAND_FREQ, 1), socket_fd=sa.fileno())
    assert code == 0
    ra = Reader(sb, len(want_a))
    bl = blocks()
    for blk in bl[:3]:
        s.blocks_host(blk)
    code, _, b = s.request(xl.wire_build_request(REQS[0][0], 48000, BAND_FREQ, 0))  # joins ...
    assert code == 0
    s.remove(a)  # ... and leaves, between two calls
    for blk in bl[3:5]:
        s.blocks_host(blk)
    s.flush()
    s.close()
    ra.join(30)
    assert not ra.is_alive() and bytes(ra.data) == want_a
    assert open(tmp_path / f"{b}.cf32", "rb").read() == want_b
    sa.close(), sb.close()


# ------------------------------------------------------------------------------------------------------------ the tool and the C demo
def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", f"{name}.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_serve_iq_writes_replay_iqs_files(tmp_path):
    replay_iq, serve_iq = _tool("replay_iq"), _tool("serve_iq")
    path = tmp_path / "capture.cu8"
    capture().tofile(path)
    W = 64
    args = (str(path), "cu8", BAND_RATE, BAND_FREQ, REQS)
    adm, rej, st = replay_iq.replay(*args, str(tmp_path / "r"), BUFFER, 5, "native", waterfall_width=W, any_rate=True)
    adm2, rej2, st2 = serve_iq.replay(*args, str(tmp_path / "s"), BUFFER, 5, "native", waterfall_width=W, any_rate=True)
    assert adm2 == adm and rej2 == rej == [] and st2 == st
    assert sorted(os.listdir(tmp_path / "s")) == sorted(os.listdir(tmp_path / "r"))
    for name in os.listdir(tmp_path / "r"):  # (the .cf32 files and the waterfalls)
        assert open(tmp_path / "s" / name, "rb").read() == open(tmp_path / "r" / name, "rb").read(), name
    # q15 with gzip, which replay_iq refuses: the files decompress to replay_iq's raw .cs16
    adm, rej, st = replay_iq.replay(*args, str(tmp_path / "rq"), BUFFER, 5, "q15", any_rate=True)
    a = serve_iq.parse_args([str(path), "--band-freq", str(BAND_FREQ), "--out", str(tmp_path / "sq"), "--variant", "q15", "--gzip"])
    assert a.gzip and a.variant == "q15"
    adm2, rej2, st2 = serve_iq.replay(*args, str(tmp_path / "sq"), BUFFER, 5, "q15", gzip=True, any_rate=True, overlap=True)
    assert adm2 == adm and rej2 == rej and st2 == st
    for cid in adm:
        assert gzip.open(tmp_path / "sq" / f"{cid}.cs16.gz", "rb").read() == open(tmp_path / "rq" / f"{cid}.cs16", "rb").read()
    # without --any-rate the fractional request is refused as by replay_iq
    adm, rej, st = serve_iq.replay(*args, str(tmp_path / "plain"), BUFFER, 5, "native")
    assert sorted(adm.values()) == [REQS[1]] and rej == [(REQS[0][0], REQS[0][1], 1)]


@pytest.mark.parametrize("family,overlap", [("cf32", ""), ("cs16", "overlap")])
def test_c_demo_builds_and_runs(family, overlap, tmp_path):
    libdir = os.path.dirname(xl.serve_library_path())
    demo = str(tmp_path / "serve_demo")
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "serve_demo.c"),
                        "-o", demo, "-L", libdir, "-lxlating_serve", "-lxlating_resample", "-lxlating_hip", f"-Wl,-rpath,{libdir}"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = tmp_path / "out"
    out.mkdir()
    r = subprocess.run([demo, str(out), family] + ([overlap] if overlap else []), capture_output=True, text=True, timeout=120)
    lines = r.stdout.split("\n")
    assert r.returncode == 0 and lines[2] == "0", (r.stdout, r.stderr[-2000:])
    esz = 4 if family == "cs16" else 8
    assert [int(v.split()[1]) for v in lines[:2]] == [49152 * esz, 45159 * esz]
