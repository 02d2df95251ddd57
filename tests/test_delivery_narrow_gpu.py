"""GPU tests of the narrowing delivery (xlating_delivery_pack_device_cs16) and of the serve family built on it (XL_SERVE_CF32_AS_CS16).
The kernel against the numpy restatement (tests/delivery_narrow_ref.py, which test_delivery_narrow_cpu.py pins), bit for bit: rows cut
from ONE device buffer at source residues 0, 8, 16 and 24 mod 32, whose contents are the table of exact cases at every position of a
32-byte span and then normal noise at four scales; every delivered byte is compared, the bytes that cross and the operation counts are
checked, and the source buffer is read back unchanged.  Narrowing and plain batches alternating on one object.  Then the serve object in
family 2 on the band of tests/test_serve_gpu.py (whose helpers are imported): every file is the restatement applied to the cf32 family's
stream -- the oracle's for an integer-rate client, a float ResamplerBank's driven by hand for a fractional one -- and on a cf32 band of
BASELINE config 5's shape, which the cs16 family refuses."""
import errno
import gzip
import os
import socket

import numpy as np
import pytest
import torch

import delivery_narrow_ref as NR
import sdr_server_amd as xl
import test_serve_gpu as SG
from pyoracle import Oracle

pytestmark = pytest.mark.gpu

CHUNK_SAMPLES = 4096  # XL_DLV_CHUNK image bytes / 4


def contents():
    """float32: the exact cases, each followed through all eight positions of a 32-byte span (the table is 36 floats and is laid down
    8 times at a stride of 37), twice over, then noise at scales 1e-6, 1e-3, 0.3 and 4.0"""
    table = NR.exact_values().view(np.uint32)
    assert table.size % 8 != 0 and (table.size + 1) % 8 != 0 and np.gcd(table.size + 1, 8) == 1
    span = np.concatenate([np.concatenate([table, np.zeros(1, np.uint32)]) for _ in range(8)])
    rng = np.random.default_rng(21)
    noise = [(s * rng.standard_normal(16384)).astype(np.float32).view(np.uint32) for s in (1e-6, 1e-3, 0.3, 4.0)]
    return np.concatenate([span, span] + noise).view(np.float32)


class Buffer:
    """the one torch buffer the rows are cut from, its host copy, and a cursor"""

    def __init__(self):
        self.host = contents()
        self.dev = torch.from_numpy(self.host.view(np.int32).copy()).cuda()  # (as integers: no float ever touches a signalling NaN)
        assert self.dev.data_ptr() % 32 == 0
        self.cur = 0  # in floats

    def seek(self, at):
        self.cur = at

    def cut(self, n, residue):
        """n complex samples at the next address with (address mod 32) == residue, or with residue None right behind the row before
        -> (device address, host float32 view of the row)"""
        at = self.cur if residue is None else (self.cur + 7) // 8 * 8 + residue // 4
        if at + 2 * n > self.host.size:
            at = (residue or 0) // 4  # (wrap: the rows of a batch may overlap in the source, they are only read)
        assert at + 2 * n <= self.host.size
        self.cur = at + 2 * n
        return self.dev.data_ptr() + 4 * at, self.host[at:at + 2 * n]

    def unchanged(self):
        return np.array_equal(self.dev.cpu().numpy().view(np.uint32), self.host.view(np.uint32))


def image_bytes(ptrs, lens, narrow):
    """the layout of include/xlating_delivery.h restated: the image's size for these rows in this order"""
    end = 0
    for p, n in zip(ptrs, lens):
        if n == 0:
            continue
        at = (end & ~15) + ((p & 31) >> 1 if narrow else p & 15)
        end = (at + 16 if at < end else at) + n * (4 if narrow else 8)
    return end


def deliver_and_check(d, buf, specs):
    """specs: [(complex samples, residue | None)] -> one narrowing batch, every delivered byte compared; returns last_ops"""
    rows = [buf.cut(n, r) for n, r in specs]
    assert all(p % 8 == 0 and (r is None or p % 32 == r) for (p, _), (_, r) in zip(rows, specs))
    keys = [5 + 3 * i for i in range(len(rows))]
    t = d.pack_cs16(keys, [p for p, _ in rows], [n for n, _ in specs])
    ops = d.last_ops()
    d.wait(t)
    for k, (p, h), (n, r) in zip(keys, rows, specs):
        got = d.row(t, k)
        want = np.frombuffer(NR.narrow_bytes(h), np.uint8)
        assert got.size == 4 * n and np.array_equal(got, want), (k, n, r, np.nonzero(got != want)[0][:8])
    d.release(t)
    total, nonempty = sum(n for n, _ in specs), sum(1 for n, _ in specs if n)
    if total:
        assert ops[:2] == (1, 2) and 4 * total <= ops[2] <= 4 * total + 12 * nonempty, ops
        assert ops[2] == image_bytes([p for p, _ in rows], [n for n, _ in specs], True)
    else:
        assert ops == (0, 0, 0)
    return ops


def test_kernel_against_the_restatement_bit_for_bit():
    d, buf = xl.Delivery(2), Buffer()
    lengths, residues = (0, 1, 2, 3, 4, 5, 7, 8, 9), (0, 8, 16, 24)
    nspan = 2 * 8 * (NR.exact_values().size + 1)
    # the exact cases on the head and tail paths: rows of 1 .. 3 samples (never a whole slot), each right behind the one before (so the
    # residues come as they come: all four), walking over the whole table; then rows of every length walking over it again; on the
    # body path: one row that holds the table whole, from every residue
    for first in range(4):
        buf.seek(2 * first)
        deliver_and_check(d, buf, [(1 + i % 3, None) for i in range(nspan // 4)])
    buf.seek(0)
    walk = [(lengths[i % len(lengths)], None) for i in range(90)]
    assert sum(n for n, _ in walk) >= nspan // 2
    deliver_and_check(d, buf, walk)
    for first in range(4):
        buf.seek(2 * first)
        assert deliver_and_check(d, buf, [(nspan // 2 + 8, None)])[2] == 4 * first + 4 * (nspan // 2 + 8)
    # every length at every residue: alone, and all together in two orders (into the noise)
    for n in lengths:
        for r in residues:
            deliver_and_check(d, buf, [(n, r)])
    deliver_and_check(d, buf, [(n, r) for n in lengths for r in residues])
    deliver_and_check(d, buf, [(n, r) for r in residues[::-1] for n in lengths[::-1]])
    # four 1-sample rows sharing one 16-byte slot of the image
    assert deliver_and_check(d, buf, [(1, 0), (1, 8), (1, 16), (1, 24)])[2] == 16
    # rows that end before, on and behind the first chunk's end, from image offset 0, with a short row behind them
    for n in (CHUNK_SAMPLES - 1, CHUNK_SAMPLES, CHUNK_SAMPLES + 1):
        deliver_and_check(d, buf, [(n, 0), (3, 8)])
        deliver_and_check(d, buf, [(n, 0)])
    # a first row whose residue is not 0: the image begins with padding
    assert deliver_and_check(d, buf, [(5, 16), (9, 8)])[2] == 8 + 20 + 8 + 36  # (the second row at the next offset that is 4 mod 16)
    deliver_and_check(d, buf, [(CHUNK_SAMPLES, 24), (2, 0), (CHUNK_SAMPLES + 1, 8)])
    # one row across three chunk ends, at every residue; between short rows
    for r in residues:
        deliver_and_check(d, buf, [(3 * CHUNK_SAMPLES + 5, r)])
    deliver_and_check(d, buf, [(2, 8), (3 * CHUNK_SAMPLES + 5, 16), (0, 0), (7, 24)])
    # refusals: a source that is only 4-byte aligned, a row above the maximum, a key twice; nothing was done
    p, _ = buf.cut(8, 0)
    before = d.last_ops()
    for keys, ptrs, ns in (([1], [p + 4], [2]), ([1], [p], [1 << 30]), ([1, 1], [p, p], [2, 2]), ([1], [0], [2])):
        with pytest.raises(xl.XlatingError) as e:
            d.pack_cs16(keys, ptrs, ns)
        assert e.value.code == -errno.EINVAL
    assert d.last_ops() == before
    t = d.pack_cs16([1, 2], [p + 4, 0], [0, 0])  # (an empty row goes with any pointer)
    assert d.last_ops() == (0, 0, 0) and d.query(t) is True and d.row(t, 1).size == 0
    d.release(t)
    d.close()
    torch.cuda.synchronize()
    assert buf.unchanged()  # the sources are not written


def test_narrowing_and_plain_batches_alternate_on_one_object():
    d, buf = xl.Delivery(2), Buffer()
    specs = [(CHUNK_SAMPLES + 3, 8), (0, 0), (5, 24), (1, 16), (700, 0)]

    def narrowing(keys):
        rows = [buf.cut(n, r) for n, r in specs]
        return d.pack_cs16(keys, [p for p, _ in rows], [n for n, _ in specs]), [NR.narrow_bytes(h) for _, h in rows]

    def plain(keys):
        rows = [buf.cut(n, r) for n, r in specs]
        return d.pack(keys, [p for p, _ in rows], [8 * n for n, _ in specs]), [h.tobytes() for _, h in rows]

    def check(t, keys, want):
        d.wait(t)
        for k, w in zip(keys, want):
            assert d.row(t, k).tobytes() == w, (t, k)

    keys = [3, 1, 4, 15, 9]
    n_samples = sum(n for n, _ in specs)
    t0, w0 = narrowing(keys)
    assert d.last_ops()[:2] == (1, 2) and 4 * n_samples <= d.last_ops()[2] <= 4 * n_samples + 48
    t1, w1 = plain(keys)
    assert d.last_ops()[:2] == (1, 2) and 8 * n_samples <= d.last_ops()[2] <= 8 * n_samples + 48
    ops = d.last_ops()
    with pytest.raises(xl.XlatingError) as e:  # both slots held: nothing is consumed
        narrowing(keys)
    assert e.value.code == -errno.EAGAIN and d.last_ops() == ops
    check(t0, keys, w0), check(t1, keys, w1)
    d.release(t0)
    t2, w2 = narrowing(keys[::-1])
    check(t2, keys[::-1], w2), check(t1, keys, w1)  # (the plain batch in the other slot is untouched)
    d.release(t1)
    t3 = d.pack_cs16([], [], [])  # an empty batch between them
    assert d.last_ops() == (0, 0, 0) and d.query(t3) is True
    check(t2, keys[::-1], w2)
    d.release(t3), d.release(t2)
    assert len({t0, t1, t2, t3}) == 4
    d.close()
    torch.cuda.synchronize()
    assert buf.unchanged()


# ------------------------------------------------------------------------------------------------------------ serve, the cu8 band
def narrowed(stream_bytes):
    return NR.narrow_bytes(np.frombuffer(stream_bytes, np.complex64))


def read_file(tmp, cid, ext, gz):
    path = os.path.join(tmp, f"{cid}.{ext}" + (".gz" if gz else ""))
    return gzip.open(path, "rb").read() if gz else open(path, "rb").read()


JOIN_AT = 4  # blocks before the join and the leave: a call boundary with one block a call and with two


@pytest.mark.parametrize("group,overlap,gz", [(1, False, False), (1, True, True), (2, False, True), (2, True, False)])
def test_serve_family_2_on_the_cu8_band(group, overlap, gz, tmp_path):
    """native, any_rate: an integer-rate and a fractional FILE client and a SOCKET client from the start, a FILE client that leaves and
    one that joins after JOIN_AT blocks"""
    tmp = str(tmp_path)
    (c44, r44), (c48, r48) = SG.REQS
    s = xl.Serve(SG.BAND_RATE, "cu8", SG.BUFFER, tmp, family="cf32-cs16", native=True, any_rate=True, gzip=gz, overlap=overlap,
                 group_blocks=group, queue_bytes=1 << 20)

    def join(center, rate, dest=0, fd=-1):
        code, resp, cid = s.request(xl.wire_build_request(center, rate, SG.BAND_FREQ, dest), socket_fd=fd)
        assert code == 0 and resp == xl.wire_build_response(0, cid)
        return cid

    want = {"int": narrowed(SG.oracle_stream("cf32", c48)), "frac": narrowed(SG.by_hand("cf32")[0][r44]),
            "leaver": narrowed(SG.oracle_stream("cf32", c44, 1, 0, JOIN_AT, 12000)),
            "joiner": narrowed(SG.oracle_stream("cf32", c44, 1, JOIN_AT, None))}
    ids = {"int": join(c48, r48), "frac": join(c44, r44), "leaver": join(c44, 12000)}
    sa, sb = socket.socketpair()
    ids["sock"] = join(c48, r48, 1, sa.fileno())
    reader = SG.Reader(sb, len(want["int"]))
    blocks_done, samples = 0, {k: 0 for k in ("int", "frac", "leaver", "joiner")}
    for x, n in SG.calls(group):
        if blocks_done == JOIN_AT:
            ids["joiner"] = join(c44, r48)
            left = ids.pop("leaver")
            s.remove(left)
        s.blocks_host(x, n)
        blocks_done += n
        names = sorted((k for k in ids), key=lambda k: ids[k])  # (the batch's order: by client id)
        launches, copies, d2h = s.last_ops()
        ptrs, lens = s.outputs_device([ids[k] for k in names])
        assert (launches, copies) == (3, 3)  # the bank's feed and carry + ONE pack; two tables up, the rows down
        assert d2h == image_bytes(ptrs.tolist(), lens.tolist(), True) and 4 * int(lens.sum()) <= d2h <= 4 * int(lens.sum()) + 12 * len(lens)
        assert d2h <= image_bytes(ptrs.tolist(), lens.tolist(), False) // 2 + 12 * len(lens)  # half of what the cf32 family moves for these rows
        for k, n_out in zip(names, lens.tolist()):
            if k in samples:
                samples[k] += n_out
    s.flush()
    assert s.dropped() == []
    s.close()
    reader.join(30)
    assert not reader.is_alive() and bytes(reader.data) == want["int"]
    sa.close(), sb.close()
    files = {k: read_file(tmp, cid, "cs16", gz) for k, cid in ids.items() if k != "sock"}
    files["leaver"] = read_file(tmp, left, "cs16", gz)  # (closed with what it was owed when it left)
    assert files["int"] == want["int"] and files["frac"] == want["frac"] and files["joiner"] == want["joiner"]
    assert files["leaver"] == want["leaver"] and len(os.listdir(tmp)) == 4
    for k, data in files.items():
        assert len(data) == 4 * samples[k] > 0, k  # 4 bytes a sample
    assert all(f.endswith(".cs16.gz" if gz else ".cs16") for f in os.listdir(tmp))


def test_family_0_beside_family_2_is_unchanged(tmp_path):
    """the two families on the same requests and blocks, their calls alternating in one process: family 0 writes the cf32 bytes it wrote
    before (the oracle's stream, the hand-driven bank's), family 2 their restatement"""
    (c44, r44), (c48, r48) = SG.REQS
    serves, ids = {}, {}
    for family in ("cf32", "cf32-cs16"):
        os.makedirs(tmp_path / family)
        serves[family] = xl.Serve(SG.BAND_RATE, "cu8", SG.BUFFER, str(tmp_path / family), family=family, native=True, any_rate=True,
                                  overlap=True, queue_bytes=1 << 20)
        for center, rate in SG.REQS:
            code, _, cid = serves[family].request(xl.wire_build_request(center, rate, SG.BAND_FREQ, 0))
            assert code == 0
            ids[family, rate] = cid
    d2h = {f: 0 for f in serves}
    for b in SG.blocks():
        for family, s in serves.items():
            s.blocks_host(b)
            assert s.last_ops()[:2] == (3, 3)
            d2h[family] += s.last_ops()[2]
    for s in serves.values():
        s.flush()
        assert s.dropped() == []
        s.close()
    hand = SG.by_hand("cf32")[0]
    f0 = {rate: open(tmp_path / "cf32" / f"{ids['cf32', rate]}.cf32", "rb").read() for _, rate in SG.REQS}
    f2 = {rate: open(tmp_path / "cf32-cs16" / f"{ids['cf32-cs16', rate]}.cs16", "rb").read() for _, rate in SG.REQS}
    assert f0[r48] == SG.oracle_stream("cf32", c48) == hand[r48] and f0[r44] == hand[r44]
    assert f2[r48] == narrowed(f0[r48]) and f2[r44] == narrowed(f0[r44])
    assert 2 * len(f2[r48]) == len(f0[r48]) and 2 * len(f2[r44]) == len(f0[r44])
    assert d2h["cf32-cs16"] <= d2h["cf32"] // 2 + 24 * len(SG.blocks())


# ------------------------------------------------------------------------------------------------------------ serve, a cf32 band
CF32_RATE, CF32_BUFFER, CF32_D = 10000000, 65536, 100


def cf32_band(nblocks):
    """cf32 at 10 Msps: tones of unequal amplitudes around the clients' centres and noise, peaks near 0.9"""
    n = nblocks * CF32_BUFFER // 2
    rng = np.random.default_rng(31)
    t = np.arange(n, dtype=np.float64) / CF32_RATE
    z = sum(a * np.exp(2j * np.pi * f * t) for a, f in ((0.35, 1010000.0), (0.2, -2495000.0), (0.15, 3000.0), (0.1, 4205000.0)))
    z = z + 0.03 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    return np.stack([z.real, z.imag], axis=1).reshape(-1).astype(np.float32)


@pytest.mark.parametrize("native", [True, False])
def test_serve_family_2_on_a_cf32_band(native, tmp_path):
    """BASELINE config 5's shape (cf32 input at 10 Msps, clients at 100 kHz: D = 100), which the cs16 family cannot serve.  The serve
    object designs its own filter: lpf_cutoff_rate = 1 gives 241 taps, the nearest it gets to that configuration's 257.  Native: the
    narrowed oracle bit for bit.  Optimized: within 1 LSB plus the restatement of the 1e-5 bound the cf32 family holds against the
    oracle, ceil(1e-5 * max|y| * 32768) + 1 LSBs"""
    with pytest.raises(xl.XlatingError) as e:
        xl.Serve(CF32_RATE, "cf32", CF32_BUFFER, str(tmp_path), family="cs16", any_rate=True, lpf_cutoff_rate=1)
    assert e.value.code == -errno.EINVAL
    s = xl.Serve(CF32_RATE, "cf32", CF32_BUFFER, str(tmp_path), family="cf32-cs16", native=native, any_rate=True, lpf_cutoff_rate=1,
                 queue_bytes=1 << 20)
    nblocks = 4
    x = cf32_band(nblocks)
    centers = [SG.BAND_FREQ + f for f in (1000000, -2500000, 0, 4200000, -4800000)]
    ids, oracles = {}, {}
    for c in centers:
        code, _, cid = s.request(xl.wire_build_request(c, CF32_RATE // CF32_D, SG.BAND_FREQ, 0))
        assert code == 0
        ids[c] = cid
        code, adm, rs, why = xl.wire_admit_any_rate(xl.WireRequest(c, CF32_RATE // CF32_D, SG.BAND_FREQ, 0), CF32_RATE, 0, 1)
        assert code == 0 and adm.decimation == CF32_D and (rs.L, rs.M) == (1, 1)
        code, taps = xl.create_low_pass_filter(1.0, CF32_RATE, adm.lpf_cutoff, adm.lpf_transition)
        assert code == 0 and taps.size == 241
        oracles[c] = Oracle(adm.decimation, taps, adm.center_offset, CF32_RATE, CF32_BUFFER)
    want = {c: [] for c in centers}
    for b in np.split(x, nblocks):
        s.blocks_host(b)
        launches, copies, d2h = s.last_ops()
        ptrs, lens = s.outputs_device(sorted(ids.values()))
        assert (launches, copies) == (1, 2) and d2h == image_bytes(ptrs.tolist(), lens.tolist(), True)
        for c in centers:
            want[c].append(oracles[c].process("cf32", b))
    s.flush()
    assert s.dropped() == []
    s.close()
    for c in centers:
        oracles[c].close()
        y = np.concatenate(want[c])
        got = np.frombuffer(open(tmp_path / f"{ids[c]}.cs16", "rb").read(), np.int16)
        ref = NR.narrow(y)
        assert got.size == ref.size == 2 * y.size and abs(y.size - nblocks * CF32_BUFFER // 2 // CF32_D) <= 1
        if native:
            assert np.array_equal(got, ref), c
        else:
            bound = int(np.ceil(1e-5 * float(np.abs(y).max()) * 32768.0)) + 1
            worst = int(np.abs(got.astype(np.int32) - ref.astype(np.int32)).max())
            print(f"center {c}: max|y| {np.abs(y).max():.4f}, largest difference {worst} LSB, bound {bound} LSB")
            assert worst <= bound, (c, worst, bound)
    assert float(np.abs(np.concatenate(want[centers[0]])).max()) > 0.2  # (the streams are not silence)
