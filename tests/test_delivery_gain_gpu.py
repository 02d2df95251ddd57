"""GPU tests of the narrowing delivery with a gain and a level meter (xlating_delivery_pack_device_cs16_gain, xlating_delivery_row_level):
the bytes and the three level values of every row against the numpy restatement (tests/delivery_gain_ref.py, which
test_delivery_gain_cpu.py pins), bit for bit.  Every row's contents are laid into ONE device buffer at a chosen residue of a 32-byte
span, as integers, so that no float operation ever touches a signalling NaN.  The same rows in another order and each alone in a batch
give the same bytes and levels; with every gain 0 the rows are pack_device_cs16's; the sources are unwritten; the operation counts and
bytes are the header's; the three pack calls alternate on one object."""
import errno

import numpy as np
import pytest
import torch

import delivery_gain_ref as GR
import delivery_narrow_ref as NR
import sdr_server_amd as xl

pytestmark = pytest.mark.gpu

CHUNK_SAMPLES = 4096  # XL_DLV_CHUNK image bytes / 4
NAN, SNAN, INF, NINF = 0x7FC00000, 0xFF800001, 0x7F800000, 0xFF800000


class Rows:
    """rows of explicit contents in one device buffer.  add(bits, residue): uint32 words (two a sample) at the next address with
    (address mod 32) == residue, or with residue None right behind the row before"""

    def __init__(self):
        self.words, self.at, self.n = [], [], []
        self.cur = 0  # in words

    def add(self, bits, residue=None):
        bits = np.ascontiguousarray(bits, dtype=np.uint32).reshape(-1)
        assert bits.size % 2 == 0
        at = self.cur if residue is None else (self.cur + 7) // 8 * 8 + residue // 4
        self.words.append((at, bits))
        self.at.append(at), self.n.append(bits.size // 2)
        self.cur = at + bits.size
        return len(self.n) - 1

    def upload(self):
        self.host = np.zeros(self.cur + 8, np.uint32)
        for at, bits in self.words:
            self.host[at:at + bits.size] = bits
        self.dev = torch.from_numpy(self.host.view(np.int32).copy()).cuda()
        assert self.dev.data_ptr() % 32 == 0
        self.ptr = [self.dev.data_ptr() + 4 * at for at in self.at]
        self.f32 = [self.host[at:at + 2 * n].view(np.float32) for at, n in zip(self.at, self.n)]
        return self

    def unchanged(self):
        torch.cuda.synchronize()
        return np.array_equal(self.dev.cpu().numpy().view(np.uint32), self.host)


def image_bytes(ptrs, lens):
    """the narrowed layout of include/xlating_delivery.h restated: the image's size for these rows in this order"""
    end = 0
    for p, n in zip(ptrs, lens):
        if n == 0:
            continue
        at = (end & ~15) + ((p & 31) >> 1)
        end = (at + 16 if at < end else at) + 4 * n
    return end


def stated_bytes(ptrs, lens):
    """what the header says crosses: the image rounded up to 16 and 12 bytes a non-empty row"""
    rows = sum(1 for n in lens if n)
    return (image_bytes(ptrs, lens) + 15) // 16 * 16 + 12 * rows if rows else 0


def deliver(d, R, which, gains):
    """one batch of the rows `which` of R (in that order) under `gains` -> {row: (bytes, level)}; the operation counts are checked"""
    keys = [7 + 2 * i for i in which]
    ptrs, lens = [R.ptr[i] for i in which], [R.n[i] for i in which]
    t = d.pack_device_cs16_gain(keys, ptrs, lens, gains)
    ops = d.last_ops()
    assert ops == ((1, 3, stated_bytes(ptrs, lens)) if sum(lens) else (0, 0, 0)), (ops, stated_bytes(ptrs, lens))
    d.wait(t)
    out = {i: (d.row(t, k).tobytes(), d.row_level(t, k)) for i, k in zip(which, keys)}
    d.release(t)
    return out


def check(R, which, gains, got):
    for i, g in zip(which, gains):
        data, lvl = got[i]
        want = GR.narrow_bytes(R.f32[i], g)
        assert len(data) == 4 * R.n[i] and data == want, (i, R.n[i], g, np.nonzero(np.frombuffer(data, np.int16) != np.frombuffer(want, np.int16))[0][:8])
        assert lvl == GR.level(R.f32[i], g), (i, R.n[i], g, lvl, GR.level(R.f32[i], g))


def scaled_bits(rng, n_words, g):
    """random floats that exercise gain g: the exponent field drawn from the fields around the rule's edges for that gain (e + g in
    100 .. 135), fractions and signs at random"""
    e = (rng.integers(100, 136, n_words) - g).clip(0, 255).astype(np.uint32)
    return (rng.integers(0, 2, n_words).astype(np.uint32) << 31) | (e << 23) | rng.integers(0, 1 << 23, n_words).astype(np.uint32)


@pytest.fixture(scope="module")
def main_rows():
    """the rows of the issue's list, their gains, and the reference delivery: one batch in the order given"""
    rng = np.random.default_rng(77)
    R, gains = Rows(), []
    cycle = [-48, -9, -1, 0, 1, 9, 48, 17, -30]
    # every length at every residue: random bit patterns over ALL exponents for the short rows, patterns around the rule's edges for
    # the gain in force in the long ones
    for n in (0, 1, 2, 3, 4, 5, 7, 8, 9, CHUNK_SAMPLES - 1, CHUNK_SAMPLES, CHUNK_SAMPLES + 1, 2 * CHUNK_SAMPLES + 1):
        for r in (0, 8, 16, 24):
            g = cycle[len(gains) % len(cycle)]
            bits = rng.integers(0, 1 << 32, 2 * n, dtype=np.uint64).astype(np.uint32) if n < 100 else scaled_bits(rng, 2 * n, g)
            R.add(bits, r), gains.append(g)
    # 64 one- and two-sample rows back to back in the source, so that they share image slots; neighbouring gains -48 / +48
    for i in range(64):
        g = -48 if i % 2 == 0 else 48
        R.add(scaled_bits(rng, 2 * (1 + (i // 3) % 2), g), None if i else 8), gains.append(g)
    # the exact-case table scaled per row, at every residue, and laid so that each case meets every position of a 32-byte span
    for g in (0,) + GR.PINNED_GAINS:
        table = np.array([b for b, _ in GR.exact_table(g)], np.uint32)
        pad = 1 if table.size % 2 == 0 else 2  # an odd stride: the 8 copies begin at 8 different words of a span
        span = np.concatenate([np.concatenate([table, np.zeros(pad, np.uint32)]) for _ in range(8)])
        assert (table.size + pad) % 2 == 1 and span.size % 2 == 0
        for r in (0, 8, 16, 24):
            R.add(span, r), gains.append(g)
        for k in range(8):  # the table from each of its first 8 words on, in rows of 3 samples and a tail: the partial-slot path
            words = np.concatenate([table[k:], np.zeros((table.size - k) % 2, np.uint32)])
            R.add(words[:6], None if k else 16), gains.append(g)
            R.add(words[6:], None), gains.append(g)
    # NaN and Inf first and last in a row, an all-NaN row, an empty row between full ones
    body = scaled_bits(rng, 40, 0)
    for first, last, r in ((NAN, INF, 0), (INF, SNAN, 8), (NINF, NAN, 16), (SNAN, NINF, 24)):
        row = body.copy()
        row[0], row[-1] = first, last
        R.add(row, r), gains.append(0 if r % 16 == 0 else -3)
    R.add(np.array([NAN, SNAN] * 10, np.uint32), 8), gains.append(5)
    R.add(scaled_bits(rng, 2 * 300, 2), 16), gains.append(2)
    R.add(np.zeros(0, np.uint32), 0), gains.append(-7)
    R.add(scaled_bits(rng, 2 * 300, -2), 24), gains.append(-2)
    R.upload()
    d = xl.Delivery(2)
    which = list(range(len(R.n)))
    ref = deliver(d, R, which, gains)
    d.close()
    return R, gains, ref


def test_bytes_and_levels_of_every_row_against_the_restatement(main_rows):
    R, gains, ref = main_rows
    assert len(R.n) > 200 and {0, 1, 9, CHUNK_SAMPLES, 2 * CHUNK_SAMPLES + 1} <= set(R.n)
    check(R, list(range(len(R.n))), gains, ref)
    # the batch was not trivial: rows that clipped, rows with NaNs, silent rows, and both extreme gains
    levels = [ref[i][1] for i in range(len(R.n))]
    assert sum(1 for l in levels if l[1] > 0) > 20 and sum(1 for l in levels if l[2] > 0) > 10 and {-48, 48} <= set(gains)
    assert R.unchanged()  # the sources are not written


def test_a_row_that_begins_in_the_last_slot_of_a_chunk():
    rng = np.random.default_rng(78)
    for lead, tail in ((CHUNK_SAMPLES - 4, 9), (CHUNK_SAMPLES - 1, 2), (CHUNK_SAMPLES - 3, 1), (2 * CHUNK_SAMPLES - 2, CHUNK_SAMPLES + 3)):
        R = Rows()
        R.add(scaled_bits(rng, 2 * lead, -5), 0)
        R.add(scaled_bits(rng, 2 * tail, 48), (4 * lead % 16) * 2)  # right behind it in the image: inside the chunk's last slot
        R.add(scaled_bits(rng, 2 * 5, -48), 24)
        R.upload()
        assert image_bytes(R.ptr[:2], R.n[:2]) == 4 * (lead + tail) and (4 * lead) // 16 % 1024 == 1023
        d = xl.Delivery(2)
        check(R, [0, 1, 2], [-5, 48, -48], deliver(d, R, [0, 1, 2], [-5, 48, -48]))
        d.close()
        assert R.unchanged()


def test_another_order_and_each_row_alone_give_the_same(main_rows):
    R, gains, ref = main_rows
    d = xl.Delivery(2)
    which = list(range(len(R.n)))
    rng = np.random.default_rng(79)
    for order in (which[::-1], [int(i) for i in rng.permutation(len(which))]):
        assert deliver(d, R, order, [gains[i] for i in order]) == ref
    for i in which:
        assert deliver(d, R, [i], [gains[i]])[i] == ref[i], i
    d.close()
    assert R.unchanged()


def test_every_gain_zero_is_pack_device_cs16(main_rows):
    R, _, _ = main_rows
    d = xl.Delivery(2)
    which = list(range(len(R.n)))
    keys, ptrs = [7 + 2 * i for i in which], [R.ptr[i] for i in which]
    got = deliver(d, R, which, [0] * len(which))
    t = d.pack_cs16(keys, ptrs, R.n)
    launches, copies, plain_bytes = d.last_ops()
    assert (launches, copies) == (1, 2) and plain_bytes == image_bytes(ptrs, R.n)
    d.wait(t)
    for i, k in zip(which, keys):
        assert d.row(t, k).tobytes() == got[i][0] == NR.narrow_bytes(R.f32[i]), i
    with pytest.raises(xl.XlatingError) as e:  # a plain ticket records no levels
        d.row_level(t, keys[0])
    assert e.value.code == -errno.ENODATA
    d.release(t)
    d.close()


def test_the_three_pack_calls_alternate_and_refusals():
    rng = np.random.default_rng(80)
    R = Rows()
    specs = [(CHUNK_SAMPLES + 3, 8), (0, 0), (5, 24), (1, 16), (700, 0)]
    for n, r in specs:
        R.add(scaled_bits(rng, 2 * n, 0), r)
    R.upload()
    keys, lens, gains = [3, 1, 4, 15, 9], [n for n, _ in specs], [3, 0, -48, 48, -1]
    d = xl.Delivery(2)

    def rows(t):
        d.wait(t)
        return [d.row(t, k).tobytes() for k in keys]

    want_gain = [GR.narrow_bytes(f, g) for f, g in zip(R.f32, gains)]
    want_narrow = [NR.narrow_bytes(f) for f in R.f32]
    want_plain = [f.tobytes() for f in R.f32]
    t0 = d.pack_device_cs16_gain(keys, R.ptr, lens, gains)
    assert d.last_ops() == (1, 3, stated_bytes(R.ptr, lens))
    t1 = d.pack(keys, R.ptr, [8 * n for n in lens])
    ops = d.last_ops()
    assert ops[:2] == (1, 2)
    with pytest.raises(xl.XlatingError) as e:  # both slots held: nothing is consumed
        d.pack_device_cs16_gain(keys, R.ptr, lens, gains)
    assert e.value.code == -errno.EAGAIN and d.last_ops() == ops
    assert rows(t0) == want_gain and rows(t1) == want_plain
    for k, f, g in zip(keys, R.f32, gains):
        assert d.row_level(t0, k) == GR.level(f, g)
        with pytest.raises(xl.XlatingError) as e:
            d.row_level(t1, k)
        assert e.value.code == -errno.ENODATA
    with pytest.raises(xl.XlatingError) as e:
        d.row_level(t0, 1000)  # no such key
    assert e.value.code == -errno.EINVAL
    d.release(t0)
    t2 = d.pack_cs16(keys, R.ptr, lens)
    assert d.last_ops() == (1, 2, image_bytes(R.ptr, lens))
    assert rows(t2) == want_narrow and rows(t1) == want_plain
    d.release(t1)
    # refusals: a gain outside -48 .. 48 (an empty row's too), a source at 8k + 4; nothing was done
    before = d.last_ops()
    for bad in ([49, 0, 0, 0, 0], [0, 0, 0, 0, -49], [0, 49, 0, 0, 0], [0, 0, 127, 0, 0], [-128, 0, 0, 0, 0]):
        with pytest.raises(xl.XlatingError) as e:
            d.pack_device_cs16_gain(keys, R.ptr, lens, bad)
        assert e.value.code == -errno.EINVAL
    with pytest.raises(xl.XlatingError) as e:
        d.pack_device_cs16_gain(keys, [R.ptr[0] + 4] + R.ptr[1:], lens, gains)
    assert e.value.code == -errno.EINVAL and d.last_ops() == before
    t3 = d.pack_device_cs16_gain(keys[::-1], R.ptr[::-1], lens[::-1], gains[::-1])  # the slot of t0 again, with gains
    assert rows(t3) == want_gain and rows(t2) == want_narrow
    assert [d.row_level(t3, k) for k in keys] == [GR.level(f, g) for f, g in zip(R.f32, gains)]
    d.release(t2)
    t4 = d.pack_device_cs16_gain([1, 2], [R.ptr[0] + 4, 0], [0, 0], [48, -48])  # an empty batch: done at once, levels of zeros
    assert d.last_ops() == (0, 0, 0) and d.query(t4) is True and d.row(t4, 1).size == 0 and d.row_level(t4, 2) == (0, 0, 0)
    d.release(t4), d.release(t3)
    assert len({t0, t1, t2, t3, t4}) == 5
    d.close()
    assert R.unchanged()
