"""GPU tests of the delivery object (include/xlating_delivery.h): every delivered row is np.array_equal to its source -- no tolerance, the
object moves bytes -- over the layout sweep of tests/c/delivery_plan_sweep.c run on the device (row sizes 0 .. 80 bytes in steps of 4 at
source residues 0, 4, 8, 12 mod 16; rows of chunk - 4, chunk, chunk + 4 and 2 chunk + 4 bytes; empty rows first, last and in runs;
n = 1, 2 and 1025; rows cut from several allocations); the operation counts; the slots; a source overwritten on the same stream right
behind the pack; and a batch beside a running engine call on another stream."""
import errno

import numpy as np
import pytest
import torch

import sdr_server_amd as xl
import siggen

pytestmark = pytest.mark.gpu


class Pool:
    """seeded byte tensors on the device (several allocations) and their host copies; rows are cut from them in turn, each at the
    residue mod 16 asked for"""

    def __init__(self, seed, nalloc=4, size=1 << 20):
        g = torch.Generator().manual_seed(seed)
        self.host = [torch.randint(0, 256, (size,), dtype=torch.uint8, generator=g) for _ in range(nalloc)]
        self.dev = [h.cuda() for h in self.host]
        assert all(d.data_ptr() % 16 == 0 for d in self.dev)
        self.cur = [0] * nalloc
        self.turn = 0

    def cut(self, nbytes, residue):
        """-> (device address, host uint8 array of the row)"""
        for _ in range(len(self.dev)):
            a = self.turn
            self.turn = (self.turn + 1) % len(self.dev)
            at = (self.cur[a] + 15) // 16 * 16 + residue
            if at + nbytes <= self.dev[a].numel():
                self.cur[a] = at + nbytes
                return self.dev[a].data_ptr() + at, self.host[a][at:at + nbytes].numpy()
        raise AssertionError("pool exhausted")


def deliver_and_check(d, pool, specs, stream=0):
    """specs: [(bytes, residue)] -> one batch, every row compared; returns last_ops"""
    rows = [pool.cut(n, r) for n, r in specs]
    keys = [7 + 3 * i for i in range(len(rows))]
    t = d.pack(keys, [p for p, _ in rows], [h.size for _, h in rows], stream)
    ops = d.last_ops()
    d.wait(t)
    assert d.query(t) is True
    for k, (p, h), (n, r) in zip(keys, rows, specs):
        got = d.row(t, k)
        assert got.size == n and np.array_equal(got, h), (k, n, r)
    d.release(t)
    pad = sum(1 for n, _ in specs if n)
    assert ops[2] >= sum(n for n, _ in specs) and ops[2] <= sum(n for n, _ in specs) + 12 * pad
    return ops


def test_layout_sweep_on_the_device():
    CHUNK = xl.delivery_chunk_bytes()
    assert CHUNK >= 1024 and CHUNK % 16 == 0
    d = xl.Delivery(2)
    pool = Pool(1)
    small = [(n, r) for n in range(0, 84, 4) for r in (0, 4, 8, 12)]
    edges = [(n, r) for n in (CHUNK - 4, CHUNK, CHUNK + 4, 2 * CHUNK + 4) for r in (0, 4, 8, 12)]
    # every size alone (n = 1), neighbours in pairs (n = 2)
    for spec in small[4:12] + edges[:4]:
        assert deliver_and_check(d, pool, [spec])[:2] == (1, 2)
    for a, b in zip(small[::5], edges + small[1::7]):
        deliver_and_check(d, pool, [a, b])
        deliver_and_check(d, pool, [b, a])
    # all of them in one batch, in three orders; empty rows first, last and in a run in the middle
    deliver_and_check(d, pool, small + edges)
    deliver_and_check(d, pool, edges + small[::-1])
    mixed = [(0, 0), (0, 4)] + [s for pair in zip(small[4:20], edges) for s in pair] + [(0, 8)] * 5 + small[20:] + [(0, 12), (0, 0)]
    deliver_and_check(d, pool, mixed)
    # n = 1025: short rows of every kind, so that many share 16-byte slots and chunks begin inside and between rows
    rng = np.random.default_rng(3)
    pool = Pool(2)
    many = [(int(4 * rng.integers(0, 21)), int(4 * rng.integers(0, 4))) for _ in range(1025)]
    many[0], many[-1], many[500] = (0, 0), (0, 4), (CHUNK + 4, 12)
    assert deliver_and_check(d, pool, many)[:2] == (1, 2)
    tiny = [(4 if i % 3 else 0, 4 * (i % 4)) for i in range(1025)]
    deliver_and_check(d, pool, tiny)
    d.close()


def test_last_ops_counts():
    d = xl.Delivery(2)
    pool = Pool(4)
    # n = 1: the row and its residue, nothing else
    ptr, host = pool.cut(4 * 1001, 8)
    t = d.pack([5], [ptr], [host.size])
    assert d.last_ops() == (1, 2, 8 + 4 * 1001)
    d.wait(t)
    assert np.array_equal(d.row(t, 5), host)
    d.release(t)
    # n = 1025 rows of 40 bytes, all at residue 0: 8 bytes of padding between neighbours
    rows = [pool.cut(40, 0) for _ in range(1025)]
    t = d.pack(list(range(1025)), [p for p, _ in rows], [40] * 1025)
    assert d.last_ops() == (1, 2, 1025 * 40 + 1024 * 8)
    d.wait(t)
    assert all(np.array_equal(d.row(t, k), h) for k, (_, h) in enumerate(rows))
    d.release(t)
    # empty batches: no rows, and rows without bytes
    for keys, ptrs, nb in (([], [], []), ([1, 2], [0, ptr], [0, 0])):
        t = d.pack(keys, ptrs, nb)
        assert d.last_ops() == (0, 0, 0) and d.query(t) is True
        for k in keys:
            assert d.row(t, k).size == 0
        d.release(t)
    # refusals leave the counts and the slots alone
    t = d.pack([5], [ptr], [host.size])
    before = d.last_ops()
    for keys, ptrs, nb in (([1, 1], [ptr, ptr], [4, 4]), ([1], [ptr + 2], [4]), ([1], [ptr], [6]), ([1], [0], [4])):
        with pytest.raises(xl.XlatingError) as e:
            d.pack(keys, ptrs, nb)
        assert e.value.code == -errno.EINVAL
    assert d.last_ops() == before
    with pytest.raises(xl.XlatingError):
        d.row(t, 6)  # no such key
    d.wait(t)
    d.release(t)
    with pytest.raises(xl.XlatingError):
        d.release(t)  # no such ticket any more
    d.close()


def test_two_slots_five_batches_and_eagain():
    d = xl.Delivery(2)
    pool = Pool(5)
    batches = [[pool.cut(4 * (100 + 7 * b + i), 4 * (i % 4)) for i in range(9)] for b in range(5)]

    def pack(b):
        return d.pack(list(range(9)), [p for p, _ in batches[b]], [h.size for _, h in batches[b]])

    def check(t, b):
        d.wait(t)
        for k, (_, h) in enumerate(batches[b]):
            assert np.array_equal(d.row(t, k), h), (b, k)

    t0, t1 = pack(0), pack(1)
    assert t1 != t0
    ops = d.last_ops()
    with pytest.raises(xl.XlatingError) as e:  # two tickets unreleased: nothing is consumed
        pack(2)
    assert e.value.code == -errno.EAGAIN and d.last_ops() == ops
    check(t0, 0), check(t1, 1)
    d.release(t0)  # in order
    t2 = pack(2)
    with pytest.raises(xl.XlatingError) as e:
        pack(3)
    assert e.value.code == -errno.EAGAIN
    check(t1, 1)  # (untouched by the batch that took the other slot)
    check(t2, 2)
    d.release(t2)  # out of order: the younger first
    t3 = pack(3)
    check(t3, 3), check(t1, 1)
    d.release(t1)
    t4 = pack(4)
    check(t4, 4), check(t3, 3)
    d.release(t4), d.release(t3)
    assert len({t0, t1, t2, t3, t4}) == 5
    d.close()


def test_sources_may_be_overwritten_right_behind_the_pack():
    d = xl.Delivery(2)
    g = torch.Generator().manual_seed(6)
    host = torch.randint(0, 256, (24 << 20,), dtype=torch.uint8, generator=g)
    dev = host.cuda()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    cuts = [(0, 8 << 20), ((8 << 20) + 4, (8 << 20) - 4), ((16 << 20) + 8, (8 << 20) - 8)]
    t = d.pack([0, 1, 2], [dev.data_ptr() + a for a, _ in cuts], [n for _, n in cuts], s.cuda_stream)
    with torch.cuda.stream(s):
        dev.fill_(0xAA)  # enqueued behind the pack launch, long before the copy to the host is through
    d.wait(t)
    for k, (a, n) in enumerate(cuts):
        assert np.array_equal(d.row(t, k), host[a:a + n].numpy()), k
    s.synchronize()
    assert int(dev[12345]) == 0xAA
    d.release(t)
    d.close()


def test_beside_a_running_engine_call():
    """a batch on one stream while an engine call (native: the same numbers in any company) runs on another: both bit for bit what they
    are alone"""
    code, taps = xl.create_low_pass_filter(1.0, 2016000, 24000, 9600)
    assert code == 0
    x = siggen.xs_u8(siggen.XS_SEED + 40, 4 * 262144)
    dx = torch.from_numpy(x).cuda()
    fcs = [-400000 + 9000 * c for c in range(96)]

    def run(beside):
        eng = xl.BatchEngine(2016000, "cu8", 262144, group_blocks=4)
        ids = [eng.add_client(42, taps, fc) for fc in fcs]
        sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
        torch.cuda.synchronize()
        d = xl.Delivery(2)
        pool = Pool(7, nalloc=3, size=8 << 20)
        rows = [pool.cut(4 * (50000 + 11 * i), 4 * (i % 4)) for i in range(60)]
        torch.cuda.synchronize()
        outs = []
        for call in range(2):
            eng.process_device_group(dx.data_ptr(), 262144, 4, "native", sa.cuda_stream)
            if beside:
                t = d.pack(list(range(60)), [p for p, _ in rows], [h.size for _, h in rows], sb.cuda_stream)
                d.wait(t)
                for k, (_, h) in enumerate(rows):
                    assert np.array_equal(d.row(t, k), h), (call, k)
                d.release(t)
            eng.fetch()
            outs.append(np.concatenate([eng.output(c) for c in ids]))
        d.close()
        eng.close()
        return outs

    alone, beside = run(False), run(True)
    for a, b in zip(alone, beside):
        assert a.size > 0 and np.array_equal(a.view(np.uint32), b.view(np.uint32))
