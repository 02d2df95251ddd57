"""GPU tests (-m gpu) of the tuner bank (include/xlating_tune.h): every output BIT FOR BIT the restatement's (tests/tune_ref.py: Python
integer phases, the library's cs, float32 numpy products in the stated order) -- at the row lengths around a workgroup's piece, at
both alignments, at the state values where the 64-bit arithmetic wraps, under every split of a stream into feeds and in any company;
`set` between feeds; the identity; the accuracy against float64 within the bound derived from the sweep's E; the cost of a feed; the
refusals.  Device rows are read back through the delivery object's plain pack."""
import errno

import numpy as np
import pytest

import sdr_server_amd as xl
import tune_ref as TR
from conftest import bits_equal

pytestmark = pytest.mark.gpu

CH = xl.tune_chunk_samples()
LENGTHS = [0, 1, 2, 3, CH - 1, CH, CH + 1, 2 * CH + 1]


def noise(n, seed):
    rng = np.random.default_rng(seed)
    return (0.5 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64)


def stream():
    import torch

    return torch.cuda.current_stream().cuda_stream


def to_device(rows, odd=None):
    """rows: complex64 arrays -> (tensor kept alive, address of each row): row i starts at an address that is 8 mod 16 where odd[i],
    else 0 mod 16, with poisoned padding between rows"""
    import torch

    odd = odd or [False] * len(rows)
    parts, offs, pos = [], [], 0
    for x, o in zip(rows, odd):
        start = pos + 2  # (in complex samples of 8 bytes: a gap, then the parity asked for)
        start += (start % 2) != (1 if o else 0)
        parts.append(np.full(2 * (start - pos), np.nan, np.float32))
        pos = start
        offs.append(pos)
        parts.append(np.ascontiguousarray(x, np.complex64).view(np.float32))
        pos += x.size
    parts.append(np.full(4, np.nan, np.float32))
    t = torch.from_numpy(np.concatenate(parts)).cuda()
    assert t.data_ptr() % 16 == 0
    addrs = [t.data_ptr() + 8 * o for o in offs]
    for a, o in zip(addrs, odd):
        assert a % 16 == (8 if o else 0)
    return t, addrs


class Reader:
    """reads the bank's latest rows back: one plain delivery pack of them, waited for"""

    def __init__(self):
        self.dlv = xl.Delivery(2)

    def rows(self, bank, sids, counts):
        import torch

        ptrs, ns = [], []
        for sid, c in zip(sids, counts):
            p, n = bank.output_device(sid)
            assert n == c and (p is None) == (n == 0), (sid, n, c)
            assert p is None or p % 8 == 0
            ptrs.append(p or 0), ns.append(n)
        torch.cuda.synchronize()
        t = self.dlv.pack(list(range(len(sids))), ptrs, [8 * n for n in ns], stream())
        self.dlv.wait(t)
        out = [self.dlv.row(t, k).view(np.complex64) for k in range(len(sids))]
        self.dlv.release(t)
        return out

    def close(self):
        self.dlv.close()


@pytest.fixture(scope="module")
def reader():
    r = Reader()
    yield r
    r.close()


def feed_rows(bank, reader, sids, rows, odd=None):
    keep, addrs = to_device(rows, odd)
    before = keep.cpu().numpy().view(np.uint32).copy()
    bank.feed(sids, addrs, [r.size for r in rows], stream())
    out = reader.rows(bank, sids, [r.size for r in rows])
    assert np.array_equal(keep.cpu().numpy().view(np.uint32), before), "the rows are read in place and never written"
    del keep
    return out


def same(got, want, what):
    assert got.size == want.size, (what, got.size, want.size)
    bad = np.nonzero(got.view(np.uint32) != want.view(np.uint32))[0]
    assert bad.size == 0, (what, bad[:8], got.view(np.float32)[bad[:8]], want.view(np.float32)[bad[:8]])


# the states of the issue: F = 0, +-1, 2^62, -2^63; R large enough that phi wraps many times inside a row, and negative; P = 2^64 - 1
STATES = [((1 << 64) - 1, 0, 0), (0, 1, 0), (5, -1, 0), (1 << 63, 1 << 62, 0), ((1 << 64) - 1, -(1 << 63), 0),
          (123456789123456789, 987654321987654321, (1 << 57) + 12345), ((1 << 64) - 1, -(1 << 61) + 1, -(1 << 58) - 777),
          (0, (1 << 63) - 1, (1 << 63) - 1)]


def test_row_lengths_alignments_and_states_in_one_feed(reader):
    """every length around a workgroup's piece, at both alignments, each under another of the state values: one feed, bit for bit"""
    bank = xl.TuneBank()
    rows, odd, states, sids = [], [], [], []
    k = 0
    for o in (False, True):
        for n in LENGTHS:
            st = STATES[k % len(STATES)]
            rows.append(noise(n, 100 + k)), odd.append(o), states.append(st), sids.append(bank.add(*st))
            k += 1
    got = feed_rows(bank, reader, sids, rows, odd)
    assert bank.last_feed_ops() == (1, 1)
    for i, (x, st, sid) in enumerate(zip(rows, states, sids)):
        want, after = TR.rotate(x, *st)
        same(got[i], want, (i, x.size, odd[i], st))
        assert bank.state(sid) == after + (x.size,)
    bank.close()


@pytest.mark.parametrize("state", STATES, ids=[f"s{i}" for i in range(len(STATES))])
def test_state_values_over_more_than_one_workgroup(reader, state):
    bank = xl.TuneBank()
    sid = bank.add(*state)
    x = noise(2 * CH + 1, 7)
    (got,) = feed_rows(bank, reader, [sid], [x], [True])
    want, after = TR.rotate(x, *state)
    same(got, want, state)
    if state[2] != 0:  # the ramp wraps the phase many times inside the row
        assert abs(state[2]) * x.size * x.size // 2 >> 64 > 100
    assert bank.state(sid) == after + (x.size,)
    bank.close()


def test_split_invariance(reader):
    """one stream fed whole and split at 1, at an odd position, at chunk and at chunk +- 1: equal bytes"""
    state = STATES[5]
    x = noise(2 * CH + 1, 11)
    whole, _ = TR.rotate(x, *state)
    bank = xl.TuneBank()
    for cut in (None, 1, 777, CH, CH - 1, CH + 1):
        sid = bank.add(*state)
        pieces = [x] if cut is None else [x[:cut], x[cut:]]
        got = np.concatenate([feed_rows(bank, reader, [sid], [p], [cut is not None and cut % 2 == 1])[0] for p in pieces])
        same(got, whole, cut)
        assert bank.state(sid) == TR.advance(*state, x.size) + (x.size,)
        bank.remove(sid)
    bank.close()


def test_company_invariance_and_feed_cost(reader):
    """one stream alone and among 299 others gives equal bytes; one launch and one copy at 1 stream and at 300"""
    state = STATES[6]
    x = noise(CH + 37, 13)
    want, _ = TR.rotate(x, *state)
    alone = xl.TuneBank()
    sid = alone.add(*state)
    (got1,) = feed_rows(alone, reader, [sid], [x])
    assert alone.last_feed_ops() == (1, 1)
    same(got1, want, "alone")
    alone.close()
    bank = xl.TuneBank()
    rng = np.random.default_rng(17)
    others = [noise(int(n), 200 + i) for i, n in enumerate(rng.integers(0, 90, 299))]
    ostates = [(int(rng.integers(0, 1 << 63)) * 2 + 1, TR.signed64(int(rng.integers(0, 1 << 63)) * 2), TR.signed64(int(rng.integers(0, 1 << 62)) * 4))
               for _ in others]
    sids = [bank.add(*s) for s in ostates[:150]] + [bank.add(*state)] + [bank.add(*s) for s in ostates[150:]]
    rows = others[:150] + [x] + others[150:]
    got = feed_rows(bank, reader, sids, rows, [i % 2 == 1 for i in range(300)])
    assert bank.last_feed_ops() == (1, 1)
    same(got[150], want, "in company")
    assert bits_equal(got[150], got1)
    for i in (0, 77, 149, 151, 299):  # the company is served too
        st = (ostates[:150] + [state] + ostates[150:])[i]
        same(got[i], TR.rotate(rows[i], *st)[0], i)
    # a feed that consumes nothing issues nothing
    bank.feed(sids[:3], [0, 0, 0], [0, 0, 0], stream())
    assert bank.last_feed_ops() == (0, 0) and bank.output_device(sids[0]) == (None, 0)
    bank.close()


def test_set_between_feeds_is_continuous(reader):
    bank = xl.TuneBank()
    P, F, R = 99, 1 << 59, 1 << 40
    sid = bank.add(P, F, R)
    x = noise(3 * 1000, 19)
    outs, st = [], (P, F, R)
    for k, (nF, nR) in enumerate([(None, None), (-(1 << 60), -(1 << 45)), (0, 0)]):
        if nF is not None:
            bank.set(sid, nF, nR)
            st = (st[0], nF, nR)  # P is untouched
        assert bank.state(sid) == st + (1000 * k,)
        piece = x[1000 * k:1000 * (k + 1)]
        outs.append(feed_rows(bank, reader, [sid], [piece])[0])
        want, st = TR.rotate(piece, *st)
        same(outs[-1], want, k)
        assert bank.state(sid) == st + (1000 * (k + 1),)
    # under (0, 0) the phase the stream had reached stays: a constant rotation, not the identity
    assert st[0] >> 32 != 0 and not np.array_equal(outs[2], x[2000:]) and np.array_equal(outs[2], TR.rotate(x[2000:], st[0], 0, 0)[0])
    # ids are reused, and a reused id starts from its own state
    bank.remove(sid)
    again = bank.add(0, 0, 0)
    assert again == sid and bank.state(again) == (0, 0, 0, 0)
    bank.close()


def test_identity(reader):
    bank = xl.TuneBank()
    sid = bank.add(0, 0, 0)
    x = noise(CH + 5, 23)
    x[:4] = np.array([0, -0.0, 1e-38 + 1e-40j, 3e38 - 3e38j], np.complex64)
    (got,) = feed_rows(bank, reader, [sid], [x])
    assert np.array_equal(got, x)  # (as values: a zero may change its sign)
    bank.close()


def test_accuracy_against_float64(reader):
    """every component within hypot(xr, xi) (sqrt(2) E + 2 pi 2^-32 + 3 2^-24) of x exp(2 pi i phi_j / 2^64) in float64: the rule's
    error (E, the sweep's value: its printed hex as DESIGN 3.11 carries it, which tests/test_tune_cpu.py pins to the sweep's output; the
    sanitized sweep itself runs on the CPU side only), the 32-bit phase, the three float32 roundings"""
    E = TR.design_E()
    assert 0.0 < E <= 2.0 ** -22
    bound = np.sqrt(2.0) * E + 2 * np.pi * 2.0 ** -32 + 3 * 2.0 ** -24
    bank = xl.TuneBank()
    worst = 0.0
    for k, st in enumerate(STATES[3:7]):
        sid = bank.add(*st)
        x = noise(CH + 1, 31 + k)
        (got,) = feed_rows(bank, reader, [sid], [x])
        ref = TR.exact(x, *st)
        err = np.maximum(np.abs(got.real.astype(np.float64) - ref.real), np.abs(got.imag.astype(np.float64) - ref.imag))
        lim = np.hypot(x.real.astype(np.float64), x.imag.astype(np.float64)) * bound
        worst = max(worst, float((err / np.maximum(lim, 1e-300)).max()))
        assert (err <= lim).all(), (st, float((err / lim).max()))
    print(f"E = {E.hex()}; the largest error is {worst:.3f} of the bound")
    bank.close()


def test_refusals_consume_nothing(reader):
    bank = xl.TuneBank()
    a, b = bank.add(1, 2, 3), bank.add(4, 5, 6)
    x = noise(64, 41)
    keep, (addr,) = to_device([x])
    other = bank.add(7, 8, 9)
    for ids, counts in (([a, a], [8, 8]), ([a, b + 5], [8, 8]), ([a, b], [8, (1 << 30) + 1])):
        bank.feed([other], [addr], [8], stream())
        assert bank.last_feed_ops() == (1, 1)
        with pytest.raises(xl.XlatingError) as e:
            bank.feed(ids, [addr, addr], counts, stream())
        assert e.value.code == -errno.EINVAL
        assert bank.state(a) == (1, 2, 3, 0) and bank.state(b) == (4, 5, 6, 0)
        assert bank.last_feed_ops() == (0, 0)  # a refused feed issued nothing
    bank.remove(b)
    with pytest.raises(xl.XlatingError) as e:
        bank.feed([a, b], [addr, addr], [8, 8], stream())  # a dead id
    assert e.value.code == -errno.EINVAL and bank.state(a) == (1, 2, 3, 0)
    with pytest.raises(xl.XlatingError) as e:
        bank.feed([a], [addr + 4], [8], stream())  # a row that is not 8-byte aligned
    assert e.value.code == -errno.EINVAL and bank.state(a) == (1, 2, 3, 0)
    for fn in (lambda: bank.set(b, 0, 0), lambda: bank.state(b), lambda: bank.remove(b), lambda: bank.output_device(b)):
        with pytest.raises(xl.XlatingError):
            fn()
    # the bank still works, from the untouched state
    (got,) = feed_rows(bank, reader, [a], [x])
    same(got, TR.rotate(x, 1, 2, 3)[0], "after the refusals")
    del keep
    bank.close()
