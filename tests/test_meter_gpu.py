"""GPU tests of the power meter (include/xlating_meter.h): the rows of tests/meter_cases.py -- lengths 0 .. 4097 around the thread
count and the piece, noise at three scales, zeros, subnormal squares, a NaN and an infinity alone in a last piece, an overflow, cs16
rows at both ends of the range -- laid out in one device buffer at both alignments with poisoned padding between them, measured all
in ONE measurement and each alone: the partials bit for bit the restatement's (tests/meter_ref.py), the powers equal as doubles, the
buffer untouched, the operations counted."""
import functools
import math

import numpy as np
import pytest

import meter_cases as MC
import meter_ref as MR
import sdr_server_amd as xl

pytestmark = pytest.mark.gpu


def _layout(rows, esz, shifts, poison):
    """rows (uint8 views) placed one behind the other, row k at an address congruent to shifts[k % 2] mod 2 * max(shifts), with at least
    64 bytes of poison in front of, between and behind them -> (uint8 buffer, offsets)"""
    period = 2 * max(shifts)
    offs, at = [], 64
    for k, r in enumerate(rows):
        at += (shifts[k % 2] - at) % period
        offs.append(at)
        at += r.size + 64
    buf = np.frombuffer(np.tile(poison, (at + 64) // poison.size + 1).tobytes(), np.uint8)[:at + 64].copy()
    for o, r in zip(offs, rows):
        buf[o:o + r.size] = r
    return buf, offs


@functools.lru_cache(maxsize=None)
def device(fmt):
    """-> (torch uint8 tensor on the device, the host image, offsets, sample counts, expected partials, expected powers)"""
    import torch

    if fmt == "cf32":
        rows = [x for _, x, _ in MC.cf32_rows()]
        raw = [np.frombuffer(x.tobytes(), np.uint8) for x in rows]
        buf, offs = _layout(raw, 8, (0, 8), np.array([0x7FC00000], np.uint32).view(np.uint8))  # NaNs between the rows
        parts = [MR.partials_cf32(x) for x in rows]
        powers = [MR.mean_cf32(p, x.size) for p, x in zip(parts, rows)]
        counts = [x.size for x in rows]
    else:
        rows = [x for _, x, _ in MC.cs16_rows()]
        raw = [np.frombuffer(x.tobytes(), np.uint8) for x in rows]
        buf, offs = _layout(raw, 4, (0, 4), np.array([0x7FFF], np.uint16).view(np.uint8))
        parts = [MR.partials_cs16(x) for x in rows]
        powers = [MR.mean_cs16(p, x.shape[0]) for p, x in zip(parts, rows)]
        counts = [x.shape[0] for x in rows]
    d = torch.from_numpy(buf.copy()).cuda()
    assert d.data_ptr() % 16 == 0
    buf.setflags(write=False)
    return d, buf, offs, counts, parts, powers


def _same(a, b):
    return (math.isnan(a) and math.isnan(b)) or a == b


@pytest.mark.parametrize("fmt", ["cf32", "cs16"])
def test_all_rows_in_one_measurement(fmt):
    import torch

    d, buf, offs, counts, parts, powers = device(fmt)
    mod = 16 if fmt == "cf32" else 8
    assert {(d.data_ptr() + o) % mod for o, n in zip(offs, counts) if n} == {0, mod // 2}, "both alignments"
    m = xl.Meter()
    assert m.query() is True and m.last_ops() == (0, 0)
    st = torch.cuda.current_stream().cuda_stream
    m.measure(fmt, [d.data_ptr() + o for o in offs], counts, st)
    assert m.last_ops() == (1, 2), "one launch, one table copy and one copy back"
    m.wait()
    assert m.query() is True
    for i, (name, *_rest) in enumerate(MC.cf32_rows() if fmt == "cf32" else MC.cs16_rows()):
        got = m.partials(i)
        assert got.size == -(-counts[i] // MR.PIECE) and np.array_equal(got, parts[i]), (name, got[:4], parts[i][:4])
        p, n = m.power(i)
        assert n == counts[i] and _same(p, powers[i]), (name, p, powers[i])
    with pytest.raises(xl.XlatingError) as e:
        m.power(len(counts))
    assert e.value.code == -22
    # what the rows hold, stated once more where the figures are exact
    names = [r[0] for r in (MC.cf32_rows() if fmt == "cf32" else MC.cs16_rows())]
    if fmt == "cf32":
        z = m.power(names.index("zeros_4097"))[0]
        assert z == 0.0 and math.copysign(1.0, z) == 1.0
        assert m.power(names.index("subnormal_2049"))[0] > 0.0, "subnormal squares are kept, not flushed"
        for bad, after in (("nan_4097", "after_nan_257"), ("inf_2049", "after_inf_3")):
            assert not math.isfinite(m.power(names.index(bad))[0]) and math.isfinite(m.power(names.index(after))[0])
            fin = np.isfinite(m.partials(names.index(bad)).astype(np.uint32).view(np.float32))
            assert list(fin) == [True] * (fin.size - 1) + [False], "its other pieces are untouched"
        assert m.power(names.index("overflow_300"))[0] == float("inf")
    else:
        assert m.power(names.index("min_4097"))[0] == 2.0
        assert m.power(names.index("max_2049"))[0] == 2.0 * 32767.0 ** 2 / 2.0 ** 30
        assert m.power(names.index("zeros_257"))[0] == 0.0
    torch.cuda.synchronize()
    assert np.array_equal(d.cpu().numpy(), buf), "the rows are read in place and never written"
    m.close()


@pytest.mark.parametrize("fmt", ["cf32", "cs16"])
def test_each_row_alone(fmt):
    """company changes nothing: every row measured by itself gives the bits it gave among the others; an empty measurement issues
    nothing"""
    import torch

    d, buf, offs, counts, parts, powers = device(fmt)
    st = torch.cuda.current_stream().cuda_stream
    m = xl.Meter()
    for i, (o, n) in enumerate(zip(offs, counts)):
        m.measure(fmt, [d.data_ptr() + o], [n], st)
        assert m.last_ops() == ((1, 2) if n else (0, 0)), i
        m.wait()
        assert np.array_equal(m.partials(0), parts[i]), i
        assert _same(m.power(0)[0], powers[i]) and m.power(0)[1] == n, i
    m.measure(fmt, [0, 0, 0], [0, 0, 0], st)
    assert m.last_ops() == (0, 0) and m.query() is True
    assert [m.power(i) for i in range(3)] == [(0.0, 0)] * 3 and m.partials(1).size == 0
    m.measure(fmt, [], [], st)
    assert m.last_ops() == (0, 0)
    m.close()


def test_refusals():
    import torch

    d, buf, offs, counts, parts, powers = device("cf32")
    st = torch.cuda.current_stream().cuda_stream
    m = xl.Meter()
    base = d.data_ptr() + offs[counts.index(2048)]
    for fmt, ptr, n in (("cf32", base + 4, 8), ("cs16", base + 2, 8), ("cf32", 0, 8), ("cf32", base, (1 << 30) + 1)):
        with pytest.raises(xl.XlatingError) as e:
            m.measure(fmt, [ptr], [n], st)
        assert e.value.code == -22 and m.last_ops() == (0, 0)
    assert xl.meter_lib().xlating_meter_measure_device(m.h, 2, 0, None, None, None) == -22
    m.measure("cf32", [base + 8, 0], [100, 0], st)  # (a count of 0: its address is not looked at)
    m.wait()
    assert np.array_equal(m.partials(0), MR.partials_cf32(MC.cf32_rows()[counts.index(2048)][1][1:101]))
    m.close()
