"""CPU test (-m "not gpu") of the squelch scenario (tests/squelch_cases.py) against the oracle: every call's power of every client,
from pyoracle's stream (through tests/resample_ref.py for the fractional pair), lies far from both marks -- a full call at least 10x
above the open mark, a quiet call at least 10x below the close mark, a half-level call at least 3x from both -- so that no run on a GPU
can sit on a threshold; and the envelopes hold the cases the GPU test is about."""
import functools

import numpy as np

import meter_ref as MR
import resample_ref as RR
import sdr_server_amd as xl
import squelch_cases as SC
from pyoracle import Oracle


@functools.lru_cache(maxsize=None)
def oracle_powers():
    """-> {client index: ([power per call], [samples per call])} in float64"""
    raw = SC.capture()
    out = {}
    for i in (0, 2):
        center, rate = SC.CLIENTS[i]
        req = xl.WireRequest(center, rate, SC.BAND_FREQ, 0)
        code, adm, rs, why = xl.wire_admit_any_rate(req, SC.BAND_RATE, 0, 5)
        assert code == 0
        code, taps = xl.create_low_pass_filter(1.0, SC.BAND_RATE, adm.lpf_cutoff, adm.lpf_transition)
        assert code == 0
        o = Oracle(adm.decimation, taps, adm.center_offset, SC.BAND_RATE, SC.BUFFER)
        blocks = [o.process("cu8", raw[off:off + SC.BUFFER], "cf32") for off in range(0, raw.size, SC.BUFFER)]
        o.close()
        per_call = [sum(b.size for b in blocks[k * SC.GROUP:(k + 1) * SC.GROUP]) for k in range(SC.CALLS)]
        y = np.concatenate(blocks).astype(np.complex128)
        if (rs.L, rs.M) != (1, 1):
            code, rtaps = xl.wire_resample_taps(req, rs, 5)
            assert code == 0
            y, _, _ = RR.restate(rs.L, rs.M, rtaps, np.concatenate(blocks))
            ends = [RR.counts(rs.L, rs.M, n) for n in np.cumsum(per_call)]
            per_call = [int(e - s) for s, e in zip([0] + ends[:-1], ends)]
        assert sum(per_call) == y.size
        pos, powers = 0, []
        for n in per_call:
            powers.append(float(np.mean(np.abs(y[pos:pos + n]) ** 2)))
            pos += n
        out[i] = out[i + 1] = (powers, per_call)
    return out


def test_every_call_is_far_from_both_marks():
    assert SC.OPEN_POWER >= SC.CLOSE_POWER > 0
    for i in (0, 2):
        powers, lens = oracle_powers()[i]
        assert len(powers) == SC.CALLS and min(lens) > 1000
        for k, (what, P) in enumerate(zip(SC.envelope(i), powers)):
            print(f"client {i} call {k} {what:5s} power {P:.3e}  /open {P / SC.OPEN_POWER:.3g}  /close {P / SC.CLOSE_POWER:.3g}")
            if what == "full":
                assert P >= 10 * SC.OPEN_POWER, (i, k, P)
            elif what == "off":
                assert P <= SC.CLOSE_POWER / 10, (i, k, P)
            else:
                assert 3 * SC.CLOSE_POWER <= P <= SC.OPEN_POWER / 3, (i, k, P)
    assert (SC.CLIENTS[0][1], SC.CLIENTS[2][1]) == (48000, 44100)


def test_the_envelopes_hold_the_cases():
    """with the oracle's powers the Python policy walks through: a half-level call while closed and while open, two quiet calls in a
    row, a reopening, a quiet last call; hang 1 delivers one quiet call more; in call 0 nobody is open"""
    for i in (1, 3):
        powers, lens = oracle_powers()[i]
        env = SC.envelope(i)
        g0, log0, w0 = SC.expected_gates(powers, lens, 0)
        g1, log1, w1 = SC.expected_gates(powers, lens, 1)
        assert g0 == [w == "full" or (w == "half" and k > 0 and g0[k - 1]) for k, w in enumerate(env)]
        half = [k for k, w in enumerate(env) if w == "half"]
        assert any(not g0[k] for k in half) and any(g0[k] for k in half), "half level while closed, and while open"
        assert any(env[k] == env[k + 1] == "off" for k in range(SC.CALLS - 1)), "two quiet calls in a row"
        assert any(g0[k] and not g0[k - 1] and any(g0[:k - 1]) for k in range(2, SC.CALLS)), "a reopening"
        assert env[-1] == "off" and not g0[-1], "a quiet last call"
        assert not g0[0] and not g1[0]
        assert sum(g1) > sum(g0) and all(a or not b for a, b in zip(g1, g0)), "the hang time only adds calls"
        assert w0 == sum(n for g, n in zip(g0, lens) if not g) and w1 < w0
        assert [e[2] for e in log0] == [k % 2 for k in range(len(log0))] and log0[0][:2] == (0, 0), "closed from the first sample on"
        assert len(log0) >= 4
