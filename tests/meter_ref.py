"""The power meter's rule (sdr-server_amd/csrc/xl_meter_rule.h) and the squelch policy with its log (xl_serve_squelch.h), restated:
numpy float32 in exactly the stated order for cf32 rows, Python integers for cs16 rows, plain Python for the policy.  Nothing here
calls the library."""
import math

import numpy as np

PIECE, THREADS, PER_THREAD = 2048, 256, 8
U = 2.0 ** -24
GAMMA17 = 17 * U / (1 - 17 * U)
LOG = 64


def bound(pieces):
    """the relative bound of a cf32 row's mean power against exact arithmetic (no underflow): gamma_17 for the float32 tree, and the
    host's pieces - 1 double additions and one division"""
    return GAMMA17 + 1.0001 * pieces * 2.0 ** -53


def partials_cf32(x):
    """x: complex64 [n] -> uint64 [ceil(n / 2048)]: each piece's float32 partial, its bits in the low half"""
    x = np.asarray(x, dtype=np.complex64)
    n = x.size
    m = -(-n // PIECE)
    out = np.zeros(m, np.uint64)
    with np.errstate(all="ignore"):
        for k in range(m):
            z = np.zeros(PIECE, np.complex64)
            seg = x[k * PIECE:(k + 1) * PIECE]
            z[:seg.size] = seg
            re, im = z.real.astype(np.float32), z.imag.astype(np.float32)
            p = (re * re).astype(np.float32) + (im * im).astype(np.float32)  # (a padded sample: +0)
            p = p.astype(np.float32).reshape(PER_THREAD, THREADS)  # [i][t]: sample t + 256 i
            s = p[0].copy()
            for i in range(1, PER_THREAD):
                s = (s + p[i]).astype(np.float32)
            s = s.reshape(THREADS // 64, 64)
            stride = 32
            while stride >= 1:
                s[:, :stride] = (s[:, :stride] + s[:, stride:2 * stride]).astype(np.float32)
                stride //= 2
            w = s[:, 0]
            part = np.float32(np.float32(w[0] + w[1]) + np.float32(w[2] + w[3]))
            out[k] = int(np.array([part], np.float32).view(np.uint32)[0])
    return out


def mean_cf32(partials, n):
    s = 0.0
    for v in np.asarray(partials, np.uint64):
        s += float(np.array([int(v) & 0xFFFFFFFF], np.uint32).view(np.float32)[0])
    return s / float(n) if n else 0.0


def partials_cs16(x):
    """x: int16 [n, 2] -> uint64 [ceil(n / 2048)]: each piece's exact sum of re^2 + im^2"""
    x = np.asarray(x, dtype=np.int16).reshape(-1, 2).astype(np.int64)
    n = x.shape[0]
    m = -(-n // PIECE)
    out = np.zeros(m, np.uint64)
    for k in range(m):
        seg = x[k * PIECE:(k + 1) * PIECE]
        out[k] = sum(int(a) * int(a) + int(b) * int(b) for a, b in seg)
    return out


def mean_cs16(partials, n):
    s = sum(int(v) for v in np.asarray(partials, np.uint64))
    return float(s) / float(n) / 2.0 ** 30 if n else 0.0


def power_cf32(x):
    x = np.asarray(x, dtype=np.complex64)
    return mean_cf32(partials_cf32(x), x.size)


def power_cs16(x):
    x = np.asarray(x, dtype=np.int16).reshape(-1, 2)
    return mean_cs16(partials_cs16(x), x.shape[0])


def exact_power_cf32(x):
    """float64, pairwise: what the bound is held against"""
    x = np.asarray(x, dtype=np.complex64)
    if x.size == 0:
        return 0.0
    re, im = x.real.astype(np.float64), x.imag.astype(np.float64)
    return math.fsum((re * re + im * im).tolist()) / x.size  # (each float32 square is exact in double; the sum of two within 2^-53)


class Squelch:
    """one client's policy: the gate is closed at first"""

    def __init__(self, open_power, close_power, hang_calls):
        assert open_power >= close_power >= 0.0 and math.isfinite(open_power)
        self.open_power, self.close_power, self.hang = open_power, close_power, hang_calls
        self.open, self.below = False, 0

    def step(self, P):
        """-> the gate after the call: True delivers this call's row"""
        if not (P < self.open_power):
            self.open, self.below = True, 0
        elif self.open:
            if P < self.close_power:
                self.below += 1
                if self.below > self.hang:
                    self.open, self.below = False, 0
            else:
                self.below = 0
        return self.open


class SquelchLog:
    """gate changes (stream_sample, delivered_sample, open): begins open, entries alternate, two at one stream sample cancel, the
    latest 64 are kept"""

    def __init__(self):
        self.entries, self.closed = [], False

    def note(self, stream_sample, delivered_sample, open_):
        if (not open_) == self.closed:
            return
        self.closed = not open_
        if self.entries and self.entries[-1][0] == stream_sample:
            self.entries.pop()
            return
        if len(self.entries) == LOG:
            self.entries.pop(0)
        self.entries.append((int(stream_sample), int(delivered_sample), 1 if open_ else 0))


def run_policy(powers, lens, open_power, close_power, hang_calls):
    """a client squelched from its first call: per-call powers and row lengths -> (gates [calls], log entries, withheld samples)"""
    q, log = Squelch(open_power, close_power, hang_calls), SquelchLog()
    produced = delivered = withheld = 0
    gates = []
    for P, n in zip(powers, lens):
        g = q.step(P)
        log.note(produced, delivered, g)
        gates.append(bool(g))
        produced += n
        if g:
            delivered += n
        else:
            withheld += n
    return gates, log.entries, withheld
