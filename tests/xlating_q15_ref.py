"""The integer restatement of the reference's cs16 output family (xlating.c:92-140, 416-433), in numpy int64, with a count of
how often each of its saturating or truncating lines acts.

Per stream: decimation D, the reversed band-pass taps in Q15 as pairs h[T, 2] (Oracle.rtaps_q15), the Q15 phase increment
(ir, ii), a history of T - 1 .. T + D - 2 int16 pairs (zeros at creation) and a phase (pr, pi) = (32767, 0) at creation.  Per call
the converted samples are appended to the history; for every window start 0, D, 2 D, .. that holds T samples:
    sr = sum_i xr[i] hr[i] - xi[i] hi[i]       si = sum_i xr[i] hi[i] + xi[i] hr[i]            exact in int64      (:114-115)
    ar = clip(wrap32(sr >> 15)),  ai = clip(wrap32(si >> 15))      wrap32: the low 32 bits as two's complement      (:118-119)
    yr = clip((ar pr - ai pi) >> 15),  yi = clip((ar pi + ai pr) >> 15)                                             (:121-124)
    (pr, pi) <- (clip((pr ir - pi ii) >> 15), clip((pr ii + pi ir) >> 15))                                          (:126-129)
clip is to [-32768, 32767]; wrap32 is what passing an int64 to saturate_to_int16(int32_t) does.  Unlike the oracle, a stream here
can be started from any history and phase."""
import numpy as np

SITES = ("sum_hi", "sum_lo", "out_hi", "out_lo", "wrap_hi", "wrap_lo")


def convert(fmt, x):
    """The three conversions to Q15 (xlating.c:417-433): 1-D scalar elements (I, Q interleaved) -> int64 [N // 2, 2]"""
    x = np.asarray(x)
    n = x.size // 2
    v = x[:2 * n].astype(np.int64).reshape(n, 2)
    if fmt == "cu8":
        assert x.dtype == np.uint8
        return (v - 128) << 8
    if fmt == "cs8":
        assert x.dtype == np.int8
        return v << 8
    assert fmt == "cs16" and x.dtype == np.int16
    return v


def increment(phase_incr):
    """Oracle.phase_incr (float32 re, im) -> the Q15 increment: (int16)(re * 32767), the product in float32 (xlating.c:548-549)"""
    re, im = (np.float32(v) * np.float32(32767.0) for v in phase_incr)
    assert re.dtype == np.float32
    return int(np.trunc(re)), int(np.trunc(im))


def wrap32(v):
    """int64 -> the value of its low 32 bits as two's complement"""
    return ((v + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)


def clip16(v):
    return np.clip(v, -32768, 32767)


class Stream:
    def __init__(self, D, taps_q15, incr, history=None, phase=(32767, 0)):
        self.D = int(D)
        self.h = np.asarray(taps_q15).astype(np.int64).reshape(-1, 2)
        self.T = self.h.shape[0]
        self.ir, self.ii = int(incr[0]), int(incr[1])
        self.hist = np.zeros((self.T - 1, 2), np.int64) if history is None else np.asarray(history, np.int64).reshape(-1, 2)
        assert self.hist.shape[0] >= self.T - 1
        self.pr, self.pi = int(phase[0]), int(phase[1])
        self.counts = dict.fromkeys(SITES, 0)  # over all calls so far
        self.last = dict.fromkeys(SITES, 0)    # of the latest call

    def process(self, fmt, x):
        """one call: -> int16 [K, 2]"""
        T, D = self.T, self.D
        work = np.concatenate([self.hist, convert(fmt, x)])
        self.last = dict.fromkeys(SITES, 0)
        K = 0 if work.shape[0] < T else (work.shape[0] - T) // D + 1
        out = np.zeros((K, 2), np.int16)
        if K:
            idx = (np.arange(K) * D)[:, None] + np.arange(T)[None, :]
            wr, wi = work[idx, 0], work[idx, 1]
            hr, hi = self.h[:, 0], self.h[:, 1]
            s = np.stack([wr @ hr - wi @ hi, wr @ hi + wi @ hr], axis=1) >> 15
            self.last["wrap_hi"] = int((s > 0x7FFFFFFF).sum())
            self.last["wrap_lo"] = int((s < -0x80000000).sum())
            s = wrap32(s)
            self.last["sum_hi"] = int((s > 32767).sum())
            self.last["sum_lo"] = int((s < -32768).sum())
            a = clip16(s)
            ph = np.zeros((K, 2), np.int64)
            pr, pi = self.pr, self.pi
            for m in range(K):
                ph[m] = pr, pi
                tr, ti = pr * self.ir - pi * self.ii, pr * self.ii + pi * self.ir
                pr, pi = min(max(tr >> 15, -32768), 32767), min(max(ti >> 15, -32768), 32767)
            self.pr, self.pi = pr, pi
            y = np.stack([a[:, 0] * ph[:, 0] - a[:, 1] * ph[:, 1], a[:, 0] * ph[:, 1] + a[:, 1] * ph[:, 0]], axis=1) >> 15
            self.last["out_hi"] = int((y > 32767).sum())
            self.last["out_lo"] = int((y < -32768).sum())
            out = clip16(y).astype(np.int16)
        self.hist = work[K * D:]
        for k in SITES:
            self.counts[k] += self.last[k]
        return out

    @property
    def phase(self):
        return self.pr, self.pi


def of_oracle(o, history=None, phase=(32767, 0)):
    """a Stream with the taps, decimation and increment of a pyoracle.Oracle"""
    return Stream(o.D, o.rtaps_q15, increment(o.phase_incr), history, phase)
