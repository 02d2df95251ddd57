"""The integer restatement of the Q15 resampler bank's definition (include/xlating_resample_q15.h), in numpy int64.

Per stream: coprime L, M, a float32 prototype h (h[i] = 0 for i >= P), Q = ceil(P / L), int16 pairs x (x[n] = 0 for n < 0):
    c[i] = (int16) trunc(h[i] * 32768)          the product in float32, truncation toward zero; out of range: refused
    t = m * M,  n_m = t // L,  p_m = t % L,   s = sum_{q < Q} c[p_m + q L] * x[n_m - q],   y[m] = clip(s >> 15, -32768, 32767)
for m < ceil(N L / M).  |s| <= Q * 2^30 <= 2^40: exact in int64, in any order.  The positions and counts are resample_ref's."""
import numpy as np

import resample_ref as RR


def quantize(taps):
    """float32 taps -> int64 array of the int16 values; ValueError where the definition refuses"""
    h = np.asarray(taps, dtype=np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        v = h * np.float32(32768.0)
    assert v.dtype == np.float32
    if not np.all(np.isfinite(v)):
        raise ValueError("a tap is not finite")
    c = np.trunc(v.astype(np.float64)).astype(np.int64)
    if c.size and (c.min() < -32768 or c.max() > 32767):
        raise ValueError("a tap does not fit int16")
    return c


def table(L, taps):
    """-> int64 [L][Q], [p][q] = c[p + q L]"""
    c = quantize(taps)
    Q = -(-c.size // L)
    cp = np.zeros(L * Q, np.int64)
    cp[:c.size] = c
    return cp.reshape(Q, L).T


def phase_abs_sums(L, taps):
    """sum_q |c| per phase: <= 65535 everywhere is the 32-bit condition"""
    return np.abs(table(L, taps)).sum(axis=1)


def sums(L, M, taps, x):
    """x: int16 [N, 2] -> the exact sums s, int64 [ceil(N L / M), 2]"""
    x = np.asarray(x)
    assert x.dtype == np.int16 and x.ndim == 2 and x.shape[1] == 2
    tab = table(L, taps)
    Q = tab.shape[1]
    N = x.shape[0]
    nout = RR.counts(L, M, N)
    n, p = RR.positions(L, M, np.arange(nout))
    xp = np.concatenate([np.zeros((Q - 1, 2), np.int64), x.astype(np.int64)])
    s = np.zeros((nout, 2), np.int64)
    for q in range(Q):
        s += tab[p, q][:, None] * xp[n + (Q - 1) - q]
    return s


def restate(L, M, taps, x):
    """x: int16 [N, 2] -> y int16 [ceil(N L / M), 2]"""
    return np.clip(sums(L, M, taps, x) >> 15, -32768, 32767).astype(np.int16)
