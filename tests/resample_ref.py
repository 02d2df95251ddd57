"""The float64 restatement of the resampler bank's definition (include/xlating_resample.h), and the bound its float32 result obeys.

Per stream: coprime L, M, a float32 prototype h (h[i] = 0 for i >= P), Q = ceil(P / L), complex float32 input x (x[n] = 0 for n < 0):
    t = m * M,  n_m = t // L,  p_m = t % L,   y[m] = sum_{q < Q} h[p_m + q L] * x[n_m - q],   m < ceil(N L / M)
Here with the same float32 h and x, every product (exact in double: 24 + 24 bits) summed in double.

The bound is derived, not measured: a float32 dot product of Q terms summed in a fixed order obeys (Higham, Accuracy and Stability of
Numerical Algorithms, 3.1)  |y32 - y| <= gamma_Q * S,  gamma_Q = Q u / (1 - Q u),  u = 2^-24,  S = sum_q |h| |x component|,
per component; a term that underflows adds at most the smallest normal number, 2^-126, Q of them at most."""
import numpy as np

U = 2.0 ** -24


def counts(L, M, N):
    """outputs after N consumed samples"""
    return -((-N * L) // M)


def positions(L, M, m):
    """(n_m, p_m) of output indices m (int64 array or int), by the definition"""
    t = np.asarray(m, dtype=np.int64) * M
    return t // L, t % L


def restate(L, M, taps, x):
    """x: complex64 [N] -> (y complex128 [ceil(N L / M)], S_re, S_im float64)"""
    h = np.asarray(taps, dtype=np.float32)
    x = np.asarray(x, dtype=np.complex64)
    P, N = h.size, x.size
    Q = -(-P // L)
    hp = np.zeros(L * Q, np.float64)
    hp[:P] = h
    table = hp.reshape(Q, L).T  # [p][q] = h[p + q L]
    nout = counts(L, M, N)
    n, p = positions(L, M, np.arange(nout))
    xr = np.concatenate([np.zeros(Q - 1), x.real.astype(np.float64)])
    xi = np.concatenate([np.zeros(Q - 1), x.imag.astype(np.float64)])
    yr, yi, sr, si = (np.zeros(nout) for _ in range(4))
    for q in range(Q):
        c = table[p, q]
        a, b = xr[n + (Q - 1) - q], xi[n + (Q - 1) - q]
        yr += c * a
        yi += c * b
        sr += np.abs(c) * np.abs(a)
        si += np.abs(c) * np.abs(b)
    return yr + 1j * yi, sr, si


def bound(Q, S):
    return Q * U / (1.0 - Q * U) * S + Q * 2.0 ** -126


def check(y32, L, M, taps, x, what=""):
    """every output of y32 (complex64) within the derived bound of the restatement of (L, M, taps) applied to x; -> the largest
    error over its bound (<= 1)"""
    y, sr, si = restate(L, M, taps, x)
    y32 = np.asarray(y32)
    assert y32.dtype == np.complex64 and y32.shape == y.shape, (what, y32.shape, y.shape)
    Q = -(-np.asarray(taps).size // L)
    er, ei = np.abs(y32.real.astype(np.float64) - y.real), np.abs(y32.imag.astype(np.float64) - y.imag)
    br, bi = bound(Q, sr), bound(Q, si)
    worst = max(float((er / br).max(initial=0.0)), float((ei / bi).max(initial=0.0)))
    print(f"resample {what}: L {L} M {M} Q {Q} outputs {y.size} worst error / bound {worst:.3f}")
    bad = np.nonzero((er > br) | (ei > bi))[0]
    assert bad.size == 0, (what, L, M, bad[:5], er[bad[:5]], br[bad[:5]], ei[bad[:5]], bi[bad[:5]])
    return worst
