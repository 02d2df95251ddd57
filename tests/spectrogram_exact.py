"""Inputs of the spectrogram family whose reference answer is known without an FFT library, and that answer: what
tests/test_spectrogram_exact_cpu.py counts and tests/test_spectrogram_exact_gpu.py holds the kernels to, bit for bit.

The expected values restate spectrogram.c:146-162 (power, row maximum, 10 log10f, half swap) and png_util.c:53-63 (the pixel) of the
reference tree in float32, step by step, as its library computes them (-ffp-contract=off: every product and sum rounds on its own).

  the ladder      cf32, W = 1, sampling_rate = 1: a one-point transform is the identity and norm is 1, so every sample is one row of one
                  bin whose power is fl(fl(fl(re re) + fl(im im)) + 1e-20f).  Samples whose dB sits next to every integer from -200 to
                  +4 (the pixel boundaries), both clamps, the floor, powers that overflow.
  the constants   a constant c, c (-1)^n and (cf32) c i^n at a power-of-two W: all data are sums of equal powers of two or exact
                  cancellations and the only non-zero values travel through twiddle w^0 = 1, so the peak column holds c's exact float32
                  power and every other column 1e-20f: dB bits of -200.0, pixel 55.
  the NaN cases   four rows of spectrogram_ref.signal with NaN samples placed so that the reference's fmaxf rule (a NaN power loses
                  against any number) shows: in one transform of a row, among the skipped samples, in every transform of a row."""
import functools

import numpy as np

import spectrogram_ref as R

F32 = np.float32
FLOOR = F32(1e-20)  # spectrogram.c:142: + 1e-20f


# ----------------------------------------------------------------------------------------------------- the float32 restatement
def power_f32(re, im):
    """spectrogram.c:140-142 of a bin whose X / W is (re, im): float32 products, their float32 sum, + 1e-20f"""
    re, im = np.asarray(re, F32), np.asarray(im, F32)
    with np.errstate(over="ignore", under="ignore"):
        return (re * re + im * im) + FLOOR


def log10_f32(p, via=np.float64):
    """the correctly rounded log10f of float32 powers: taken in `via` (float64, or np.longdouble as a cross-check) and rounded once.
    Not numpy's float32 log10: that one is an ulp off the correctly rounded value on about half of the powers next to 10^(k/10)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.log10(np.asarray(p, F32).astype(via)).astype(F32)


def db_f32(p):
    """spectrogram.c:150: 10 * log10f(p), the product in float32"""
    return F32(10) * log10_f32(p)


def pixel_f32(d):
    """png_util.c:53-63: the float32 sum d + 255, then 255 if >= 255, the truncation if > 0, else 0 (a NaN: 0)"""
    f = np.asarray(d, F32) + F32(255)
    with np.errstate(invalid="ignore"):
        v = np.where(f >= 255, 255, np.where(f > 0, np.trunc(f), 0))
    return v.astype(np.uint8)


def midpoint_margin(p):
    """for float32 powers p: how far the float64 log10 lies from the nearest midpoint of two neighbouring float32 values, in float64
    ulps of the logarithm.  Beyond a few ulps, any double log10 that is good to a few ulps -- the device's -- rounds to the same
    float32.  log10(1) = 0 is exact and counts as infinitely far (its neighbours are subnormal: nothing here may depend on whether the
    process flushes those)."""
    L = np.log10(np.asarray(p, F32).astype(np.float64))
    f = np.where(L == 0, F32(1), L.astype(F32))
    lo = (f.astype(np.float64) + np.nextafter(f, F32(-np.inf)).astype(np.float64)) / 2
    hi = (f.astype(np.float64) + np.nextafter(f, F32(np.inf)).astype(np.float64)) / 2
    margin = np.minimum(np.abs(L - lo), np.abs(L - hi)) / np.spacing(np.where(L == 0, 1.0, np.abs(L)))
    return np.where(L == 0, np.inf, margin)


# ----------------------------------------------------------------------------------------------------- the pixel ladder
def _step(v, n):
    """the positive float32 v moved by n ulps"""
    return (np.asarray(v, F32).view(np.uint32).astype(np.int64) + n).astype(np.uint32).view(F32)


def _first_at_or_above(k):
    """the smallest positive float32 re with db_f32(power_f32(re, 0)) >= k (both are monotone in re; k > -200: re = 0 gives -200.0)"""
    lo, hi = 1, int(F32(4.0).view(np.uint32))  # bit patterns: lo below, hi at or above
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if db_f32(power_f32(np.uint32(mid).view(F32), 0)) >= k:
            hi = mid
        else:
            lo = mid
    return np.uint32(hi).view(F32)


LADDER_EXTRA = [0.0, 1e-30, 1e-12, 1.0, 0.5, 0.70710678, 2.0, 1e4, 3e19]


@functools.lru_cache(maxsize=None)
def ladder():
    """-> (raw float32 [2 n] interleaved, power float32 [n], dB float32 [n, 1], pixels uint8 [n, 1]): n rows of W = 1 at
    sampling_rate 1.
      - for every integer k of -200 .. +4 the float32 nearest sqrt(10^(k/10)) and its neighbours to +-3 ulps, im = 0; for every tenth
        k a second set with re = im (a sum of two products);
      - for every k of -199 .. +4 the smallest re whose dB is at or above k, three neighbours below it and two above.  Below about
        -125 dB the first set does not straddle k: the + 1e-20f moves those powers by more than 3 ulps of re;
      - 0, 1e-30, 1e-12 (powers absorbed by the floor or nearly so); 1, 0.5, 0.70710678 (both parts: power 0.99999994, dB -2.6e-7, the
        float32 sum exactly 255.0); 2, 1e4, 3e19 (3e19: the power overflows to +Inf, dB +Inf, pixel 255) -- each with im = 0 and with
        re = im.
    The expected dB and pixel are those of the float32 sample as stored: no sample has to hit a target."""
    re, im = [], []
    for k in range(-200, 5):
        a = F32(np.sqrt(10.0 ** (k / 10.0)))
        for u in range(-3, 4):
            re.append(_step(a, u))
            im.append(F32(0))
        if k % 10 == 0:
            b = F32(np.sqrt(10.0 ** (k / 10.0) / 2.0))
            for u in range(-3, 4):
                re.append(_step(b, u))
                im.append(_step(b, u))
    for k in range(-199, 5):
        a = _first_at_or_above(k)
        for u in range(-3, 3):
            re.append(_step(a, u))
            im.append(F32(0))
    for v in LADDER_EXTRA:
        re += [F32(v), F32(v)]
        im += [F32(0), F32(v)]
    pairs = np.unique(np.stack([np.asarray(re, F32), np.asarray(im, F32)], axis=1).view(np.uint32), axis=0).view(F32)
    raw = np.ascontiguousarray(pairs).reshape(-1)
    p = power_f32(pairs[:, 0], pairs[:, 1])
    d = db_f32(p)
    for a in (raw, p, d):
        a.setflags(write=False)
    return raw, p, d.reshape(-1, 1), pixel_f32(d).reshape(-1, 1)


# ----------------------------------------------------------------------------------------------------- constants and on-bin tones
PLAIN_WIDTHS = [2, 4, 8, 64, 1024, 8192]   # one-workgroup transforms
PLAIN_WIDE = [16384]                       # the two-level plain transform
BLUE_WIDTHS = [3, 100, 1000, 8191]         # Bluestein
BLUE_WIDE = [20000]
# raw (I, Q) per format: silence; the nearest cu8 gets to silence (+-2^-8: peak power 2^-15, pixel 209) and its ends; the ends of cs16
# (-32768: power 2.0, dB 3.0103002, pixel 255 by the clamp) and one LSB (pixel 167); cf32 above and below full scale
CONSTANTS = {"cu8": [(127, 127), (128, 128), (0, 0), (255, 255)],
             "cs16": [(0, 0), (-32768, -32768), (32767, 32767), (1, 1)],
             "cf32": [(0.0, 0.0), (1.0, 1.0), (0.5, 0.0)]}
_NP = {"cu8": np.uint8, "cs16": np.int16, "cf32": np.float32}


def _negated(fmt, c):
    """the raw pair whose converted value is -convert(c), or None where the format has none (cs16 -32768) or it is c itself (0)"""
    if fmt == "cu8":
        return (255 - c[0], 255 - c[1])  # (b - 127.5) / 128 -> -(b - 127.5) / 128
    if c == (0, 0) or -32768 in c:
        return None
    return (-c[0], -c[1])


def row_shapes(W):
    """sampling rates: F = 1 without a skip; F = 3 with a skip of W // 2 + 1 where that stays below W (W = 2: F = 3, no skip)"""
    return [W, 3 * W + (W // 2 + 1 if W // 2 + 1 < W else 0)]


def _pattern(fmt, c, kind, n):
    """n samples (interleaved scalars of the format): c, c (-1)^n, or c i^n"""
    if kind == "const":
        cyc = [c]
    elif kind == "alt":
        cyc = [c, _negated(fmt, c)]
    else:
        cyc = [c, (-c[1], c[0]), (-c[0], -c[1]), (c[1], -c[0])]
    reps = -(-n // len(cyc))
    return np.tile(np.asarray(cyc, _NP[fmt]).reshape(-1), reps)[:2 * n].copy()


def _kinds(fmt, c, W, bluestein):
    kinds = ["const"]
    if not bluestein:
        if _negated(fmt, c) is not None:
            kinds.append("alt")  # bin W / 2: column 0 after the half swap
        if fmt == "cf32" and c != (0.0, 0.0) and W >= 4:
            kinds.append("quarter")  # bin W / 4: column 3 W / 4
    return kinds


def constant_cases(fmt, W, bluestein=False):
    """-> [dict(name, sr, raw, power, col, db, px)]: two rows of every constant / tone of the format at both row shapes.  `power` is
    the peak's exact float32 power, `col` its column; db / px [2, W] are exact at a power-of-two W.  At a Bluestein W (constants only)
    they are exact for silence; otherwise only px[:, col] and the amplitudes (amplitudes_ok) hold."""
    out = []
    half = W // 2
    for c in CONSTANTS[fmt]:
        z = R.to_complex(np.asarray(c, _NP[fmt]), fmt)[0]
        p = power_f32(F32(z.real), F32(z.imag))
        for kind in _kinds(fmt, c, W, bluestein):
            col = {"const": half, "alt": 0, "quarter": (W // 4 + half) % W}[kind]
            for sr in row_shapes(W):
                db = np.full((2, W), db_f32(FLOOR), F32)
                db[:, col] = db_f32(p)
                out.append(dict(name=f"{fmt} {c} {kind} W={W} sr={sr}", sr=sr, raw=_pattern(fmt, c, kind, 2 * sr), power=p, col=col, db=db,
                                px=pixel_f32(db), silent=bool(p == FLOOR)))
    return out


def amplitudes_ok(db, want_db):
    """criterion (a) of spectrogram_ref.check_parity against an exact expectation: amplitudes within 1e-5 of the row's peak -> the worst
    ratio"""
    got = np.sqrt(10.0 ** (np.asarray(db, np.float64) / 10.0))
    want = np.sqrt(10.0 ** (np.asarray(want_db, np.float64) / 10.0))
    return (np.abs(got - want).max(axis=1) / want.max(axis=1)).max()


# ----------------------------------------------------------------------------------------------------- NaN samples
NAN_WIDTHS = [64, 100]
NAN_WIDE = [16384, 20000]
NAN_BITS = [0x7FC00000, 0xFFC00001]  # the default quiet NaN; one with the sign set and a payload


def nan_case(W, bits):
    """cf32, F = 3 with a skip of W // 2 + 1, four rows of `signal`: row 0 clean; row 1 one NaN (re) in its second transform; row 2 a
    NaN only among the skipped samples; row 3 a NaN in every transform.  -> dict(sr, raw, zeroed: the same with the skipped NaN
    replaced by 0, at: the sample index of row 1's NaN, pieces: feed lengths that put that sample last in a feed, first in a feed and
    inside the carry)"""
    sr = 3 * W + W // 2 + 1
    raw = R.signal("cf32", 4 * sr, W, seed=4099 * W + 1)
    at = sr + W + W // 3
    skipped = 2 * sr + 3 * W + 1
    for pos in [at, skipped] + [3 * sr + t * W + W // 3 + t for t in range(3)]:
        raw.view(np.uint32)[2 * pos] = bits
    zeroed = raw.copy()
    zeroed[2 * skipped] = 0.0
    return dict(sr=sr, raw=raw, zeroed=zeroed, at=at, pieces=[[at + 1], [at], [at + 5]])


def exact_powers():
    """every finite power whose dB the GPU tests assert bit for bit: the ladder's, the constants' peaks, the floor"""
    p = [ladder()[1], [FLOOR]]
    for fmt in CONSTANTS:
        p.append([c["power"] for c in constant_cases(fmt, 4)])
    p = np.unique(np.concatenate([np.asarray(a, F32) for a in p]))
    return p[np.isfinite(p)]
