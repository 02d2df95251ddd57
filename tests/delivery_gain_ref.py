"""The numpy restatement of the narrowing delivery's rule with a gain (sdr-server_amd/csrc/xl_dlv_gain.h,
xlating_delivery_pack_device_cs16_gain) and of a delivered row's level: float32 y and a gain g in -48 .. 48 -> int16 as
clamp(rint(float64(y) * 2.0 ** (15 + g)), -32768, 32767), NaN -> 0.  The product is exact in float64 for every admitted g and every
finite float32: a power of two times a 24-bit significand, between 2^-149 * 2^-33 and 2^128 * 2^63, far inside float64's range at
either end.  np.rint rounds to nearest, ties to even.  The levels are restated in numpy integers.  tests/test_delivery_gain_cpu.py pins narrow() to a table of exact
cases; the C rule is held to the same statement in libm (tests/c/delivery_gain_sweep.c); the GPU tests compare the kernel's bytes and
levels with these functions applied to the sources."""
import numpy as np

import delivery_narrow_ref as NR

GAIN_MIN, GAIN_MAX = -48, 48
PINNED_GAINS = (1, -1, 9, -9, 48, -48)


def _floats(y):
    y = np.ascontiguousarray(y)
    if y.dtype == np.complex64:
        y = y.view(np.float32)
    assert y.dtype == np.float32
    return y


def _rounded(y, g):
    """float64: rint(y * 2^(15 + g)), NaN where y is NaN"""
    assert GAIN_MIN <= int(g) <= GAIN_MAX
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        return np.rint(_floats(y).astype(np.float64) * 2.0 ** (15 + int(g)))


def narrow(y, g=0):
    """float32 array (any shape; complex64 is read as its re, im pairs), one gain -> int16 array of the same float shape"""
    r = _rounded(y, g)
    with np.errstate(invalid="ignore"):
        r = np.where(np.isnan(r), 0.0, np.clip(r, -32768.0, 32767.0))
    return r.astype(np.int16)


def narrow_bytes(y, g=0):
    """the delivered row of a cf32 row under gain g: bytes"""
    return narrow(y, g).tobytes()


def level(y, g=0):
    """-> (peak_bits, clipped, nans) of a row, in integers: the largest bits & 0x7FFFFFFF among the floats that are no NaN (0 if there
    is none); the floats whose rounded value lies outside -32768 .. 32767 (an Inf does, a NaN does not); the NaN floats"""
    bits = _floats(y).reshape(-1).view(np.uint32)
    mag = bits & np.uint32(0x7FFFFFFF)
    nan = mag > np.uint32(0x7F800000)
    r = _rounded(y, g).reshape(-1)
    with np.errstate(invalid="ignore"):
        clipped = (~nan) & ((r > 32767.0) | (r < -32768.0))
    peak = int(mag[~nan].max()) if (~nan).any() else 0
    return peak, int(clipped.sum()), int(nan.sum())


def undo(i16, g):
    """int16 delivered under gain g -> float64, exactly: i * 2^-(15 + g)"""
    return np.asarray(i16).astype(np.float64) * 2.0 ** -(15 + int(g))


def exact_table(g):
    """(bits of the float32, int16 expected) at gain g: delivery_narrow_ref.EXACT with every input scaled by 2^-g where that is exact
    -- a finite, normal float32 whose exponent stays in the normal range -- so that y * 2^(15 + g) is the table's y * 2^15 and the
    expected value is the table's; NaNs and Infs stand as they are (no scale moves them); the rest (zeros go as they are; denormals,
    and values the scaling would push out of the normal range) are left out at g != 0"""
    out = []
    for bits, want in NR.EXACT:
        e = (bits >> 23) & 0xFF
        if g == 0 or e == 0xFF or (bits & 0x7FFFFFFF) == 0:
            out.append((bits, want))
        elif e != 0 and 1 <= e - g <= 254:
            out.append((bits - (g << 23), want))  # the exponent field lowered by g: y * 2^-g, exactly
    return out
