"""The numpy restatement of the narrowing delivery's rule (sdr-server_amd/csrc/xl_dlv_narrow.h, xlating_delivery_pack_device_cs16):
float32 -> int16 as clamp(rint(float64(y) * 32768), -32768, 32767), NaN -> 0.  The product is exact in float64 and np.rint rounds to
nearest, ties to even.  tests/test_delivery_narrow_cpu.py pins it to a table of exact cases; the C rule is held to the same statement in
libm on all 2^32 bit patterns (tests/c/delivery_narrow_sweep.c); the GPU tests compare the kernel's bytes with narrow() of the sources."""
import numpy as np

F32 = np.float32
LSB = 2.0 ** -15


def _b(y):
    """the bits of float32(y)"""
    return int(np.array([y], np.float32).view(np.uint32)[0])


def _next(y, toward):
    return np.nextafter(F32(y), F32(toward), dtype=np.float32)


FLT_MAX = np.finfo(np.float32).max
# (bits of the float32, int16 expected): the exact cases.  NaNs are given as bits, so that no arithmetic ever quiets a signalling one;
# a multiple of half an LSB below 2^16 LSB is an exact float32.
EXACT = [
    (_b(0.0), 0), (_b(-0.0), 0),
    (_b(2.0 ** -16), 0), (_b(-2.0 ** -16), 0),  # half an LSB: a tie, to the even 0
    (_b(_next(2.0 ** -16, 1)), 1), (_b(_next(2.0 ** -16, 0)), 0), (_b(_next(-2.0 ** -16, -1)), -1), (_b(_next(-2.0 ** -16, 0)), 0),
    (_b(1.5 * LSB), 2), (_b(-1.5 * LSB), -2), (_b(2.5 * LSB), 2), (_b(-2.5 * LSB), -2),
    (_b(32766.5 * LSB), 32766), (_b(-32766.5 * LSB), -32766),
    (_b(32767.5 * LSB), 32767), (_b(-32767.5 * LSB), -32768),  # ties to the even 32768: clamped on the positive side only
    (_b(1.0), 32767), (_b(-1.0), -32768),
    (_b(-32768.5 * LSB), -32768),
    (_b(256.0), 32767), (_b(_next(256.0, 0)), 32767),
    (_b(FLT_MAX), 32767), (_b(-FLT_MAX), -32768),
    (0x7F800000, 32767), (0xFF800000, -32768),  # +-Inf
    (0x7FC00000, 0), (0xFFC00000, 0), (0x7FC12345, 0),  # quiet NaNs
    (0x7F800001, 0), (0xFF800001, 0), (0x7FA00000, 0), (0xFFBFFFFF, 0),  # signalling NaNs
    (0x00000001, 0), (0x80000001, 0), (0x007FFFFF, 0), (0x807FFFFF, 0),  # the smallest and the largest denormal
]


def exact_values():
    """the table's inputs as a float32 array (a view of the bits)"""
    return np.array([v for v, _ in EXACT], np.uint32).view(np.float32)


def exact_expected():
    return np.array([w for _, w in EXACT], np.int16)


def narrow(y):
    """float32 array (any shape; complex64 is read as its re, im pairs) -> int16 array of the same float shape"""
    y = np.ascontiguousarray(y)
    if y.dtype == np.complex64:
        y = y.view(np.float32)
    assert y.dtype == np.float32
    with np.errstate(invalid="ignore", over="ignore"):
        r = np.rint(y.astype(np.float64) * 32768.0)
        r = np.where(np.isnan(r), 0.0, np.clip(r, -32768.0, 32767.0))
    return r.astype(np.int16)


def narrow_bytes(y):
    """the delivered row of a cf32 row: bytes"""
    return narrow(y).tobytes()
