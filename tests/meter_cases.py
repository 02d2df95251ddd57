"""The rows the power meter's tests measure (tests/test_meter_gpu.py on the device, tests/test_meter_cpu.py against float64), built once.
Lengths around every boundary of the rule: the thread count 256, the piece 2048, two pieces and one sample."""
import functools

import numpy as np

LENS = [0, 1, 2, 3, 255, 256, 257, 2047, 2048, 2049, 4097]
SCALES = [2.0 ** -60, 1.0, 2.0 ** 60]


def _noise(rng, n, scale):
    """magnitudes in [1/4, 1) of the scale, random signs: at 2^-60 every square is still a normal float32 (>= 2^-124), so the bound,
    which assumes no underflow, applies"""
    v = rng.uniform(0.25, 1.0, 2 * n) * rng.choice([-1.0, 1.0], 2 * n) * scale
    v = v.astype(np.float32)
    return (v[0::2] + 1j * v[1::2]).astype(np.complex64)


@functools.lru_cache(maxsize=None)
def cf32_rows():
    """-> [(name, complex64 row, kind)]; kind: "finite" (the bound applies), "maybe" (it applies unless a sum overflows), "zero",
    "subnormal", "nonfinite" """
    rng = np.random.default_rng(41)
    rows = []
    for sc in SCALES:
        for n in LENS:
            # (at 2^60 a piece of 255 samples and more sums to about 2^128, the end of the float32 range: "maybe" finite)
            rows.append((f"noise{np.log2(sc):+.0f}_{n}", _noise(rng, n, sc), "zero" if n == 0 else "maybe" if sc > 1 and n >= 255 else "finite"))
    rows.append(("zeros_4097", np.zeros(4097, np.complex64), "zero"))
    rows.append(("subnormal_2049", _noise(rng, 2049, 2.0 ** -70), "subnormal"))  # squares near 2^-140
    x = _noise(rng, 4097, 1.0)
    x[-1] = np.complex64(complex(float("nan"), 0.5))  # the last piece holds this one sample
    rows.append(("nan_4097", x, "nonfinite"))
    rows.append(("after_nan_257", _noise(rng, 257, 1.0), "finite"))
    x = _noise(rng, 2049, 1.0)
    x[-1] = np.complex64(complex(0.5, float("inf")))
    rows.append(("inf_2049", x, "nonfinite"))
    rows.append(("after_inf_3", _noise(rng, 3, 1.0), "finite"))
    rows.append(("overflow_300", _noise(rng, 300, 2.0 ** 100), "nonfinite"))  # squares above the float32 range
    for _, r, _k in rows:
        r.setflags(write=False)
    return rows


@functools.lru_cache(maxsize=None)
def cs16_rows():
    """-> [(name, int16 [n, 2] row, exact power or None)]"""
    rng = np.random.default_rng(42)
    rows = [(f"noise_{n}", rng.integers(-32768, 32768, (n, 2)).astype(np.int16), None) for n in LENS]
    rows.append(("min_4097", np.full((4097, 2), -32768, np.int16), 2.0))
    rows.append(("max_2049", np.full((2049, 2), 32767, np.int16), 2.0 * 32767.0 ** 2 / 2.0 ** 30))
    rows.append(("zeros_257", np.zeros((257, 2), np.int16), 0.0))
    rows.append(("small_2048", rng.integers(-3, 4, (2048, 2)).astype(np.int16), None))
    for _, r, _p in rows:
        r.setflags(write=False)
    return rows
