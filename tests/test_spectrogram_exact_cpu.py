"""CPU tests (-m "not gpu") of tests/spectrogram_exact.py: the float32 restatement behind the exact GPU tests still decodes to the
reference's goldens, its logarithm is the correctly rounded one wherever a test asserts bits, and every case list holds what it is for.
All counted against the restatement alone, never against a GPU result."""
import os

import numpy as np
import pytest

import spectrogram_exact as E
import spectrogram_ref as R
from conftest import GOLDEN


@pytest.mark.parametrize("fmt,W,name", [("cu8", 64, "cu8"), ("cs16", 64, "cs16"), ("cf32", 64, "cf32"), ("cf32", 63, "cf32_odd")])
def test_fmax_and_float32_db_still_decode_to_the_goldens(fmt, W, name):
    """the restatement with its maximum by fmax, then db_f32 / pixel_f32 in place of the float64 logarithm: the four golden PNGs pixel
    for pixel"""
    golden = R.decode_png(os.path.join(GOLDEN, f"spectrogram_{name}.png"))
    p = R.power_rows(R.to_complex(R.reference_input(fmt), fmt), 128, W)
    px = E.pixel_f32(R.shifted(E.db_f32(p.astype(np.float32))))
    assert np.array_equal(px, golden)
    assert np.array_equal(R.spectrogram(R.reference_input(fmt), fmt, 128, W)[1], golden)


def test_log10_rounds_once_at_every_asserted_power():
    """for every power whose dB a GPU test asserts bit for bit: the float64 route and a long double route round to the same float32, and
    the float64 logarithm is more than 8 of its ulps from a float32 rounding midpoint -- so a double log10 a few ulps off (the
    device's) lands on the same float32 too"""
    assert np.longdouble(1) + np.longdouble(2) ** -60 != 1  # (a long double wider than float64: a second opinion, not the same route)
    p = E.exact_powers()
    a, b = E.log10_f32(p), E.log10_f32(p, via=np.longdouble)
    margin = E.midpoint_margin(p)
    print(f"exact powers: {p.size}; float64 and long double routes differ at {(a.view(np.uint32) != b.view(np.uint32)).sum()}; "
          f"hazards (within 8 float64 ulps of a midpoint): {(margin <= 8).sum()}; smallest margin {margin.min():.3g} ulps")
    assert p.size >= 1500
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert np.all(margin > 8)
    # what the warning in log10_f32 is about: numpy's float32 log10 is not that function
    with np.errstate(divide="ignore"):
        off = (np.log10(p).view(np.uint32) != a.view(np.uint32)).sum()
    print(f"numpy's float32 log10 differs from the correctly rounded one at {off} of {p.size}")


def test_ladder_holds_both_sides_of_every_pixel_boundary():
    raw, p, db, px = E.ladder()
    d = db[:, 0].astype(np.float64)
    print(f"ladder rows: {p.size}")
    assert raw.size == 2 * p.size and 1500 <= p.size <= 4000
    fin = np.isfinite(d)
    for k in range(-200, 5):
        above = d[fin & (d >= k)]
        assert above.size and above.min() - k < 1e-3, k
        if k > -200:  # (no power undercuts the floor: nothing lies below -200.0, and -200.0 itself is there)
            below = d[d < k]
            assert below.size and k - below.max() < 1e-3, k
    assert d.min() == -200.0
    # every pixel a power >= 1e-20 can give
    assert set(np.unique(px)) == set(range(55, 256))
    # the upper clamp from both sides of 255.0: a sum of exactly 255.0, sums above it, +Inf; 254 right below
    f = db[:, 0] + np.float32(255)
    assert np.any(f == 255) and np.any((f > 255) & np.isfinite(f)) and np.any(np.isposinf(f))
    assert np.all(px[f >= 255] == 255) and px[f < 255].max() == 254
    assert np.any((d < 0) & (f == 255))  # power 0.99999994: dB -2.6e-7, pixel 255
    # the floor: samples whose power the + 1e-20f absorbs
    assert np.sum(p == E.FLOOR) >= 2 and np.all(px[p == E.FLOOR] == 55)
    # sums of two products
    assert np.sum(raw[1::2] != 0) >= 100


@pytest.mark.parametrize("fmt", ["cu8", "cs16", "cf32"])
def test_constants_reach_the_clamp_and_the_floor(fmt):
    counts = {"peak255": 0, "floor55": 0, "silent": 0}
    for W in E.PLAIN_WIDTHS + E.PLAIN_WIDE:
        cases = E.constant_cases(fmt, W)
        assert len({c["name"] for c in cases}) == len(cases)
        for c in cases:
            assert c["raw"].size == 4 * c["sr"] and c["db"].shape == (2, W)
            off = np.ones(W, bool)
            off[c["col"]] = False
            assert np.all(c["db"][:, off].view(np.uint32) == np.float32(-200.0).view(np.uint32)) and np.all(c["px"][:, off] == 55)
            peak = c["px"][:, c["col"]]
            assert np.all(peak == 255) if c["power"] >= 1 else np.all((peak >= 55) & (peak < 255) & (peak == peak[0]))
            assert np.all(peak == 55) == c["silent"]
            counts["peak255"] += int(c["power"] >= 1)
            counts["floor55"] += 1
            counts["silent"] += int(c["silent"])
    print(fmt, counts)
    assert counts["peak255"] > 0 and counts["floor55"] > 0
    assert counts["silent"] > 0 or fmt == "cu8"  # (cu8 has no silence: 127 and 128 are its nearest)
    by_name = {c["name"]: c for c in E.constant_cases(fmt, 64)}
    if fmt == "cu8":
        c = by_name["cu8 (127, 127) const W=64 sr=64"]
        assert c["power"] == np.float32(2.0 ** -15) and c["px"][0, 32] == 209
    if fmt == "cs16":
        c = by_name["cs16 (-32768, -32768) const W=64 sr=64"]
        assert c["power"] == 2.0 and c["db"][0, 32] == np.float32(3.0103002) and c["px"][0, 32] == 255
        assert by_name["cs16 (1, 1) alt W=64 sr=64"]["px"][0, 0] == 167
    if fmt == "cf32":
        assert by_name["cf32 (1.0, 1.0) quarter W=64 sr=225"]["col"] == 48


def test_bluestein_peaks_stay_clear_of_a_pixel_boundary():
    """at a Bluestein width the peak's power is the exact one to about 1e-6: its pixel can be asserted where the exact dB is not within
    1e-3 of an integer"""
    for fmt in E.CONSTANTS:
        for c in E.constant_cases(fmt, 100, bluestein=True):
            if not c["silent"]:
                d = float(c["db"][0, c["col"]])
                assert abs(d - round(d)) > 1e-3, (c["name"], d)
                assert c["col"] == 50


@pytest.mark.parametrize("bits", E.NAN_BITS)
def test_restatement_follows_fmaxf_on_the_nan_cases(bits):
    """a transform with a NaN sample is all NaN and drops out of its row's maximum; a row of such transforms stays at -255: dB NaN,
    pixel 0"""
    W = 64
    c = E.nan_case(W, bits)
    sr, raw = c["sr"], c["raw"]
    assert np.isnan(raw).sum() == 5 and np.isnan(c["zeroed"]).sum() == 4
    assert sr + W <= c["at"] < sr + 2 * W - 5 and all(n[0] < raw.size // 2 for n in c["pieces"])
    db, px, _ = R.spectrogram(raw, "cf32", sr, W)
    assert db.shape == (4, W) and np.all(np.isfinite(db[:3])) and np.all(np.isnan(db[3])) and np.all(px[3] == 0)
    clean = np.where(np.isnan(raw), np.float32(0), raw)
    x = R.to_complex(clean, "cf32")[sr:2 * sr]
    two = np.concatenate([x[:W], x[2 * W:3 * W]])  # row 1's first and third transform as a row of F = 2
    want = R.shift_db(R.power_rows(two, 2 * W, W))
    assert np.array_equal(db[1], want[0])
    assert np.array_equal(db[[0, 2]], R.spectrogram(clean, "cf32", sr, W)[0][[0, 2]])
