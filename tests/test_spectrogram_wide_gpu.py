"""GPU tests (-m gpu) of the spectrogram's widths above 8192 (xlating_spectrum_create_wide, spectrogram_main_wide, sdr_spectrogram -W):
the two-level transform of sdr-server_amd/csrc/xl_spectrum_wide.hip against the float64 restatement (tests/spectrogram_ref.py, its
check_parity unchanged) at every transform length once, plain and Bluestein; exact cases; the same object below the cap; bit-identical
rows under any split of the input, any scratch size and from device memory; the file path and the command line."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import sdr_server_amd as xl
import spectrogram_ref as R
from conftest import ROOT
from spectrogram_ref import signal

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "sdr-server_amd", "bin", "sdr_spectrogram")
_PIXELS = {"total": 0, "equal": 0}


def check_parity(db, px, raw, fmt, sr, W):
    """R.check_parity's criteria; its pixel counts go into the aggregate of test_pixel_agreement_wide.  Prints the (a) ratio first."""
    _, _, amp = R.spectrogram(raw, fmt, sr, W)
    if db.shape == amp.shape:
        want = R.shifted(amp)
        err = np.abs(np.sqrt(10.0 ** (db.astype(np.float64) / 10.0)) - want).max(axis=1) / want.max(axis=1)
        print(f"wide parity {fmt} W={W} sr={sr}: worst (a) ratio {err.max():.3e}")
    total, equal = R.check_parity(db, px, raw, fmt, sr, W)
    print(f"wide parity {fmt} W={W} sr={sr}: {total - equal} of {total} pixels differ")
    _PIXELS["total"] += total
    _PIXELS["equal"] += equal


def run_spectrum(raw, fmt, sr, W, wide=True, pieces=None):
    """rows of the whole recording; pieces: sample counts to feed one by one (the rest in a last feed), rows taken between feeds"""
    s = xl.Spectrum(sr, W, fmt, wide=wide)
    parts_db, parts_px, pos = [], [], 0
    for n in list(pieces or []) + [raw.size // 2]:
        end = min(pos + n, raw.size // 2)
        if end > pos:
            s.feed(raw[2 * pos:2 * end])
            d, p = s.take_rows()
            parts_db.append(d)
            parts_px.append(p)
        pos = end
    s.close()
    return np.concatenate(parts_db), np.concatenate(parts_px)


def same(a, b):
    return a[0].shape == b[0].shape and np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1], b[1])


def parity_shapes(fmt, W, with_skip):
    """F = 1 (sampling_rate = W, 2 rows and a partial one) and, with_skip, F = 3 with a skip of W // 2 + 1"""
    for k, sr in enumerate([W] + ([3 * W + W // 2 + 1] if with_skip else [])):
        raw = signal(fmt, sr * 2 + sr // 3, W, seed=(1000 * W + k) % (1 << 32))
        db, px = run_spectrum(raw, fmt, sr, W)
        assert db.shape[0] == 2
        check_parity(db, px, raw, fmt, sr, W)


# ------------------------------------------------------------------------------------------------------------ parity
PLAIN = [("cf32", 1 << e) for e in range(14, 21)] + [(f, W) for f in ("cu8", "cs16") for W in (1 << 14, 1 << 20)]


@pytest.mark.parametrize("fmt,W", PLAIN)
def test_parity_plain(fmt, W):
    """every transform length 2^14 .. 2^20 (every split N1 x N2 of the plain path) once"""
    parity_shapes(fmt, W, with_skip=W in (1 << 14, 1 << 17))


BLUESTEIN = [("cf32", W) for W in (8193, 16385, 50000, 100000, 200000, 262145, 1048575)] + \
    [(f, W) for f in ("cu8", "cs16") for W in (8193, 1048575)]


@pytest.mark.parametrize("fmt,W", BLUESTEIN)
def test_parity_bluestein(fmt, W):
    """every Bluestein length 2^15 .. 2^21 once"""
    parity_shapes(fmt, W, with_skip=W == 8193)


def test_parity_many_transforms_per_row():
    """F = 200 with a skip: many scratch chunks per span and 200 atomic maxima per bin"""
    fmt, W = "cu8", 16384
    sr = 200 * W + W // 3
    raw = signal(fmt, 2 * sr + 5, W, seed=200)
    check_parity(*run_spectrum(raw, fmt, sr, W), raw, fmt, sr, W)


def test_pixel_agreement_wide():
    """(c): over this file's whole parity matrix, at least 99.9 % of the pixels equal the float64 restatement's"""
    assert _PIXELS["total"] > 0
    print("wide pixel agreement", _PIXELS)
    assert _PIXELS["equal"] >= 0.999 * _PIXELS["total"], _PIXELS


# ------------------------------------------------------------------------------------------------------------ exact cases
@pytest.mark.parametrize("W", [16384, 20000])
def test_all_zero_input(W):
    """zero samples: every power is exactly 1e-20f, every dB 10 log10f(1e-20f) with the host libm's correctly rounded log10f (-200.0
    exactly), every pixel the restatement's 55.  The finishing passes take their log10 in double and round once for this (xl_spec_db):
    the device's own log10f(1e-20f) is -20.000002, which gave -200.00002 and pixel 54 when a pass used it (measured on an MI355X).  The
    object of the widths up to 8192 answered so until it got the same dB function; its silent cases at every width, and the bits of
    10 log10f next to every pixel boundary, are in tests/test_spectrogram_exact_gpu.py."""
    raw = np.zeros(2 * (2 * W + 100), np.float32)
    db, px = run_spectrum(raw, "cf32", W, W)
    assert db.shape == (2, W)
    want = np.float32(10.0) * np.log10(np.float32(1e-20))
    print("zero input", W, "wide", db.min(), db.max(), hex(int(db.view(np.uint32).max())), "host", want, "pixels", px.min(), px.max())
    assert np.all(db.view(np.uint32) == np.float32(want).view(np.uint32))
    assert np.array_equal(px, R.spectrogram(raw, "cf32", W, W)[1])


@pytest.mark.parametrize("W", [16384, 20000])
def test_impulses_at_both_ends(W):
    """an impulse at sample 0 and one at sample W - 1 of every transform: the first and the last column, the first and the last row of
    the split"""
    z = np.zeros((2, W, 2), np.float32)
    z[:, 0, 0] = 1.0
    z[:, W - 1, 0] = 1.0
    raw = np.concatenate([z.reshape(-1), np.zeros(200, np.float32)])
    db, px = run_spectrum(raw, "cf32", W, W)
    R.check_parity(db, px, raw, "cf32", W, W)


# ------------------------------------------------------------------------------------------------------------ below the cap
@pytest.mark.parametrize("W", [100, 8191, 8192])
def test_same_object_below_the_cap(W):
    sr = 2 * W + 3
    raw = signal("cs16", 3 * sr + 11, W, seed=W)
    assert same(run_spectrum(raw, "cs16", sr, W, wide=True), run_spectrum(raw, "cs16", sr, W, wide=False))


def test_default_entry_still_refuses():
    with pytest.raises(xl.XlatingError) as e:
        xl.Spectrum(100000, 8193, "cu8")
    assert e.value.code == -22


# ------------------------------------------------------------------------------------------------------------ splits
@pytest.mark.parametrize("fmt,W", [("cs16", 16384), ("cu8", 8193)])
def test_split_invariance(fmt, W, monkeypatch):
    """F = 2 with a skip, 3 rows: whole, in pieces of 1000 samples (the carry is appended to many times: a piece is shorter than W),
    in seeded random pieces, and through a staging buffer shorter than W"""
    sr = 2 * W + W // 3
    raw = signal(fmt, 3 * sr + 77, W, seed=7)
    whole = run_spectrum(raw, fmt, sr, W)
    assert whole[0].shape == (3, W)
    n = raw.size // 2
    assert same(run_spectrum(raw, fmt, sr, W, pieces=[1000] * (n // 1000)), whole)
    rng = np.random.default_rng(11)
    assert same(run_spectrum(raw, fmt, sr, W, pieces=[int(v) for v in np.concatenate([rng.integers(1, W // 2, 12), rng.integers(W, 2 * W, 2), rng.integers(1, W // 2, 12)])]), whole)
    monkeypatch.setenv("XL_TESTING", "1")
    monkeypatch.setenv("XL_EXP_SPEC_CHUNK", "5000")
    assert same(run_spectrum(raw, fmt, sr, W), whole)


@pytest.mark.parametrize("W,N", [(16384, 16384), (8193, 32768)])
def test_scratch_chunking(W, N, monkeypatch):
    """F = 7, 2 rows, fed a row at a time (7 transforms per launch sequence): a scratch that holds 3 transforms (chunks of 3, 3 and 1)
    and one that holds 1 give the rows of the default scratch"""
    sr = 7 * W
    raw = signal("cf32", 2 * sr, W, seed=5)
    whole = run_spectrum(raw, "cf32", sr, W, pieces=[sr])
    assert whole[0].shape == (2, W)
    monkeypatch.setenv("XL_TESTING", "1")
    for held in (3, 1):
        monkeypatch.setenv("XL_EXP_SPEC_SCRATCH", str(held * 8 * N))
        assert same(run_spectrum(raw, "cf32", sr, W, pieces=[sr]), whole), held


@pytest.mark.parametrize("W", [32768, 50000])
def test_device_feed_matches_host_feed(W):
    import torch

    fmt, sr = "cf32", 2 * W + 100
    raw = signal(fmt, sr * 2 + 999, W, seed=3)
    want = run_spectrum(raw, fmt, sr, W)
    d = torch.from_numpy(raw).cuda()
    st = torch.cuda.current_stream()
    s = xl.Spectrum(sr, W, fmt, wide=True)
    n = raw.size // 2
    for a, b in ((0, 1000), (1000, sr + 17), (sr + 17, n)):  # in place, in three pieces
        s.feed(d.data_ptr() + 8 * a, b - a, st.cuda_stream)
    got = s.take_rows()
    s.close()
    assert same(got, want)


# ------------------------------------------------------------------------------------------------------------ file path and CLI
@pytest.mark.parametrize("W,gz", [(16384, False), (20000, False), (20000, True)])
def test_drop_in_and_cli(tmp_path, W, gz):
    """2 rows plus a tail of a cu8 file: spectrogram_main(wide=True) writes a W x 2 PNG whose pixels meet (c); sdr_spectrogram -W writes
    the same bytes; without -W it refuses and writes nothing"""
    raw = signal("cu8", 2 * W + W // 2, W, seed=W)
    inp, out, out2 = str(tmp_path / ("in.raw.gz" if gz else "in.raw")), str(tmp_path / "a.png"), str(tmp_path / "b.png")
    with (gzip.open(inp, "wb") if gz else open(inp, "wb")) as f:
        f.write(raw.tobytes())
    assert xl.spectrogram_main(inp, out, W, W, "cu8", wide=True) == 0
    px = R.decode_png(out)
    assert px.shape == (2, W)
    want = R.spectrogram(raw, "cu8", W, W)[1]
    d = np.abs(px.astype(np.int32) - want.astype(np.int32))
    assert d.max() <= 1 and (d != 0).sum() <= max(2, px.size // 1000), (d.max(), (d != 0).sum())
    args = [CLI, "-w", str(W), "-s", str(W), "-d", "cu8", "-i", inp, "-o", out2]
    r = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and not os.path.exists(out2), r.stderr
    r = subprocess.run(args + ["-W"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert open(out2, "rb").read() == open(out, "rb").read()
