"""GPU tests (-m gpu) of the spectrogram (include/xlating_spectrum.h, include/spectrogram.h, bin/sdr_spectrogram): the reference test's
goldens through spectrogram_main and the CLI, parity with the float64 restatement (tests/spectrogram_ref.py) over widths, formats and
row shapes, bit-identical rows under any split of the input and from device memory, and no interference with the batch engine."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import sdr_server_amd as xl
import siggen
import spectrogram_ref as R
from conftest import GOLDEN, ROOT
from spectrogram_ref import signal

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "sdr-server_amd", "bin", "sdr_spectrogram")
GOLDEN_CASES = [("cu8", 64, "cu8"), ("cs16", 64, "cs16"), ("cf32", 64, "cf32"), ("cf32", 63, "cf32_odd")]


def _write(path, raw, gz=False):
    data = np.ascontiguousarray(raw).tobytes()
    if gz:
        with gzip.open(path, "wb") as f:
            f.write(data)
    else:
        with open(path, "wb") as f:
            f.write(data)


@pytest.mark.parametrize("gz", [False, True], ids=["plain", "gz"])
@pytest.mark.parametrize("fmt,W,name", GOLDEN_CASES)
def test_reference_goldens(tmp_path, fmt, W, name, gz):
    """test/test_spectrogram.c:14-60: 256 samples at sampling_rate 128, decoded pixels equal to the reference's PNGs."""
    inp = str(tmp_path / ("input.raw.gz" if gz else "input.raw"))
    out = str(tmp_path / "spectrogram.png")
    _write(inp, R.reference_input(fmt), gz)
    assert xl.spectrogram_main(inp, out, W, 128, fmt) == 0
    assert np.array_equal(R.decode_png(out), R.decode_png(os.path.join(GOLDEN, f"spectrogram_{name}.png")))


def test_unsupported_fftw_flag_falls_back(tmp_path, capfd):
    """test_spectrogram.c:34-37: an unknown fftw flag is reported and the image is the same."""
    inp, out = str(tmp_path / "input.raw"), str(tmp_path / "spectrogram.png")
    _write(inp, R.reference_input("cf32"))
    assert xl.spectrogram_main(inp, out, 63, 128, "cf32", "unsupported") == 0
    assert "unsupported fftw flag: unsupported. Fallback to FFTW_ESTIMATE" in capfd.readouterr().err
    assert np.array_equal(R.decode_png(out), R.decode_png(os.path.join(GOLDEN, "spectrogram_cf32_odd.png")))


def test_cli_golden(tmp_path):
    inp, out = str(tmp_path / "input.raw.gz"), str(tmp_path / "spectrogram.png")
    _write(inp, R.reference_input("cs16"), gz=True)
    r = subprocess.run([CLI, "-w", "64", "-s", "128", "-d", "cs16", "-i", inp, "-o", out, "-f", "FFTW_ESTIMATE"], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert np.array_equal(R.decode_png(out), R.decode_png(os.path.join(GOLDEN, "spectrogram_cs16.png")))


# ------------------------------------------------------------------------------------------------------------ parity
_PIXELS = {"total": 0, "equal": 0}


def check_parity(db, px, raw, fmt, sr, W):
    """R.check_parity's criteria; its pixel counts go into the aggregate of test_pixel_agreement"""
    total, equal = R.check_parity(db, px, raw, fmt, sr, W)
    _PIXELS["total"] += total
    _PIXELS["equal"] += equal


def run_spectrum(raw, fmt, sr, W):
    s = xl.Spectrum(sr, W, fmt)
    s.feed(raw)
    db, px = s.take_rows()
    s.close()
    return db, px


WIDTHS = [1, 2, 3, 63, 64, 100, 509, 1000, 1024, 4096, 8191, 8192]


@pytest.mark.parametrize("fmt", ["cu8", "cs16", "cf32"])
@pytest.mark.parametrize("W", WIDTHS)
def test_parity_small_rows(fmt, W):
    """rows of F = 1 (sampling_rate = W, no skip) and of F = 3 with a skip (S = W // 2 + 1 when that stays below W)"""
    for k, (sr, rows) in enumerate(((W, 3), (3 * W + (W // 2 + 1 if W > 1 else 0), 2))):
        raw = signal(fmt, sr * rows + (sr // 3), W, seed=1000 * W + k)
        check_parity(*run_spectrum(raw, fmt, sr, W), raw, fmt, sr, W)


@pytest.mark.parametrize("fmt,W,F", [("cu8", 64, 4000), ("cf32", 1000, 1500), ("cs16", 1024, 1200), ("cf32", 8192, 60)])
def test_parity_long_rows(fmt, W, F):
    """F in the thousands (many workgroups and atomics per row), with a skip"""
    sr = F * W + W // 3
    raw = signal(fmt, 2 * sr + 5, W, seed=F)
    check_parity(*run_spectrum(raw, fmt, sr, W), raw, fmt, sr, W)


def test_pixel_agreement():
    """(c): over the whole parity matrix, at least 99.9 % of the pixels equal the float64 restatement's"""
    assert _PIXELS["total"] > 0
    assert _PIXELS["equal"] >= 0.999 * _PIXELS["total"], _PIXELS


# ------------------------------------------------------------------------------------------------------------ split invariance
SPLIT_CASES = [("cu8", 100, 64 * 37 + 19), ("cf32", 64, 64 * 50 + 33), ("cs16", 1000, 3 * 1000 + 7)]


@pytest.mark.parametrize("fmt,W,sr", SPLIT_CASES)
def test_split_invariance(fmt, W, sr, monkeypatch, tmp_path):
    raw = signal(fmt, sr * 5 + 123, W, seed=7)
    db0, px0 = run_spectrum(raw, fmt, sr, W)
    assert db0.shape[0] == 5
    # pieces that cut transforms and rows at odd places (in samples), fed one by one; rows taken between feeds
    rng = np.random.default_rng(11)
    cuts = np.unique(np.concatenate([rng.integers(1, raw.size // 2, 25), [1, 2, W - 1, W + 1, sr - 1, sr, sr + 1, 2 * sr + W // 2]]))
    s = xl.Spectrum(sr, W, fmt)
    parts_db, parts_px = [], []
    prev = 0
    for c in list(cuts) + [raw.size // 2]:
        s.feed(raw[2 * prev:2 * c])
        prev = c
        d, p = s.take_rows()
        parts_db.append(d)
        parts_px.append(p)
    s.close()
    assert np.array_equal(np.concatenate(parts_db).view(np.uint32), db0.view(np.uint32))
    assert np.array_equal(np.concatenate(parts_px), px0)
    # a small staging size: every host feed is cut into many spans, and the row store grows (rows are taken only at the end)
    monkeypatch.setenv("XL_EXP_SPEC_CHUNK", "777")
    db1, px1 = run_spectrum(raw, fmt, sr, W)
    assert np.array_equal(db1.view(np.uint32), db0.view(np.uint32)) and np.array_equal(px1, px0)
    # the file path (reader thread, pinned buffers) gives the same pixels
    inp, out = str(tmp_path / "in.raw"), str(tmp_path / "out.png")
    _write(inp, raw)
    assert xl.spectrogram_main(inp, out, W, sr, fmt) == 0
    assert np.array_equal(R.decode_png(out), px0)
    monkeypatch.delenv("XL_EXP_SPEC_CHUNK")
    assert xl.spectrogram_main(inp, out, W, sr, fmt) == 0
    assert np.array_equal(R.decode_png(out), px0)


def test_device_feed_matches_host_feed():
    import torch

    fmt, W, sr = "cf32", 1024, 1024 * 7 + 100
    raw = signal(fmt, sr * 4 + 999, W, seed=3)
    db0, px0 = run_spectrum(raw, fmt, sr, W)
    d = torch.from_numpy(raw).cuda()
    st = torch.cuda.current_stream()
    s = xl.Spectrum(sr, W, fmt)
    n = raw.size // 2
    for a, b in ((0, 1000), (1000, sr + 17), (sr + 17, n)):  # in place, in three pieces
        s.feed(d.data_ptr() + 8 * a, b - a, st.cuda_stream)
    db1, px1 = s.take_rows()
    s.close()
    assert np.array_equal(db1.view(np.uint32), db0.view(np.uint32)) and np.array_equal(px1, px0)


def test_beside_the_batch_engine():
    """config 5's shape (cf32, D = 100, 257 taps, 64 clients: the two-half matrix-core mix) and a Spectrum fed the same device
    super-blocks on the same stream: each one's results are bit-identical to a run without the other."""
    import torch

    taps = siggen.hamming_sinc(257, 0.004)
    nsamp = 131072
    fcs = [-4900000 + (9800000 // 64) * c for c in range(64)]
    blocks = [signal("cf32", nsamp, 64, seed=50 + k) for k in range(3)]
    dev = [torch.from_numpy(b).cuda() for b in blocks]
    st = torch.cuda.current_stream()

    def run(with_engine, with_spec):
        eng = spec = None
        outs, rows = [], []
        if with_engine:
            eng = xl.BatchEngine(10000000, "cf32", 2 * nsamp)
            ids = [eng.add_client(100, taps, fc) for fc in fcs]
        if with_spec:
            spec = xl.Spectrum(10000, 1000, "cf32")
        for d in dev:
            if eng:
                eng.process_device(d.data_ptr(), 2 * nsamp, "optimized", st.cuda_stream)
            if spec:
                spec.feed(d.data_ptr(), nsamp, st.cuda_stream)
            if eng:
                eng.fetch()
                outs.append([eng.output(c).copy() for c in ids])
            if spec:
                rows.append(spec.take_rows()[0])
        if eng:
            assert "mix=mfma" in eng.describe(), eng.describe()
            eng.close()
        if spec:
            spec.close()
        return outs, rows

    outs_alone, _ = run(True, False)
    _, rows_alone = run(False, True)
    outs_both, rows_both = run(True, True)
    for a, b in zip(outs_alone, outs_both):
        for x, y in zip(a, b):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    for a, b in zip(rows_alone, rows_both):
        assert a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))
