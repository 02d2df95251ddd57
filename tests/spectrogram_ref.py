"""Test oracle of the spectrogram: the reference's sdr_spectrogram restated in numpy float64, a PNG decoder and the reference test's
input generators.  Citations point into the reference tree (src/spectrogram/*, test/utils.c).

The restatement runs each FFT in float64 on the float32-converted samples; it reproduces the reference's four golden PNGs pixel for
pixel (tests/test_spectrogram_cpu.py).  The last section is what the GPU tests of the single object and of the bank share: their
seeded signal and the parity criteria against the restatement."""
import struct
import zlib

import numpy as np

SAMPLE_BYTES = {"cu8": 2, "cs16": 4, "cf32": 8}


def to_complex(raw, fmt):
    """iq_file.c:142-143 (cu8: (b - 127.5f) / 128.0f), :167-168 (cs16 little-endian / 32768.0f), cf32 as stored; float32 values,
    returned as complex128."""
    raw = np.asarray(raw)
    if fmt == "cu8":
        v = (raw.astype(np.uint8).astype(np.float32) - np.float32(127.5)) / np.float32(128.0)
    elif fmt == "cs16":
        v = raw.astype("<i2").astype(np.float32) / np.float32(32768.0)
    elif fmt == "cf32":
        v = raw.astype(np.float32)
    else:
        raise ValueError(fmt)
    v = v.reshape(-1, 2).astype(np.float64)
    return v[:, 0] + 1j * v[:, 1]


def power_rows(x, sampling_rate, width):
    """spectrogram.c:84-148: row r is samples r * sampling_rate ..; its F = sampling_rate // width transforms of `width` samples
    (the S = sampling_rate % width after them skipped, :154), each bin's power |X / W|^2 + 1e-20 (:140-142), the maximum over the
    row's transforms (:148: fmaxf(temp[j], power) from -255, which no power undercuts and against which a NaN power loses: a transform
    that holds a NaN sample does not contribute to its row, and a row of such transforms only stays at -255).
    Height = samples // sampling_rate (:93)."""
    W, sr = width, sampling_rate
    F = sr // W
    H = x.size // sr
    rows = x[:H * sr].reshape(H, sr)[:, :F * W].reshape(H, F, W)
    with np.errstate(invalid="ignore"):
        X = np.fft.fft(rows, axis=2) / W
        p = X.real ** 2 + X.imag ** 2 + 1e-20
    return np.fmax.reduce(p, axis=1, initial=-255.0)


def shift_db(p):
    """spectrogram.c:150-158: 10 log10 per bin, halves of half = W // 2 swapped; an odd W's last bin stays last."""
    W = p.shape[1]
    half = W // 2
    with np.errstate(invalid="ignore"):  # (a row left at -255: NaN, as log10f(-255) in the reference)
        d = 10.0 * np.log10(p)
    out = d.copy()
    out[:, :half] = d[:, half:2 * half]
    out[:, half:2 * half] = d[:, :half]
    return out


def pixels(db):
    """png_util.c:53-63: (int)(dB + 255) clamped to [0, 255] (the sum in float32 as in the reference: float + int)."""
    f = np.asarray(db, dtype=np.float32) + np.float32(255)
    with np.errstate(invalid="ignore"):
        v = np.where(f >= 255, 255, np.where(f > 0, np.trunc(f), 0))
    return v.astype(np.uint8)


def spectrogram(raw, fmt, sampling_rate, width):
    """(db float64 [H, W], pixels uint8 [H, W], amplitudes sqrt(p) float64 [H, W] in bin order) of a raw recording."""
    p = power_rows(to_complex(raw, fmt), sampling_rate, width)
    db = shift_db(p)
    with np.errstate(invalid="ignore"):
        amp = np.sqrt(p)
    return db, pixels(db), amp


# ----------------------------------------------------------------------------------------------------- inputs of test/utils.c:137-174
def input_cu8(n_scalars):
    """setup_input_cu8: (uint8_t)(i)"""
    return (np.arange(n_scalars) & 0xFF).astype(np.uint8)


def input_cs16(n_scalars):
    """setup_input_cs16: (int16_t)(i) - (int16_t)(len / 2)"""
    return (np.arange(n_scalars).astype(np.int16) - np.int16(n_scalars // 2)).astype(np.int16)


def input_cf32(n_scalars):
    """setup_input_cf32: sinf((float) i)"""
    return np.sin(np.arange(n_scalars, dtype=np.float32)).astype(np.float32)


def reference_input(fmt, samples=256):
    """the reference test's recording (test/utils.c setup_file: 2 * len scalars)"""
    return {"cu8": input_cu8, "cs16": input_cs16, "cf32": input_cf32}[fmt](2 * samples)


# ----------------------------------------------------------------------------------------------------- PNG decoding (8-bit gray)
def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    if pa <= pb and pa <= pc:
        return a
    return b if pb <= pc else c


def decode_png(data):
    """-> uint8 [H, W] of a non-interlaced 8-bit grayscale PNG; chunk CRCs checked, filter types 0-4."""
    if isinstance(data, str):
        with open(data, "rb") as f:
            data = f.read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n", "not a PNG"
    pos, idat, hdr, seen_end = 8, b"", None, False
    while pos < len(data):
        (n,) = struct.unpack(">I", data[pos:pos + 4])
        typ, body = data[pos + 4:pos + 8], data[pos + 8:pos + 8 + n]
        (crc,) = struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])
        assert zlib.crc32(typ + body) & 0xFFFFFFFF == crc, f"bad CRC in {typ}"
        if typ == b"IHDR":
            hdr = struct.unpack(">IIBBBBB", body)
        elif typ == b"IDAT":
            idat += body
        elif typ == b"IEND":
            seen_end = True
            break
        pos += 12 + n
    assert hdr is not None and seen_end
    W, H, depth, color, _, _, interlace = hdr
    assert depth == 8 and color == 0 and interlace == 0, hdr
    raw = zlib.decompress(idat)
    assert len(raw) == H * (W + 1), (len(raw), H, W)
    out = np.zeros((H, W), np.uint8)
    prev = np.zeros(W, np.int64)
    for r in range(H):
        ft = raw[r * (W + 1)]
        line = np.frombuffer(raw, np.uint8, W, r * (W + 1) + 1).astype(np.int64)
        cur = np.zeros(W, np.int64)
        for i in range(W):
            a = cur[i - 1] if i > 0 else 0
            b = prev[i]
            c = prev[i - 1] if i > 0 else 0
            pred = {0: 0, 1: a, 2: b, 3: (a + b) // 2, 4: _paeth(a, b, c)}[ft]
            cur[i] = (line[i] + pred) & 0xFF
        out[r] = cur
        prev = cur
    return out


# ----------------------------------------------------------------------------------------------------- shared by the GPU tests
def signal(fmt, n, W, seed):
    """a few seeded tones (one on a bin, one between bins) plus noise, scaled into the format's range; interleaved scalars"""
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    f1 = (rng.integers(0, max(W, 1)) / max(W, 1)) - 0.5
    f2 = rng.uniform(-0.5, 0.5)
    z = 0.5 * np.exp(2j * np.pi * f1 * t) + 0.2 * np.exp(2j * np.pi * f2 * t + 1.0)
    z = z + 0.05 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    v = np.stack([z.real, z.imag], axis=1).reshape(-1)
    if fmt == "cu8":
        return np.clip(np.round(127.5 + 127 * v / 0.8), 0, 255).astype(np.uint8)
    if fmt == "cs16":
        return np.clip(np.round(32767 * v / 0.8), -32768, 32767).astype(np.int16)
    return v.astype(np.float32)


def shifted(a):
    """the bin permutation of spectrogram.c:150-158 applied to any per-bin array"""
    W = a.shape[1]
    half = W // 2
    out = a.copy()
    out[:, :half] = a[:, half:2 * half]
    out[:, half:2 * half] = a[:, :half]
    return out


def check_parity(db, px, raw, fmt, sr, W):
    """rows (dB floats, pixels) of a GPU object against the restatement of the same recording -> (pixels, pixels equal to the float64
    ones), for an aggregate over many calls"""
    want_db, want_px, amp = spectrogram(raw, fmt, sr, W)
    assert db.shape == want_db.shape and px.shape == want_px.shape, (db.shape, want_db.shape)
    # (a) amplitudes within 1e-5 of the row's peak
    got_amp = np.sqrt(10.0 ** (db.astype(np.float64) / 10.0))
    want_amp = shifted(amp)
    err = np.abs(got_amp - want_amp).max(axis=1)
    peak = want_amp.max(axis=1)
    assert np.all(err <= 1e-5 * peak), (fmt, sr, W, (err / peak).max())
    # (b) the pixels are what the returned dB floats give
    assert np.array_equal(px, pixels(db)), (fmt, sr, W)
    # (c) within 1 of the float64 pixels, at most max(2, size // 1000) of them differing
    d = np.abs(px.astype(np.int32) - want_px.astype(np.int32))
    assert d.max() <= 1, (fmt, sr, W)
    assert (d != 0).sum() <= max(2, px.size // 1000), (fmt, sr, W, (d != 0).sum())
    return px.size, int((d == 0).sum())
