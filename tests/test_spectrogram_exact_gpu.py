"""GPU tests (-m gpu) of the spectrogram family at inputs whose reference answer is known exactly (tests/spectrogram_exact.py): the dB
float and the pixel of every row bit for bit at both ends of the pixel scale, on the 1e-20f floor and next to every pixel boundary, and
the reference's fmaxf rule for NaN samples -- through xl.Spectrum (wide=True above 8192), through xl.SpectrumBank (narrow and wide)
with all cases of one width and format as the streams of ONE bank fed raggedly, and for one case per format through spectrogram_main."""
import numpy as np
import pytest

import sdr_server_amd as xl
import spectrogram_exact as E
import spectrogram_ref as R

pytestmark = pytest.mark.gpu

SSZ = {"cu8": 2, "cs16": 4, "cf32": 8}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same(a, b):
    return a[0].shape == b[0].shape and np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(a[1], b[1])


def run_single(raw, fmt, sr, W, pieces=()):
    """rows of the whole recording from one xl.Spectrum; pieces: sample counts fed one by one (the rest in a last feed)"""
    s = xl.Spectrum(sr, W, fmt, wide=W > 8192)
    parts, pos, n = [], 0, raw.size // 2
    for c in list(pieces) + [n]:
        end = min(pos + c, n)
        if end > pos:
            s.feed(raw[2 * pos:2 * end])
            parts.append(s.take_rows())
        pos = end
    s.close()
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


def ragged(rng, n, W, nfeeds=7):
    """nfeeds feed lengths that sum to n: 0, 1, W - 1 and W + 1 among them where they fit, the others seeded random"""
    special = []
    for c in (0, 1, W - 1, W + 1):
        if sum(special) + c <= n:
            special.append(c)
    rest = n - sum(special)
    cuts = np.sort(rng.integers(0, rest + 1, nfeeds - len(special) - 1))
    counts = np.concatenate([special, np.diff(np.concatenate([[0], cuts, [rest]]))]).astype(np.int64)
    rng.shuffle(counts)
    assert counts.size == nfeeds and counts.sum() == n
    return [int(c) for c in counts]


def run_bank(W, fmt, streams):
    """streams: [(sampling_rate, raw, feed lengths)]: feed f gives every stream its f-th length (0 once its list has ended, what the
    list leaves over in a last feed) in one call from device memory; rows are taken between feeds from every other stream and at the end
    from all -> [(db, px)] per stream"""
    import torch

    st = torch.cuda.current_stream().cuda_stream
    bank = xl.SpectrumBank(W, fmt, wide=W > 8192)
    S = []
    for k, (sr, raw, counts) in enumerate(streams):
        n = raw.size // 2
        counts = [int(c) for c in counts]
        assert sum(counts) <= n
        if sum(counts) < n:
            counts.append(n - sum(counts))
        S.append(dict(id=bank.add(sr), dev=torch.from_numpy(np.array(raw)).cuda(), counts=counts, pos=0, parts=[],
                      early=k % 2 == 0))
    for f in range(max(len(s["counts"]) for s in S)):
        ids, ptrs, cnts = [], [], []
        for s in S:
            c = s["counts"][f] if f < len(s["counts"]) else 0
            ids.append(s["id"])
            ptrs.append(s["dev"].data_ptr() + s["pos"] * SSZ[fmt])
            cnts.append(c)
            s["pos"] += c
        bank.feed(ids, ptrs, cnts, st)
        for s in S:
            if s["early"] and f % 3 == 0:
                s["parts"].append(bank.take_rows(s["id"]))
    out = []
    for s in S:
        s["parts"].append(bank.take_rows(s["id"]))
        assert bank.rows_pending(s["id"]) == 0
        out.append((np.concatenate([p[0] for p in s["parts"]]), np.concatenate([p[1] for p in s["parts"]])))
    bank.close()
    return out


def report(name, got, want_db, want_px):
    """a line per case that misses its exact expectation, before the assertion: how many dB floats and pixels differ, where, by how
    much"""
    db, px = got
    if db.shape != want_db.shape:
        print(f"{name}: shape {db.shape}, expected {want_db.shape}")
        return False
    bad_db, bad_px = bits(db) != bits(want_db), px != want_px
    if bad_db.any() or bad_px.any():
        r, c = np.argwhere(bad_db | bad_px)[0]
        print(f"{name}: {bad_db.sum()} dB floats and {bad_px.sum()} pixels of {db.size} differ; first at row {r} column {c}: "
              f"dB {db[r, c]!r} ({int(bits(db)[r, c]):#010x}) pixel {px[r, c]}, expected {want_db[r, c]!r} "
              f"({int(bits(want_db)[r, c]):#010x}) pixel {want_px[r, c]}")
        return False
    return True


# ------------------------------------------------------------------------------------------------------------ the pixel ladder
def test_ladder():
    """W = 1 at sampling_rate 1: every sample is a row whose power, dB and pixel are known in float32 -- both sides of every pixel
    boundary from -200 to +4 dB, both clamps, the floor, powers that overflow.  One single object, one bank stream fed raggedly."""
    raw, _, want_db, want_px = E.ladder()
    one = run_single(raw, "cf32", 1, 1)
    (bank,) = run_bank(1, "cf32", [(1, raw, ragged(np.random.default_rng(1), raw.size // 2, 1))])
    ok = report("ladder, single", one, want_db, want_px)
    ok = report("ladder, bank", bank, want_db, want_px) and ok
    assert ok
    assert same(bank, one)


# ------------------------------------------------------------------------------------------------------------ constants, on-bin tones
@pytest.mark.parametrize("fmt", ["cu8", "cs16", "cf32"])
@pytest.mark.parametrize("W", E.PLAIN_WIDTHS + E.PLAIN_WIDE)
def test_constants_plain(W, fmt):
    """silence, the formats' extremes, one LSB, cf32 above full scale -- as constants (bin 0), times (-1)^n (bin W / 2: column 0) and
    times i^n (bin W / 4): the peak column's exact float32 power, 1e-20f in every other column; dB and pixel bit for bit"""
    cases = E.constant_cases(fmt, W)
    rng = np.random.default_rng(100 * W + SSZ[fmt])
    banked = run_bank(W, fmt, [(c["sr"], c["raw"], ragged(rng, 2 * c["sr"], W)) for c in cases])
    ok = True
    for c, rows in zip(cases, banked):
        one = run_single(c["raw"], fmt, c["sr"], W)
        ok = report(c["name"] + ", single", one, c["db"], c["px"]) and ok
        ok = report(c["name"] + ", bank", rows, c["db"], c["px"]) and ok
        assert same(rows, one), c["name"]
    assert ok


@pytest.mark.parametrize("fmt", ["cu8", "cs16", "cf32"])
@pytest.mark.parametrize("W", E.BLUE_WIDTHS + E.BLUE_WIDE)
def test_constants_bluestein(W, fmt):
    """the chirp products round: silence stays exact (0 . chirp = 0); of a constant, the peak column's pixel (255 by the clamp where
    the power is >= 1) and criterion (a) of check_parity for every column"""
    cases = E.constant_cases(fmt, W, bluestein=True)
    rng = np.random.default_rng(100 * W + SSZ[fmt])
    banked = run_bank(W, fmt, [(c["sr"], c["raw"], ragged(rng, 2 * c["sr"], W)) for c in cases])
    ok = True
    for c, rows in zip(cases, banked):
        one = run_single(c["raw"], fmt, c["sr"], W)
        assert same(rows, one), c["name"]
        if c["silent"]:
            ok = report(c["name"], one, c["db"], c["px"]) and ok
            continue
        db, px = one
        assert db.shape == c["db"].shape
        ratio = E.amplitudes_ok(db, c["db"])
        print(f"{c['name']}: peak pixel {px[:, c['col']]}, expected {c['px'][0, c['col']]}; worst (a) ratio {ratio:.3e}")
        assert np.all(px[:, c["col"]] == c["px"][:, c["col"]]), c["name"]
        assert ratio <= 1e-5, c["name"]
        assert np.array_equal(px, E.pixel_f32(db)), c["name"]
        if c["power"] >= 1:
            assert np.all(px[:, c["col"]] == 255)
    assert ok


# ------------------------------------------------------------------------------------------------------------ NaN samples
@pytest.mark.parametrize("nan_bits", E.NAN_BITS, ids=hex)
@pytest.mark.parametrize("W", E.NAN_WIDTHS + E.NAN_WIDE)
def test_nan_samples_follow_fmaxf(W, nan_bits):
    """spectrogram.c:148 takes the row maximum with fmaxf: a transform that holds a NaN sample does not contribute to its row.  Row 0
    clean and row 1 (a NaN in its second transform) meet check_parity against the restatement; row 2 (a NaN among the skipped samples)
    is the row of the recording without that NaN; row 3 (a NaN in every transform) is pixel 0 throughout, its dB not finite.  Feeds that
    put row 1's NaN last in a feed, first in a feed and inside the carry give the same rows; the bank gives the single object's."""
    c = E.nan_case(W, nan_bits)
    sr, raw = c["sr"], c["raw"]
    one = run_single(raw, "cf32", sr, W)
    db, px = one
    assert db.shape == (4, W)
    print(f"NaN case W={W} {nan_bits:#x}: non-finite dB per row {[int((~np.isfinite(db[r])).sum()) for r in range(4)]}, "
          f"pixel-0 columns per row {[int((px[r] == 0).sum()) for r in range(4)]}")
    R.check_parity(db[:2], px[:2], raw[:2 * 2 * sr], "cf32", sr, W)
    assert np.all(px[3] == 0) and not np.any(np.isfinite(db[3]))
    zeroed = run_single(c["zeroed"], "cf32", sr, W)
    assert np.array_equal(bits(db[2]), bits(zeroed[0][2])) and np.array_equal(px[2], zeroed[1][2])
    assert np.all(np.isfinite(db[:3]))
    for pieces in c["pieces"]:
        assert same(run_single(raw, "cf32", sr, W, pieces), one), pieces
    rng = np.random.default_rng(W + 1)
    banked = run_bank(W, "cf32", [(sr, raw, ragged(rng, 4 * sr, W))] + [(sr, raw, p) for p in c["pieces"]] +
                      [(sr, c["zeroed"], ragged(rng, 4 * sr, W))])
    for k, rows in enumerate(banked[:-1]):
        assert same(rows, one), k
    assert same(banked[-1], zeroed)


# ------------------------------------------------------------------------------------------------------------ the file path
def _main_case(name):
    if name == "ladder":
        raw, _, _, px = E.ladder()
        return "cf32", 1, 1, raw, px
    if name == "nan":
        c = E.nan_case(64, E.NAN_BITS[1])
        want = run_single(c["raw"], "cf32", c["sr"], 64)[1]
        floor = R.spectrogram(c["raw"], "cf32", c["sr"], 64)[1][:3].min()  # (the restatement's rows 0 .. 2: noise at -26 dB, no 0)
        assert np.all(want[3] == 0) and floor > 100 and np.all(want[:3] >= floor - 1)
        return "cf32", 64, c["sr"], c["raw"], want
    fmt, W, pick = {"cu8": ("cu8", 64, "cu8 (127, 127) alt W=64 sr=225"), "cs16": ("cs16", 1024, "cs16 (-32768, -32768) const W=1024 sr=1024")}[name]
    c = {c["name"]: c for c in E.constant_cases(fmt, W)}[pick]
    return fmt, W, c["sr"], c["raw"], c["px"]


@pytest.mark.parametrize("name", ["cu8", "cs16", "ladder", "nan"])
def test_spectrogram_main_writes_the_exact_pixels(tmp_path, name):
    """spectrogram_main -> PNG -> decode_png: the ladder's pixels (cf32), a cu8 tone on bin W / 2 with its floor, cs16 at the clamp,
    and the NaN recording's rows"""
    fmt, W, sr, raw, want = _main_case(name)
    inp, out = str(tmp_path / "in.raw"), str(tmp_path / "out.png")
    with open(inp, "wb") as f:
        f.write(np.ascontiguousarray(raw).tobytes())
    assert xl.spectrogram_main(inp, out, W, sr, fmt) == 0
    px = R.decode_png(out)
    assert px.shape == want.shape, (px.shape, want.shape)
    assert np.array_equal(px, want), (np.argwhere(px != want)[:4], px[px != want][:4], want[px != want][:4])
