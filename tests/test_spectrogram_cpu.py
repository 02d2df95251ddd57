"""CPU tests (-m "not gpu") of the spectrogram: the float64 restatement (tests/spectrogram_ref.py) against the reference's goldens,
every refusal of spectrogram_main (all decided before the device is touched), the C drop-in and the CLI, the kernels' scalar-FP32
code object, and the exported symbols of the two headers."""
import errno
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import sdr_server_amd as xl
import spectrogram_ref as R
from conftest import GOLDEN, ROOT

CSRC = os.path.join(ROOT, "sdr-server_amd", "csrc")
CLI = os.path.join(ROOT, "sdr-server_amd", "bin", "sdr_spectrogram")
DEMO_SRC = os.path.join(ROOT, "tests", "c", "spectrogram_demo.c")
DEMO = os.path.join(ROOT, "sdr-server_amd", "build", "spectrogram_demo")


def _have_gpu():
    try:
        return "no usable device" not in xl.device_info()
    except Exception:
        return False


@pytest.mark.parametrize("fmt,W,name", [("cu8", 64, "cu8"), ("cs16", 64, "cs16"), ("cf32", 64, "cf32"), ("cf32", 63, "cf32_odd")])
def test_restatement_reproduces_the_goldens(fmt, W, name):
    """test/test_spectrogram.c:14-37 through the float64 restatement: pixel for pixel (pins the oracle)."""
    golden = R.decode_png(os.path.join(GOLDEN, f"spectrogram_{name}.png"))
    _, px, _ = R.spectrogram(R.reference_input(fmt), fmt, 128, W)
    assert golden.shape == (2, W)
    assert np.array_equal(px, golden)


def test_png_decoder_filters():
    """the decoder undoes every filter type (the goldens use some; a writer may use any)"""
    import struct
    import zlib

    rng = np.random.default_rng(1)
    img = rng.integers(0, 256, (5, 7)).astype(np.int64)
    raw = b""
    prev = np.zeros(7, np.int64)
    for r, ft in enumerate([0, 1, 2, 3, 4]):
        cur, out = img[r], []
        for i in range(7):
            a = cur[i - 1] if i else 0
            b = prev[i]
            c = prev[i - 1] if i else 0
            pred = {0: 0, 1: a, 2: b, 3: (a + b) // 2, 4: R._paeth(a, b, c)}[ft]
            out.append((cur[i] - pred) & 0xFF)
        raw += bytes([ft]) + bytes(out)
        prev = cur

    def chunk(t, d):
        return struct.pack(">I", len(d)) + t + d + struct.pack(">I", zlib.crc32(t + d) & 0xFFFFFFFF)

    png = b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", 7, 5, 8, 0, 0, 0, 0)) + chunk(b"IDAT", zlib.compress(raw)) + \
        chunk(b"IEND", b"")
    assert np.array_equal(R.decode_png(png), img.astype(np.uint8))


def test_refusals(tmp_path):
    """test/test_spectrogram.c:63-91, then W = 8193, an unsupported format, a height-0 file: all nonzero, all decided before the
    device is touched (so the same here and on a GPU machine), and no image is left behind."""
    inp, out = str(tmp_path / "input.raw"), str(tmp_path / "spectrogram.png")
    R.reference_input("cu8").tofile(inp)
    base = dict(input_file=inp, output_file=out, width=64, sampling_rate=128, data_format="cu8")
    cases = [(dict(input_file=None), -errno.EINVAL), (dict(output_file=None), -errno.EINVAL), (dict(width=0), -errno.EINVAL),
             (dict(width=-3), -errno.EINVAL), (dict(sampling_rate=0), -errno.EINVAL), (dict(width=129), -errno.EINVAL),
             (dict(input_file="/nonexistent/non-existing-file"), -1), (dict(data_format="unsupported"), -1),
             (dict(data_format="cs8"), -1), (dict(width=8193, sampling_rate=100000), -errno.EINVAL),
             (dict(input_file=str(tmp_path / "missing.gz")), -1), (dict(sampling_rate=257), -errno.EINVAL)]
    for change, code in cases:
        assert xl.spectrogram_main(**dict(base, **change)) == code, change
        assert not os.path.exists(out), change
    # a gzip file whose trailer promises less than one row
    import gzip

    with gzip.open(str(tmp_path / "short.raw.gz"), "wb") as f:
        f.write(bytes(100))
    assert xl.spectrogram_main(**dict(base, input_file=str(tmp_path / "short.raw.gz"))) == -errno.EINVAL
    assert not os.path.exists(out)


@pytest.mark.skipif(_have_gpu(), reason="checks the no-device answer")
def test_valid_request_without_a_gpu_is_enodev(tmp_path, capfd):
    inp, out = str(tmp_path / "input.raw"), str(tmp_path / "spectrogram.png")
    R.reference_input("cu8").tofile(inp)
    assert xl.spectrogram_main(inp, out, 64, 128, "cu8") == -errno.ENODEV
    assert "<3>" in capfd.readouterr().err
    with pytest.raises(xl.XlatingError) as e:
        xl.Spectrum(128, 64, "cu8")
    assert e.value.code == -errno.ENODEV


def test_spectrum_create_refusals():
    """xlating_spectrum_create's -EINVAL cases need no device"""
    import ctypes as C

    S = xl.spectrum_lib()
    h = C.c_void_p()
    for sr, w, fmt in [(128, 0, 0), (128, 129, 0), (0, 1, 0), (100000, 8193, 0), (128, 64, 1), (128, 64, 4), (128, 64, -1)]:
        assert S.xlating_spectrum_create(sr, w, fmt, C.byref(h)) == -errno.EINVAL, (sr, w, fmt)
    assert S.xlating_spectrum_create(128, 64, 0, None) == -errno.EINVAL


def test_c_caller_builds_against_the_header_alone(tmp_path):
    os.makedirs(os.path.dirname(DEMO), exist_ok=True)
    libdir = os.path.dirname(xl.spectrum_library_path())
    r = subprocess.run(["gcc", "-std=c11", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), DEMO_SRC, "-o", DEMO,
                        "-L", libdir, "-lxlating_spectrum", f"-Wl,-rpath,{libdir}"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    und = subprocess.run(["nm", "-u", DEMO], capture_output=True, text=True).stdout
    assert "spectrogram_main" in und and "spectrogram_sighandler" in und and "hip" not in und.lower()
    # a refusal runs end to end without a device
    r = subprocess.run([DEMO, str(tmp_path / "none.raw"), str(tmp_path / "o.png"), "0", "128", "cu8"], capture_output=True, text=True,
                       timeout=60)
    assert r.returncode == 1 and r.stdout.strip() == str(-errno.EINVAL)
    hdr = open(os.path.join(ROOT, "include", "spectrogram.h")).read()
    assert "fftw3.h" not in hdr and "png.h" not in hdr
    # the reference's six request fields first, in its order
    fields = re.findall(r"^\s+(?:uint32_t|int|char \*)\s*(\w+);", hdr, re.M)
    assert fields[:6] == ["sampling_rate", "width", "data_format", "input_file", "output_file", "fftw_flags"]


def test_cli_usage_and_refusal(tmp_path):
    r = subprocess.run([CLI, "-h"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0
    for opt in ("-h", "-w", "-s", "-d", "-i", "-o", "-f"):
        assert opt in r.stdout, opt
    assert "1024" in r.stdout and "48000" in r.stdout and "cu8" in r.stdout and "FFTW_MEASURE" in r.stdout
    r = subprocess.run([CLI, "-o", str(tmp_path / "o.png")], capture_output=True, text=True, timeout=60)  # no -i
    assert r.returncode == (-errno.EINVAL) & 0xFF


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="needs hipcc")
def test_spectrum_kernels_issue_no_packed_fp32(tmp_path):
    """as tests/test_mix_no_packed_fp32.py: the file is compiled without the SLP vectoriser (SPEC_FLAGS), and its gfx950 code holds no
    v_pk_{mul,add,fma}_f32 and no matrix instruction"""
    mk = open(os.path.join(CSRC, "Makefile")).read()
    m = re.search(r"^SPEC_FLAGS\s*:=\s*(.+)$", mk, re.M)
    assert m and "-fno-slp-vectorize" in m.group(1)
    assert re.search(r"^\$\(BUILD\)/xl_spectrum_dev\.o: HIPFLAGS \+= \$\(SPEC_FLAGS\)$", mk, re.M)
    assert re.search(r"^\$\(BUILD\)/xl_spectrum_dev\.o: xl_spectrum\.hip", mk, re.M)
    out = str(tmp_path / "k.s")
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fhip-fp32-correctly-rounded-divide-sqrt",
             "--cuda-device-only", "-S"]
    r = subprocess.run(["hipcc"] + flags + m.group(1).split() + [os.path.join(CSRC, "xl_spectrum.hip"), "-o", out], capture_output=True,
                       text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    asm = open(out).read()
    assert "xl_spec_kernel" in asm and "xl_spec_finish_kernel" in asm
    assert not re.search(r"^\s*v_pk_(mul|add|fma)_f32", asm, re.M)
    assert "v_mfma" not in asm


def test_headers_symbols_are_exported():
    """every function include/xlating_spectrum.h and include/spectrogram.h declare is defined in libxlating_spectrum.so"""
    declared = set()
    for h in ("xlating_spectrum.h", "spectrogram.h"):
        src = open(os.path.join(ROOT, "include", h)).read()
        declared |= set(re.findall(r"^(?:int|void)\s+(\w+)\(", src, re.M))
    assert declared == set(xl.SPECTRUM_SYMBOLS), declared
    out = subprocess.run(["nm", "-D", "--defined-only", xl.spectrum_library_path()], capture_output=True, text=True).stdout
    defined = set(re.findall(r" T (\w+)$", out, re.M))
    assert declared <= defined, declared - defined


def test_spec_chunk_knob_goes_through_the_gate():
    src = open(os.path.join(CSRC, "xl_spectrum.cpp")).read()
    assert 'xl_exp_getenv("XL_EXP_SPEC_CHUNK")' in src
    for f in ("xl_spectrum.cpp", "xl_spectrogram.cpp"):
        assert not re.findall(r'(?<!xl_exp_)getenv\("XL_EXP_', open(os.path.join(CSRC, f)).read()), f
