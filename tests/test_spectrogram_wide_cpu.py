"""CPU tests (-m "not gpu") of the spectrogram's wide entry points (xlating_spectrum_create_wide, spectrogram_main_wide, sdr_spectrogram
-W): every refusal, decided before the device is touched; the default entries' unchanged refusal of 8193; the two-level transform's
host-side plan (sdr-server_amd/csrc/xl_spectrum_wide_plan.h) through a gcc shim and as a stand-alone program under ASan and UBSan; the
kernels' scalar-FP32 code object; the scratch knob's gate; a C caller built against the headers alone."""
import ctypes as C
import errno
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import sdr_server_amd as xl
import spectrogram_ref as R
from conftest import ROOT

CSRC = os.path.join(ROOT, "sdr-server_amd", "csrc")
CLI = os.path.join(ROOT, "sdr-server_amd", "bin", "sdr_spectrogram")
SWEEP_SRC = os.path.join(ROOT, "tests", "c", "spectrum_wide_plan_sweep.c")
DEMO_SRC = os.path.join(ROOT, "tests", "c", "spectrogram_wide_demo.c")
MAX_WIDE = 1048576


def _have_gpu():
    try:
        return "no usable device" not in xl.device_info()
    except Exception:
        return False


# ------------------------------------------------------------------------------------------------------------ refusals
def test_create_wide_refusals():
    """xlating_spectrum_create's checks with the wide cap: width <= 0, width 1048577, width > sampling_rate, sampling_rate 0, a bad
    format, NULL out -- all -EINVAL without a device"""
    S = xl.spectrum_lib()
    h = C.c_void_p()
    big = 4000000
    for sr, w, fmt in [(big, 0, 0), (big, -5, 0), (big, MAX_WIDE + 1, 0), (10000, 10001, 0), (128, 129, 0), (0, 1, 0), (0, 20000, 0),
                       (big, 20000, 1), (big, 20000, 4), (big, 20000, -1), (128, 64, 1)]:
        assert S.xlating_spectrum_create_wide(sr, w, fmt, C.byref(h)) == -errno.EINVAL, (sr, w, fmt)
    assert S.xlating_spectrum_create_wide(big, 20000, 0, None) == -errno.EINVAL
    assert S.xlating_spectrum_create_wide(128, 64, 0, None) == -errno.EINVAL
    hdr = open(os.path.join(ROOT, "include", "xlating_spectrum.h")).read()
    assert re.search(r"^#define XLATING_SPECTRUM_MAX_WIDE_WIDTH %d$" % MAX_WIDE, hdr, re.M)
    assert re.search(r"^#define XLATING_SPECTRUM_MAX_WIDTH 8192$", hdr, re.M)
    with pytest.raises(xl.XlatingError) as e:
        xl.Spectrum(big, MAX_WIDE + 1, "cu8", wide=True)
    assert e.value.code == -errno.EINVAL
    with pytest.raises(xl.XlatingError) as e:
        xl.Spectrum(big, 20000, "cs8", wide=True)
    assert e.value.code == -errno.EINVAL


def test_main_wide_refusals(tmp_path, capfd):
    """spectrogram_main's refusals, in its order, with the wide cap; no image is left behind"""
    inp, out = str(tmp_path / "input.raw"), str(tmp_path / "spectrogram.png")
    R.reference_input("cu8").tofile(inp)
    base = dict(input_file=inp, output_file=out, width=64, sampling_rate=128, data_format="cu8", wide=True)
    cases = [(dict(input_file=None), -errno.EINVAL), (dict(output_file=None), -errno.EINVAL), (dict(width=0), -errno.EINVAL),
             (dict(width=-3), -errno.EINVAL), (dict(sampling_rate=0), -errno.EINVAL), (dict(width=129), -errno.EINVAL),
             (dict(width=MAX_WIDE + 1, sampling_rate=4000000), -errno.EINVAL), (dict(width=20000, sampling_rate=19999), -errno.EINVAL),
             (dict(width=20000, sampling_rate=0), -errno.EINVAL), (dict(data_format="unsupported", width=20000, sampling_rate=20000), -1),
             (dict(data_format="cs8"), -1), (dict(input_file="/nonexistent/non-existing-file", width=20000, sampling_rate=20000), -1),
             # a file shorter than one row of a wide width
             (dict(width=20000, sampling_rate=20000), -errno.EINVAL)]
    for change, code in cases:
        capfd.readouterr()
        assert xl.spectrogram_main(**dict(base, **change)) == code, change
        assert not os.path.exists(out), change
        if change.get("width") == MAX_WIDE + 1:  # the stderr line for a width above the cap names the cap in force
            assert f"width (-w) {MAX_WIDE + 1} exceeds the largest supported width {MAX_WIDE}" in capfd.readouterr().err


def test_default_entries_still_refuse_8193(tmp_path, capfd):
    """the opt-in pinned from this side too: without `wide` every entry answers 8193 as before"""
    S = xl.spectrum_lib()
    h = C.c_void_p()
    assert S.xlating_spectrum_create(100000, 8193, 0, C.byref(h)) == -errno.EINVAL
    assert S.xlating_spectrum_bank_create(8193, 0, C.byref(h)) == -errno.EINVAL
    inp, out = str(tmp_path / "input.raw"), str(tmp_path / "spectrogram.png")
    np.zeros(2 * 10000, np.uint8).tofile(inp)
    assert xl.spectrogram_main(inp, out, 8193, 10000, "cu8") == -errno.EINVAL
    assert "exceeds the largest supported width 8192" in capfd.readouterr().err
    assert not os.path.exists(out)
    r = subprocess.run([CLI, "-w", "8193", "-s", "10000", "-i", inp, "-o", out], capture_output=True, text=True, timeout=60)
    assert r.returncode == (-errno.EINVAL) & 0xFF and not os.path.exists(out)
    with pytest.raises(xl.XlatingError):
        xl.Spectrum(100000, 8193, "cu8")


@pytest.mark.skipif(_have_gpu(), reason="checks the no-device answer")
def test_valid_wide_request_without_a_gpu_is_enodev(tmp_path, capfd):
    inp, out = str(tmp_path / "input.raw"), str(tmp_path / "spectrogram.png")
    np.zeros(2 * 20000, np.uint8).tofile(inp)
    capfd.readouterr()
    assert xl.spectrogram_main(inp, out, 20000, 20000, "cu8", wide=True) == -errno.ENODEV
    assert "<3>" in capfd.readouterr().err
    assert not os.path.exists(out)
    with pytest.raises(xl.XlatingError) as e:
        xl.Spectrum(MAX_WIDE, MAX_WIDE, "cf32", wide=True)
    assert e.value.code == -errno.ENODEV
    assert "<3>" in capfd.readouterr().err
    r = subprocess.run([CLI, "-W", "-w", "20000", "-s", "20000", "-i", inp, "-o", out], capture_output=True, text=True, timeout=60)
    assert r.returncode == (-errno.ENODEV) & 0xFF and "<3>" in r.stderr and not os.path.exists(out)


def test_cli_lists_the_flag():
    r = subprocess.run([CLI, "-h"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and re.search(r"^\s+-W\s", r.stdout, re.M) and "1048576" in r.stdout


def test_python_names():
    assert "xlating_spectrum_create_wide" in xl.SPECTRUM_SYMBOLS and "spectrogram_main_wide" in xl.SPECTRUM_SYMBOLS
    out = subprocess.run(["nm", "-D", "--defined-only", xl.spectrum_library_path()], capture_output=True, text=True).stdout
    assert " T xlating_spectrum_create_wide" in out and " T spectrogram_main_wide" in out


# ------------------------------------------------------------------------------------------------------------ the plan header
SHIM = r"""
#include "xl_spectrum_wide_plan.h"
int plan(uint32_t W, uint32_t *o) {
  XlSpecWidePlan p;
  const int rc = xl_specw_plan(W, &p);
  if (rc == 0) { o[0] = p.N; o[1] = p.N1; o[2] = p.N2; o[3] = p.pack; o[4] = p.blue; }
  return rc;
}
uint32_t length(uint32_t W) { return xl_specw_length(W); }
uint64_t chunk(uint64_t bytes, uint32_t N) { return xl_specw_chunk(bytes, N); }
void col_pos(uint32_t N1, uint32_t N2, uint32_t W, const uint32_t *j, uint32_t n, uint32_t *o) {
  for (uint32_t i = 0; i < n; ++i) o[i] = xl_specw_col_pos(N1, N2, W, j[i]);
}
void bin_pos(uint32_t N1, uint32_t N2, const uint32_t *k, uint32_t n, uint32_t *o) {
  for (uint32_t i = 0; i < n; ++i) o[i] = xl_specw_bin_pos(N1, N2, k[i]);
}
"""


@pytest.fixture(scope="module")
def planlib(tmp_path_factory):
    d = tmp_path_factory.mktemp("wideplan")
    src = d / "shim.c"
    src.write_text(SHIM)
    so = d / "libwideplan.so"
    subprocess.run(["gcc", "-std=c11", "-O1", "-Wall", "-Werror", "-shared", "-fPIC", "-I", CSRC, str(src), "-o", str(so)], check=True)
    L = C.CDLL(str(so))
    L.plan.argtypes = [C.c_uint32, C.POINTER(C.c_uint32)]
    L.length.argtypes = [C.c_uint32]
    L.length.restype = C.c_uint32
    L.chunk.argtypes = [C.c_uint64, C.c_uint32]
    L.chunk.restype = C.c_uint64
    L.col_pos.argtypes = [C.c_uint32] * 3 + [C.c_void_p, C.c_uint32, C.c_void_p]
    L.col_pos.restype = None
    L.bin_pos.argtypes = [C.c_uint32] * 2 + [C.c_void_p, C.c_uint32, C.c_void_p]
    L.bin_pos.restype = None
    return L


def _plan(L, W):
    o = (C.c_uint32 * 5)()
    assert L.plan(W, o) == 0, W
    return dict(zip(("N", "N1", "N2", "pack", "blue"), o))


def test_plan_header_is_plain_c():
    hdr = open(os.path.join(CSRC, "xl_spectrum_wide_plan.h")).read()
    assert "#include <hip" not in hdr and "hipLaunch" not in hdr


def test_plan_every_length(planlib):
    """N = 2^14 .. 2^21: N1 N2 = N, N2 <= 8192, pack runs of at least 16 samples, at least one transform per scratch chunk"""
    seen = set()
    for e in range(14, 22):
        N = 1 << e
        W = N if e <= 20 else MAX_WIDE - 1  # 2^21 is a Bluestein length only
        if e == 21:
            assert planlib.length(W) == N
        p = _plan(planlib, W)
        assert p["N"] == N and p["N1"] * p["N2"] == N and p["N2"] <= 8192
        assert p["N2"] == min(8192, N // 64) and p["N1"] in (64, 128, 256)
        assert p["pack"] == 4096 // p["N1"] and p["pack"] >= 16 and p["N2"] % p["pack"] == 0
        assert p["blue"] == (0 if e <= 20 else 1)
        for scratch in (0, 1, 8 * N - 1, 8 * N, 3 * 8 * N, 3 * 8 * N + 5, 64 << 20):
            assert planlib.chunk(scratch, N) == max(1, scratch // (8 * N))
        assert planlib.chunk(64 << 20, N) >= 1
        seen.add((p["N1"], p["N2"]))
        # a Bluestein width of the same length has the same split
        if e >= 15:
            Wb = N // 2  # 2 Wb - 1 < N, and the next width's 2 W - 1 = N + 1 > N
            for w in (Wb - 1, N // 4 + 1):
                q = _plan(planlib, w)
                assert q["N"] == N and q["blue"] == 1 and (q["N1"], q["N2"]) == (p["N1"], p["N2"]), w
    assert len(seen) == 8
    o = (C.c_uint32 * 5)()
    for W in (0, 1, 8192, MAX_WIDE + 1):
        assert planlib.plan(W, o) == -1, W


def test_plan_bluestein_lengths(planlib):
    for W, L in [(8193, 1 << 15), (16385, 1 << 16), (50000, 1 << 17), (100000, 1 << 18), (200000, 1 << 19), (262145, 1 << 20),
                 (1048575, 1 << 21), (16383, 1 << 15), (20000, 1 << 16), (524289, 1 << 21)]:
        got = planlib.length(W)
        assert got == L and got >= 2 * W - 1 and got // 2 < 2 * W - 1, (W, got)


def _shift_src(j, W):
    half = W // 2
    return np.where(j < half, j + half, np.where(j < 2 * half, j - half, j))


@pytest.mark.parametrize("W,sampled", [(16384, False), (1 << 20, True)])
def test_bin_permutation(planlib, W, sampled):
    """column j of a finished plain row reads position (k % N1) * N2 + k // N1 of bin k = the half swap's source of j: a bijection of
    0 .. W - 1 (exhaustive at 16384; at 2^20 a seeded sample and both ends, injective on it), inverse to where the row pass leaves bin k"""
    p = _plan(planlib, W)
    N1, N2 = p["N1"], p["N2"]
    if sampled:
        rng = np.random.default_rng(5)
        j = np.unique(np.concatenate([rng.integers(0, W, 5000), [0, 1, W // 2 - 1, W // 2, W // 2 + 1, W - 2, W - 1]])).astype(np.uint32)
    else:
        j = np.arange(W, dtype=np.uint32)
    pos = np.empty_like(j)
    planlib.col_pos(N1, N2, W, j.ctypes.data, j.size, pos.ctypes.data)
    assert pos.max() < W and np.unique(pos).size == j.size
    if not sampled:
        assert np.array_equal(np.sort(pos), np.arange(W))
    k = _shift_src(j.astype(np.int64), W)  # the bin column j shows
    assert np.array_equal(pos, (k % N1) * N2 + k // N1)
    # the row pass leaves bin k1 + N1 k2 at [k1][k2]: reading a layout made that way through col_pos gives the half-swapped bins
    layout = np.empty(W, np.int64)
    k1, k2 = np.meshgrid(np.arange(N1), np.arange(N2), indexing="ij")
    layout[(k1 * N2 + k2).reshape(-1)] = (k1 + N1 * k2).reshape(-1)
    bins = np.arange(W).reshape(1, W)
    assert np.array_equal(layout[pos], R.shifted(bins)[0][j])
    bp = np.empty_like(j)
    planlib.bin_pos(N1, N2, j.ctypes.data, j.size, bp.ctypes.data)
    assert np.array_equal(layout[bp], j)


def test_plan_sweep_under_the_sanitizers(tmp_path):
    """the header with a main of its own, built with ASan and UBSan and run as a process of its own"""
    exe = str(tmp_path / "spectrum_wide_plan_sweep")
    r = subprocess.run(["gcc", "-std=c11", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I", CSRC, SWEEP_SRC, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok ") and r.stderr == "", (r.stdout[-500:], r.stderr[-2000:])
    assert int(r.stdout.split()[1]) >= 20000


def test_the_core_takes_its_rules_from_the_plan():
    """xl_spectrum.cpp and the kernels decide no split or chunk count of their own"""
    host = re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, "xl_spectrum.cpp")).read())
    assert "xl_specw_plan(" in host and "xl_specw_chunk(" in host and "xl_specw_bin_pos(" in host
    dev = re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, "xl_spectrum_wide.hip")).read())
    assert "XL_SPECW_N2(" in dev and "xl_specw_col_pos(" in dev and "/ 64" not in dev


# ------------------------------------------------------------------------------------------------------------ build and source
@pytest.mark.skipif(shutil.which("hipcc") is None, reason="needs hipcc")
def test_wide_kernels_issue_no_packed_fp32(tmp_path):
    """as test_spectrum_kernels_issue_no_packed_fp32: compiled with SPEC_FLAGS, and the gfx950 code holds no v_pk_{mul,add,fma}_f32 and
    no matrix instruction"""
    mk = open(os.path.join(CSRC, "Makefile")).read()
    m = re.search(r"^SPEC_FLAGS\s*:=\s*(.+)$", mk, re.M)
    assert m and "-fno-slp-vectorize" in m.group(1)
    assert re.search(r"^\$\(BUILD\)/xl_spectrum_wide_dev\.o: HIPFLAGS \+= \$\(SPEC_FLAGS\)$", mk, re.M)
    assert re.search(r"^\$\(BUILD\)/xl_spectrum_wide_dev\.o: xl_spectrum_wide\.hip", mk, re.M)
    assert re.search(r"^SPEC_OBJS :=.*\$\(BUILD\)/xl_spectrum_wide_dev\.o", mk, re.M)
    assert re.search(r"^HIPFLAGS :=.*-ffp-contract=off", mk, re.M)
    out = str(tmp_path / "k.s")
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fhip-fp32-correctly-rounded-divide-sqrt",
             "--cuda-device-only", "-S"]
    r = subprocess.run(["hipcc"] + flags + m.group(1).split() + [os.path.join(CSRC, "xl_spectrum_wide.hip"), "-o", out], capture_output=True,
                       text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    asm = open(out).read()
    for k in ("xl_specw_col_in_kernel", "xl_specw_row_kernel", "xl_specw_col_out_kernel", "xl_specw_finish_kernel"):
        assert k in asm, k
    assert not re.search(r"^\s*v_pk_(mul|add|fma)_f32", asm, re.M)
    assert "v_mfma" not in asm
    src = open(os.path.join(CSRC, "xl_spectrum_wide.hip")).read()
    assert not re.search(r"\b(sinf?|cosf?|sincosf?|__sinf|__cosf)\s*\(", re.sub(r"//[^\n]*", "", src))
    assert "hipfft" not in src.lower() and "rocfft" not in src.lower()


def test_scratch_knob_goes_through_the_gate():
    src = open(os.path.join(CSRC, "xl_spectrum.cpp")).read()
    assert 'xl_exp_getenv("XL_EXP_SPEC_SCRATCH")' in src
    for f in os.listdir(CSRC):
        if f.startswith(("xl_spectrum", "xl_spectrogram")):
            text = open(os.path.join(CSRC, f)).read()
            assert not re.findall(r'(?<!xl_exp_)getenv\("XL_EXP_', text), f
            if f != "xl_spectrum.cpp":
                assert "XL_EXP_SPEC_SCRATCH" not in text, f
    assert src.count("XL_EXP_SPEC_SCRATCH") == 1


def test_c_caller_builds_against_the_headers_alone(tmp_path):
    exe = str(tmp_path / "spectrogram_wide_demo")
    libdir = os.path.dirname(xl.spectrum_library_path())
    r = subprocess.run(["gcc", "-std=c11", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), DEMO_SRC, "-o", exe,
                        "-L", libdir, "-lxlating_spectrum", f"-Wl,-rpath,{libdir}"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    und = subprocess.run(["nm", "-u", exe], capture_output=True, text=True).stdout
    assert "spectrogram_main_wide" in und and "xlating_spectrum_create_wide" in und and "hip" not in und.lower()
    # refusals run end to end without a device: width 1048577 through both entries
    r = subprocess.run([exe, str(tmp_path / "none.raw"), str(tmp_path / "o.png"), str(MAX_WIDE + 1), "4000000", "cu8"], capture_output=True,
                       text=True, timeout=60)
    assert r.returncode == 1 and r.stdout.split() == [str(-errno.EINVAL), str(-errno.EINVAL)], (r.stdout, r.stderr)
    assert not os.path.exists(str(tmp_path / "o.png"))
