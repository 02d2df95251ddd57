"""CPU tests (-m "not gpu") of the Q15 resampler bank (include/xlating_resample_q15.h): the tap quantiser against numpy and on its
edges -- through the library, and once more as a stand-alone program under the sanitizers -- the refusals that need no device, the
exported symbols, a C caller built against the header alone, the kernels' code object, and the admitted second-stage filters: that
they quantise, that they meet the 32-bit condition, and that the integer restatement (tests/resample_q15_ref.py) stays within the
DERIVED Q + 1 output LSBs of the unquantised filter."""
import ctypes as C
import errno
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import resample_q15_ref as QR
import resample_ref as RR
import sdr_server_amd as xl
from conftest import ROOT

CSRC = os.path.join(ROOT, "sdr-server_amd", "csrc")
BUILD = os.path.join(ROOT, "sdr-server_amd", "build")
DEMO_SRC = os.path.join(ROOT, "tests", "c", "resample_q15_demo.c")
SWEEP_SRC = os.path.join(ROOT, "tests", "c", "resample_q15_quantize_sweep.c")
BAND_FREQ = 460100000
ADMITTED = [(10000000, 48000), (2016000, 44100), (2400000, 44100), (2048000, 48000), (2400000, 2000000), (2400000, 1600000),
            (20000000, 44100)]


def _have_gpu():
    try:
        return "no usable device" not in xl.device_info()
    except Exception:
        return False


def admitted_filter(fs, fo):
    """-> (L, M, taps) of the second stage xlating_wire_admit_any_rate gives a client of rate fo on a band of rate fs"""
    req = xl.WireRequest(BAND_FREQ + 1000, fo, BAND_FREQ, 0)
    code, adm, rs, why = xl.wire_admit_any_rate(req, fs, 0, 5)
    assert code == 0 and (rs.L, rs.M) != (1, 1), (fs, fo, why)
    code, taps = xl.wire_resample_taps(req, rs, 5)
    assert code == 0
    return rs.L, rs.M, taps


# ------------------------------------------------------------------------------------------------------------ the quantiser
def code_of(taps):
    with pytest.raises(xl.XlatingError) as e:
        xl.resample_q15_quantize(taps)
    return e.value.code


def test_quantize_equals_numpy_trunc_on_random_taps():
    rng = np.random.default_rng(15)
    for scale in (0.999, 0.1, 1e-4, 3e-5):
        h = (rng.uniform(-1, 1, 5000) * scale).astype(np.float32)
        c = xl.resample_q15_quantize(h)
        assert c.dtype == np.int16 and c.shape == h.shape
        want = np.trunc(h * np.float32(32768.0))
        assert want.dtype == np.float32 and np.array_equal(c.astype(np.float64), want.astype(np.float64))
        assert np.array_equal(c.astype(np.int64), QR.quantize(h))
    assert np.any(xl.resample_q15_quantize((rng.uniform(-1, 0, 100) * 3e-5).astype(np.float32)) == 0)  # toward zero, not the floor


def test_quantize_edges():
    f32 = np.float32
    below_one = np.nextafter(f32(1), f32(0))
    assert xl.resample_q15_quantize([-1.0]).tolist() == [-32768]
    assert code_of([1.0]) == -errno.ERANGE
    assert xl.resample_q15_quantize([below_one]).tolist() == [32767]
    assert xl.resample_q15_quantize([-1e-9]).tolist() == [0]
    for bad in (np.nan, np.inf, -np.inf):
        assert code_of([0.25, bad]) == -errno.ERANGE, bad
    assert code_of([]) == -errno.EINVAL
    R = xl.resample_q15_lib()
    one, out = (C.c_float * 1)(0.5), (C.c_int16 * 1)()
    assert R.xlating_resample_q15_quantize(None, 1, out) == -errno.EINVAL
    assert R.xlating_resample_q15_quantize(one, 0, out) == -errno.EINVAL
    assert R.xlating_resample_q15_quantize(one, 1, None) == -errno.EINVAL
    assert R.xlating_resample_q15_quantize(one, 1, out) == 0 and out[0] == 16384
    # the truncated value decides, not the tap: -32768.99 truncates into range, -32769 does not; float32's largest overflows
    edge = f32(-1.0) - f32(2.0 ** -15)
    assert xl.resample_q15_quantize([np.nextafter(edge, f32(0))]).tolist() == [-32768]
    assert code_of([edge]) == -errno.ERANGE
    assert code_of([f32(3.4028235e38)]) == -errno.ERANGE and code_of([f32(-3.4028235e38)]) == -errno.ERANGE
    denormal = np.array([0x00000001, 0x80000001, 0x00800000], np.uint32).view(np.float32)  # +- the smallest, the smallest normal
    assert xl.resample_q15_quantize(denormal).tolist() == [0, 0, 0]


def test_quantize_sweep_under_the_sanitizers(tmp_path):
    """the plain-C quantiser header with a main of its own, built with ASan and UBSan (the float-to-integer conversion check among
    them) and run as a process of its own: no report"""
    hdr = open(os.path.join(CSRC, "xl_resample_q15_quant.h")).read()
    assert "hip" not in hdr.lower().replace("no hip", "")
    exe = str(tmp_path / "resample_q15_quantize_sweep")
    r = subprocess.run(["gcc", "-std=c11", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fsanitize=float-cast-overflow",
                        "-fno-sanitize-recover=all", "-I", CSRC, SWEEP_SRC, "-o", exe, "-lm"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok ") and r.stderr == "", (r.stdout[-500:], r.stderr[-2000:])
    assert int(r.stdout.split()[1]) >= 400000


def test_add_quantises_with_the_header_only():
    """add and xlating_resample_q15_quantize call the one quantiser; the -ERANGE of add is decided before the device is touched"""
    src = re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, "xl_resample.cpp")).read())
    assert '#include "xl_resample_q15_quant.h"' in src
    assert len(re.findall(r"\bxl_resample_q15_quantize\(", src)) == 2
    assert "32768" not in src
    body = src[src.index('extern "C" int xlating_resample_q15_bank_add('):]
    body = body[:body.index("\n}\n")]
    assert "hip" not in body[:body.index("xl_resample_q15_quantize(")]
    assert body.index("return -EINVAL;") < body.index("xl_resample_q15_quantize(") < body.index("xl_rs_add(")


# ------------------------------------------------------------------------------------------------------------ refusals, symbols
def test_refusals_need_no_device():
    R = xl.resample_q15_lib()
    one = (C.c_float * 1)(0.5)
    assert R.xlating_resample_q15_bank_create(None) == -errno.EINVAL
    assert R.xlating_resample_q15_bank_add(None, 1, 1, one, 1) == -errno.EINVAL
    assert R.xlating_resample_q15_bank_remove(None, 0) == -errno.EINVAL
    assert R.xlating_resample_q15_bank_feed_device(None, 0, None, None, None, None) == -errno.EINVAL
    p, n, f = C.c_void_p(), C.c_size_t(0), C.POINTER(C.c_int16)()
    assert R.xlating_resample_q15_bank_output_device(None, 0, C.byref(p), C.byref(n)) == -errno.EINVAL
    assert R.xlating_resample_q15_bank_fetch(None) == -errno.EINVAL
    assert R.xlating_resample_q15_bank_output_host(None, 0, C.byref(f), C.byref(n)) == -errno.EINVAL
    assert R.xlating_resample_q15_bank_produced(None, 0) == 0
    assert R.xlating_resample_q15_bank_last_feed_ops(None, None, None) == -errno.EINVAL
    assert R.xlating_resample_q15_bank_stats(None, None, None, None) == -errno.EINVAL
    R.xlating_resample_q15_bank_destroy(None)


def test_valid_create_without_a_gpu_is_enodev(capfd):
    if _have_gpu():
        pytest.skip("checks the no-device answer")
    R = xl.resample_q15_lib()
    h = C.c_void_p()
    assert R.xlating_resample_q15_bank_create(C.byref(h)) == -errno.ENODEV
    assert "<3>" in capfd.readouterr().err
    assert not h.value
    with pytest.raises(xl.XlatingError) as e:
        xl.ResamplerBankQ15()
    assert e.value.code == -errno.ENODEV


def test_symbols_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "xlating_resample_q15.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"^(?:int|void|uint64_t)\s+(\w+)\(", code, re.M))
    assert declared == set(xl.RESAMPLE_Q15_SYMBOLS), declared ^ set(xl.RESAMPLE_Q15_SYMBOLS)
    assert len(xl.RESAMPLE_Q15_SYMBOLS) == len(xl.RESAMPLE_SYMBOLS) + 1  # the float bank's, one for one, and the quantiser
    out = subprocess.run(["nm", "-D", "--defined-only", xl.resample_library_path()], capture_output=True, text=True).stdout
    defined = set(re.findall(r" T (\w+)$", out, re.M))
    assert set(xl.RESAMPLE_Q15_SYMBOLS) <= defined, set(xl.RESAMPLE_Q15_SYMBOLS) - defined
    R = xl.resample_q15_lib()
    for name in xl.RESAMPLE_Q15_SYMBOLS:
        assert hasattr(R, name), name
    for m in ("add", "remove", "feed", "feed_engine", "fetch", "output", "output_device", "produced", "last_feed_ops", "stats", "close"):
        assert callable(getattr(xl.ResamplerBankQ15, m)), m
    assert "hip/" not in hdr and "void *hip_stream" in hdr
    hip = subprocess.run(["nm", "-D", "--defined-only", xl.library_path()], capture_output=True, text=True).stdout
    assert "xlating_resample_q15" not in hip
    # the float bank's header is as it was: the new functions are not declared there
    assert "q15" not in open(os.path.join(ROOT, "include", "xlating_resample.h")).read().lower()


def test_c_caller_builds_against_the_header_alone():
    os.makedirs(BUILD, exist_ok=True)
    demo = os.path.join(BUILD, "resample_q15_demo")
    libdir = os.path.dirname(xl.resample_library_path())
    r = subprocess.run(["gcc", "-std=c11", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), DEMO_SRC, "-o", demo,
                        "-L", libdir, "-lxlating_resample", f"-Wl,-rpath,{libdir}"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    und = subprocess.run(["nm", "-u", demo], capture_output=True, text=True).stdout
    for name in xl.RESAMPLE_Q15_SYMBOLS:
        assert name in und, name
    assert "hip" not in und.lower()
    # a refusal runs end to end without a device
    r = subprocess.run([demo, "null"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and r.stdout.strip() == str(-errno.EINVAL)


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="needs hipcc")
def test_q15_kernels_issue_no_matrix_and_no_packed_fp32(tmp_path):
    """xl_resample_q15.hip compiled for gfx950 with the Makefile's flags: both kernels, no matrix instruction, no v_pk_{mul,add,fma}_f32"""
    mk = open(os.path.join(CSRC, "Makefile")).read()
    m = re.search(r"^RESAMPLE_Q15_FLAGS\s*:=\s*(.+)$", mk, re.M)
    assert m and "-fno-slp-vectorize" in m.group(1)
    assert re.search(r"^\$\(BUILD\)/xl_resample_q15_dev\.o: HIPFLAGS \+= \$\(RESAMPLE_Q15_FLAGS\)$", mk, re.M)
    assert re.search(r"^\$\(BUILD\)/xl_resample_q15_dev\.o: xl_resample_q15\.hip", mk, re.M)
    assert re.search(r"^RESAMP_OBJS :=.*xl_resample_dev\.o.*xl_resample_q15_dev\.o", mk, re.M)
    src = open(os.path.join(CSRC, "xl_resample_q15.hip")).read()
    assert "asm" not in re.sub(r"//[^\n]*", "", src)
    out = str(tmp_path / "k.s")
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fhip-fp32-correctly-rounded-divide-sqrt",
             "--cuda-device-only", "-S"]
    r = subprocess.run(["hipcc"] + flags + m.group(1).split() + [os.path.join(CSRC, "xl_resample_q15.hip"), "-o", out],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    asm = open(out).read()
    assert "xl_rsq_kernel" in asm and "xl_rsq_carry_kernel" in asm
    assert not re.search(r"^\s*v_pk_(mul|add|fma)_f32", asm, re.M)
    assert "v_mfma" not in asm


# ------------------------------------------------------------------------------------------------------------ the admitted filters
@pytest.mark.parametrize("fs,fo", ADMITTED)
def test_admitted_filters_quantise_and_fit_32_bits(fs, fo):
    L, M, taps = admitted_filter(fs, fo)
    c = xl.resample_q15_quantize(taps)  # in range: no -ERANGE
    assert np.array_equal(c.astype(np.int64), QR.quantize(taps))
    sums = QR.phase_abs_sums(L, taps)
    assert sums.shape == (L,) and sums.max() <= 65535, (fs, fo, int(sums.max()))
    print(f"Q15 {fs} -> {fo}: L {L} M {M} taps {taps.size} max |c| {np.abs(c).max()} phase sum |c| {sums.min()} .. {sums.max()} "
          f"phase sum c {QR.table(L, taps).sum(axis=1).min()} .. {QR.table(L, taps).sum(axis=1).max()}")


@pytest.mark.parametrize("fs,fo", ADMITTED)
def test_restatement_is_within_the_derived_distance_of_the_unquantised_filter(fs, fo):
    """|c - h 2^15| < 1 per tap and |x| <= 2^15: an output that did not saturate lies within Q + 1 LSBs of the float64 sum h x"""
    L, M, taps = admitted_filter(fs, fo)
    Q = -(-taps.size // L)
    rng = np.random.default_rng(fo)
    x = rng.integers(-32768, 32768, (4000, 2)).astype(np.int16)
    x[7] = (-32768, 32767)
    s = QR.sums(L, M, taps, x)
    y = QR.restate(L, M, taps, x)
    assert y.shape == (RR.counts(L, M, 4000), 2)
    ideal = np.stack([RR.restate(L, M, taps, x[:, k].astype(np.float32))[0].real for k in range(2)], axis=1)  # float64 sums of h x
    free = ((s >> 15) >= -32768) & ((s >> 15) <= 32767)
    assert free.sum() > free.size // 2
    err = np.abs(y.astype(np.float64) - ideal)[free]
    print(f"Q15 {fs} -> {fo}: Q {Q} largest distance {err.max():.3f} LSB of {Q + 1}, {np.count_nonzero(~free)} saturated")
    assert err.max() < Q + 1
