"""CPU tests (-m "not gpu") of the resampler bank (include/xlating_resample.h) and of the admission in front of it
(xlating_wire_admit_any_rate): the refusals that need no device, the exported symbols, a C caller built against the header alone, the
kernels' scalar-FP32 code object, the admission rule against its table and against xlating_wire_admit, and the host-side cut of a
feed (sdr-server_amd/csrc/xl_resample_cut.h, plain C) against a brute-force enumeration of the outputs' positions -- through a gcc
shim here, and once more as a stand-alone program under the sanitizers."""
import ctypes as C
import errno
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import resample_ref as RR
import sdr_server_amd as xl
from conftest import ROOT

CSRC = os.path.join(ROOT, "sdr-server_amd", "csrc")
BUILD = os.path.join(ROOT, "sdr-server_amd", "build")
DEMO_SRC = os.path.join(ROOT, "tests", "c", "resample_bank_demo.c")
SWEEP_SRC = os.path.join(ROOT, "tests", "c", "resample_cut_sweep.c")


def _have_gpu():
    try:
        return "no usable device" not in xl.device_info()
    except Exception:
        return False


# ------------------------------------------------------------------------------------------------------------ refusals, symbols
def test_refusals_need_no_device():
    R = xl.resample_lib()
    one = (C.c_float * 1)(1.0)
    assert R.xlating_resample_bank_create(None) == -errno.EINVAL
    assert R.xlating_resample_bank_add(None, 1, 1, one, 1) == -errno.EINVAL
    assert R.xlating_resample_bank_remove(None, 0) == -errno.EINVAL
    assert R.xlating_resample_bank_feed_device(None, 0, None, None, None, None) == -errno.EINVAL
    p, n, f = C.c_void_p(), C.c_size_t(0), C.POINTER(C.c_float)()
    assert R.xlating_resample_bank_output_device(None, 0, C.byref(p), C.byref(n)) == -errno.EINVAL
    assert R.xlating_resample_bank_fetch(None) == -errno.EINVAL
    assert R.xlating_resample_bank_output_host(None, 0, C.byref(f), C.byref(n)) == -errno.EINVAL
    assert R.xlating_resample_bank_produced(None, 0) == 0
    assert R.xlating_resample_bank_last_feed_ops(None, None, None) == -errno.EINVAL
    assert R.xlating_resample_bank_stats(None, None, None, None) == -errno.EINVAL
    R.xlating_resample_bank_destroy(None)


def test_valid_create_without_a_gpu_is_enodev(capfd):
    if _have_gpu():
        pytest.skip("checks the no-device answer")
    R = xl.resample_lib()
    h = C.c_void_p()
    assert R.xlating_resample_bank_create(C.byref(h)) == -errno.ENODEV
    assert "<3>" in capfd.readouterr().err
    assert not h.value
    with pytest.raises(xl.XlatingError) as e:
        xl.ResamplerBank()
    assert e.value.code == -errno.ENODEV


def test_add_refusals_are_decided_before_the_device():
    """every -EINVAL of add is an argument check placed before the first HIP call of the function (there is no bank to ask on a
    machine without a GPU, so this reads the order in the source; tests/test_resample_gpu.py asks a live bank)"""
    src = open(os.path.join(CSRC, "xl_resample.cpp")).read()
    body = src[src.index('extern "C" int xlating_resample_bank_add('):]
    body = body[:body.index("\n}\n")]
    first_hip = body.index("hip")
    checks = body[:first_hip]
    for cond in ("L == 0u", "M == 0u", "L > XLATING_RESAMPLE_MAX_L", "M >= (1u << 31)", "taps == nullptr", "taps_len == 0",
                 "(taps_len + L - 1u) / L > XLATING_RESAMPLE_MAX_Q", "xl_rs_gcd(L, M) != 1u"):
        assert cond in checks, cond
    assert "return -EINVAL;" in checks
    hdr = open(os.path.join(ROOT, "include", "xlating_resample.h")).read()
    assert re.search(r"#define XLATING_RESAMPLE_MAX_L 4096\b", hdr) and re.search(r"#define XLATING_RESAMPLE_MAX_Q 1024\b", hdr)


def test_symbols_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "xlating_resample.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"^(?:int|void|uint64_t)\s+(\w+)\(", code, re.M))
    assert declared == set(xl.RESAMPLE_SYMBOLS), declared ^ set(xl.RESAMPLE_SYMBOLS)
    out = subprocess.run(["nm", "-D", "--defined-only", xl.resample_library_path()], capture_output=True, text=True).stdout
    defined = set(re.findall(r" T (\w+)$", out, re.M))
    assert set(xl.RESAMPLE_SYMBOLS) <= defined, set(xl.RESAMPLE_SYMBOLS) - defined
    R = xl.resample_lib()
    for name in xl.RESAMPLE_SYMBOLS:
        assert hasattr(R, name), name
    for m in ("add", "remove", "feed", "feed_engine", "fetch", "output", "output_device", "produced", "last_feed_ops", "stats", "close"):
        assert callable(getattr(xl.ResamplerBank, m)), m
    assert callable(xl.wire_admit_any_rate) and callable(xl.wire_resample_taps)
    for name in ("xlating_wire_admit_any_rate", "xlating_wire_resample_taps"):
        assert name in xl.EXPORTED_SYMBOLS and hasattr(xl.lib(), name)
    assert "hip/" not in hdr and "void *hip_stream" in hdr
    # the engine's library is not what carries the bank: only the admission functions were added to it
    hip = subprocess.run(["nm", "-D", "--defined-only", xl.library_path()], capture_output=True, text=True).stdout
    assert "xlating_resample_bank" not in hip
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^all:.*\$\(RESAMP\)", mk, re.M)


def test_c_caller_builds_against_the_header_alone():
    os.makedirs(BUILD, exist_ok=True)
    demo = os.path.join(BUILD, "resample_bank_demo")
    libdir = os.path.dirname(xl.resample_library_path())
    r = subprocess.run(["gcc", "-std=c11", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), DEMO_SRC, "-o", demo,
                        "-L", libdir, "-lxlating_resample", f"-Wl,-rpath,{libdir}"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    und = subprocess.run(["nm", "-u", demo], capture_output=True, text=True).stdout
    for name in xl.RESAMPLE_SYMBOLS:
        assert name in und, name
    assert "hip" not in und.lower()
    # a refusal runs end to end without a device
    r = subprocess.run([demo, "null"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and r.stdout.strip() == str(-errno.EINVAL)


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="needs hipcc")
def test_resample_kernels_issue_no_packed_fp32(tmp_path):
    """test_spectrum_kernels_issue_no_packed_fp32's method: xl_resample.hip is compiled with RESAMPLE_FLAGS, and its gfx950 code holds
    no v_pk_{mul,add,fma}_f32, no matrix instruction and -- the sum is unfused by definition -- no fused multiply-add"""
    mk = open(os.path.join(CSRC, "Makefile")).read()
    m = re.search(r"^RESAMPLE_FLAGS\s*:=\s*(.+)$", mk, re.M)
    assert m and "-fno-slp-vectorize" in m.group(1)
    assert re.search(r"^\$\(BUILD\)/xl_resample_dev\.o: HIPFLAGS \+= \$\(RESAMPLE_FLAGS\)$", mk, re.M)
    assert re.search(r"^\$\(BUILD\)/xl_resample_dev\.o: xl_resample\.hip", mk, re.M)
    src = open(os.path.join(CSRC, "xl_resample.hip")).read()
    assert "asm" not in re.sub(r"//[^\n]*", "", src)
    out = str(tmp_path / "k.s")
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fhip-fp32-correctly-rounded-divide-sqrt",
             "--cuda-device-only", "-S"]
    r = subprocess.run(["hipcc"] + flags + m.group(1).split() + [os.path.join(CSRC, "xl_resample.hip"), "-o", out],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    asm = open(out).read()
    assert "xl_rs_kernel" in asm and "xl_rs_carry_kernel" in asm
    assert not re.search(r"^\s*v_pk_(mul|add|fma)_f32", asm, re.M)
    assert "v_mfma" not in asm
    assert not re.search(r"^\s*v_(fma|fmac|mad|mac)_f32", asm, re.M)


# ------------------------------------------------------------------------------------------------------------ admission
TABLE = [  # fs, fo, D, L, M, taps, Q
    (10000000, 48000, 125, 3, 5, 61, 21),
    (20000000, 48000, 250, 3, 5, 61, 21),
    (2016000, 44100, 40, 7, 8, 97, 14),
    (2400000, 44100, 50, 147, 160, 1927, 14),
    (10000000, 44100, 200, 441, 500, 6023, 14),
    (2048000, 48000, 32, 3, 4, 49, 17),
    (2400000, 2000000, 1, 5, 6, 73, 15),
    (2016000, 48000, 42, 1, 1, None, None),
]


def rule(fs, fo):
    """the issue's rule, restated: -> (D, L, M) or None"""
    dmax = fs // fo
    best = None
    for D in range(dmax // 2 + 1, dmax + 1):
        g = math.gcd(fo * D, fs)
        L, M = fo * D // g, fs // g
        if L <= 4096 and fo * M <= 0xFFFFFFFF and (best is None or L <= best[1]):
            best = (D, L, M)
    return best


def request(fs, fo, band=460100000, center=None):
    return xl.WireRequest(band + 1000 if center is None else center, fo, band, 0)


@pytest.mark.parametrize("fs,fo,D,L,M,ntaps,Q", TABLE)
def test_admission_table(fs, fo, D, L, M, ntaps, Q):
    req = request(fs, fo)
    code, adm, rs, why = xl.wire_admit_any_rate(req, fs, 0, 5)
    assert code == 0 and why == 0
    assert (adm.decimation, rs.L, rs.M) == (D, L, M)
    assert adm.lpf_cutoff == fo // 2 and adm.lpf_transition == fo // 5 and adm.center_offset == 1000
    if (L, M) == (1, 1):
        code1, adm1, why1 = xl.wire_admit(req, fs, 0, 5)
        assert code1 == 0 and bytes(adm1) == bytes(adm)
        return
    assert rs.virtual_rate == fo * M and rs.virtual_rate * D == L * fs
    assert fo <= fs / D < 2 * fo
    assert xl.wire_admit(req, fs, 0, 5)[0] == -errno.EINVAL and xl.wire_admit(req, fs, 0, 5)[2] == 1
    code, taps = xl.wire_resample_taps(req, rs, 5)
    assert code == 0 and taps.dtype == np.float32
    assert taps.size == ntaps and -(-taps.size // L) == Q
    want = xl.create_low_pass_filter(float(L), rs.virtual_rate, fo // 2, fo // 5)[1]
    assert np.array_equal(taps.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("fs,fo", [(10000000, 9999), (3000000, 2999999), (1000003, 48000)])
def test_admission_refuses_without_an_eligible_decimation(fs, fo):
    assert rule(fs, fo) is None
    code, adm, rs, why = xl.wire_admit_any_rate(request(fs, fo, band=460100000), fs, 0, 5)
    assert code == -errno.EINVAL and why == 1


def test_admission_equals_the_rule_on_random_rates():
    rng = np.random.default_rng(11)
    for _ in range(300):
        fs = int(rng.choice([2016000, 2400000, 10000000, 20000000, 2048000, 1000003, 192000]))
        fo = int(rng.integers(1000, fs))
        code, adm, rs, why = xl.wire_admit_any_rate(request(fs, fo, center=460100000), fs, 0, 5)
        if fs % fo == 0:
            assert code == 0 and (rs.L, rs.M) == (1, 1)
            continue
        want = rule(fs, fo)
        if want is None:
            assert code == -errno.EINVAL and why == 1, (fs, fo)
        else:
            assert code == 0 and (adm.decimation, rs.L, rs.M) == want, (fs, fo, want)


def test_admission_search_is_bounded():
    """the rate comes from the network: a tiny rate on a wide band is answered at once, and as the rule says"""
    import time

    t0 = time.perf_counter()
    for fs, fo in [(4000000007, 3), (4294967295, 2), (4294967291, 7), (20000000, 7)]:
        code, adm, rs, why = xl.wire_admit_any_rate(request(fs, fo, band=2200000000, center=2200000000), fs, 0, 5)
        if fs < 100000000:
            want = rule(fs, fo)
            assert (code == 0 and (adm.decimation, rs.L, rs.M) == want) if want else code == -errno.EINVAL
    assert time.perf_counter() - t0 < 2.0


def test_admission_of_dividing_rates_equals_admit():
    """200 random requests whose rate divides the band rate, valid and invalid ones: field for field xlating_wire_admit's, L = M = 1"""
    rng = np.random.default_rng(5)
    seen = set()
    for _ in range(200):
        fs = int(rng.choice([2016000, 2400000, 10000000, 192000]))
        divs = [d for d in range(1, 2000) if fs % d == 0]
        fo = fs // int(rng.choice(divs))
        band = int(rng.choice([460100000, 100000000, 0]))
        center = int(band + rng.integers(-fs, fs)) if rng.random() < 0.8 else 0
        dest = int(rng.choice([0, 1, 1, 2]))
        cur = int(rng.choice([0, 0, band, 433000000]))
        req = xl.WireRequest(center & 0xFFFFFFFF, fo, band, dest)
        c0, a0, w0 = xl.wire_admit(req, fs, cur, 5)
        c1, a1, rs, w1 = xl.wire_admit_any_rate(req, fs, cur, 5)
        assert (c0, w0) == (c1, w1), (fs, fo, band, center, dest, cur)
        if c0 == 0:
            assert bytes(a0) == bytes(a1) and (rs.L, rs.M, rs.virtual_rate) == (1, 1, fo)
        seen.add((c0, w0))
    assert {(0, 0), (-errno.EINVAL, 1), (-errno.EINVAL, 2)} <= seen


def test_admission_checks_keep_their_order_for_other_rates():
    """a rate that does not divide: the other checks answer as xlating_wire_admit answers a dividing rate in the same place"""
    fs, fo, band = 2016000, 44100, 460100000
    ok = xl.WireRequest(band + 5000, fo, band, 0)
    assert xl.wire_admit_any_rate(ok, fs, 0, 5)[0] == 0
    assert xl.wire_admit_any_rate(ok, fs, band, 5)[0] == 0
    assert xl.wire_admit_any_rate(ok, fs, band + 1, 5)[3] == 2  # OUT_OF_BAND_FREQ
    for bad in (xl.WireRequest(0, fo, band, 0), xl.WireRequest(band, fo, 0, 0), xl.WireRequest(band, fo, band, 2),
                xl.WireRequest(band + fs // 2, fo, band, 0), xl.WireRequest(band - fs // 2, fo, band, 0)):
        code, _, _, why = xl.wire_admit_any_rate(bad, fs, band + 1, 5)
        assert code == -errno.EINVAL and why == 1
    # the edge: the client's half-width is its own rate's
    assert xl.wire_admit_any_rate(xl.WireRequest(band + fs // 2 - fo // 2, fo, band, 0), fs, 0, 5)[0] == 0
    assert xl.wire_admit_any_rate(xl.WireRequest(band + fs // 2 - fo // 2 + 1, fo, band, 0), fs, 0, 5)[0] == -errno.EINVAL
    L = xl.lib()
    adm, rs, why = xl.WireAdmission(), xl.WireResample(), C.c_uint32(0)
    assert L.xlating_wire_admit_any_rate(C.byref(ok), fs, 0, 5, C.byref(adm), None, C.byref(why)) == -errno.EINVAL
    assert L.xlating_wire_admit_any_rate(None, fs, 0, 5, C.byref(adm), C.byref(rs), C.byref(why)) == -errno.EINVAL
    assert L.xlating_wire_admit_any_rate(C.byref(ok), fs, 0, 0, C.byref(adm), C.byref(rs), C.byref(why)) == -errno.EINVAL
    assert L.xlating_wire_admit_any_rate(C.byref(ok), fs, 0, 5, C.byref(adm), C.byref(rs), None) == 0


# ------------------------------------------------------------------------------------------------------------ the cut
SHIM = r"""
#include "xl_resample_cut.h"
void cut(uint32_t L, uint32_t M, uint32_t Q, uint64_t P0, uint64_t n, int64_t *o) {
  XlResampleCut c = xl_resample_cut(L, M, Q, P0, n);
  o[0] = (int64_t)c.m_first, o[1] = (int64_t)c.count, o[2] = c.n_first, o[3] = c.p_first, o[4] = c.carry_new, o[5] = c.carry_old;
}
uint64_t produced(uint64_t L, uint64_t M, uint64_t P) { return xl_resample_produced(L, M, P); }
"""
RATIOS = [(1, 1), (1, 3), (3, 1), (2, 3), (7, 8), (624, 625), (4096, 4095)]


@pytest.fixture(scope="module")
def cutlib(tmp_path_factory):
    d = tmp_path_factory.mktemp("rscut")
    src = d / "shim.c"
    src.write_text(SHIM)
    so = d / "librscut.so"
    subprocess.run(["gcc", "-O1", "-Wall", "-Werror", "-shared", "-fPIC", "-I", CSRC, str(src), "-o", str(so)], check=True)
    L = C.CDLL(str(so))
    L.cut.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, C.POINTER(C.c_int64)]
    L.cut.restype = None
    L.produced.argtypes = [C.c_uint64] * 3
    L.produced.restype = C.c_uint64
    return L


def brute(L, M, P0, n):
    """the outputs whose n_m lies in [P0, P0 + n), by walking m (Python integers): -> (m_first, count, n_first - P0, p_first)"""
    m = (P0 * L) // M  # at or just below the first; walk up
    while (m * M) // L < P0:
        m += 1
    while m > 0 and ((m - 1) * M) // L >= P0:
        m -= 1
    k = 0
    while ((m + k) * M) // L < P0 + n:
        k += 1
    return m, k, (m * M) // L - P0, (m * M) % L


@pytest.mark.parametrize("L,M", RATIOS)
def test_cut_matches_the_enumeration(cutlib, L, M):
    rng = np.random.default_rng(1000 * L + M)
    o = (C.c_int64 * 6)()
    for Q in (1, 2, 14, 21, 1024):
        for P_start in (0, int(rng.integers(1, 5000)), (1 << 40) - int(rng.integers(0, 3000)), int(rng.integers(1 << 39, 1 << 40))):
            P, total = P_start, 0
            for _ in range(30):
                n = int(rng.choice([0, 1, max(Q - 2, 0), Q - 1, Q, int(rng.integers(0, 3000)), int(rng.integers(0, 3 * M // L + 2))]))
                cutlib.cut(L, M, Q, P, n, o)
                m_first, count, n_first, p_first, carry_new, carry_old = list(o)
                want = brute(L, M, P, n)
                assert (m_first, count, n_first, p_first) == want, (L, M, Q, P, n)
                if count:
                    assert 0 <= n_first < n and 0 <= p_first < L
                assert carry_new == min(n, Q - 1) and carry_new + carry_old == Q - 1
                P += n
                total += count
            assert total == RR.counts(L, M, P) - RR.counts(L, M, P_start)
            assert cutlib.produced(L, M, P) == RR.counts(L, M, P)
            if P_start == 0:
                assert total == -((-P * L) // M)  # ceil(N L / M)


def test_cut_sweep_under_the_sanitizers(tmp_path):
    """the same sweep as a stand-alone C program with its own main, built with ASan and UBSan and run as a process of its own"""
    exe = str(tmp_path / "resample_cut_sweep")
    r = subprocess.run(["gcc", "-std=c11", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I", CSRC, SWEEP_SRC, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok "), (r.stdout[-500:], r.stderr[-2000:])
    assert int(r.stdout.split()[1]) >= 5000


def test_the_bank_cuts_with_the_header_only():
    """the bank's host code calls nothing else for this arithmetic: no division or remainder by L or M of its own"""
    src = re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, "xl_resample.cpp")).read())
    assert '#include "xl_resample_cut.h"' in src
    assert len(re.findall(r"\bxl_resample_cut\(", src)) == 1 and len(re.findall(r"\bxl_resample_produced\(", src)) == 1
    assert not re.search(r"[/%*]\s*s\.t->[LM]\b", src)  # (a stream's position is never computed beside the header)
    cut = open(os.path.join(CSRC, "xl_resample_cut.h")).read()
    assert "hip" not in cut.lower().replace("no hip", "") and "#include <stdint.h>" in cut
