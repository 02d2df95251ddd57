"""CPU tests (-m "not gpu") of the spectrum bank (include/xlating_spectrum.h, xlating_spectrum_bank_*): the refusals that need no
device, the exported symbols, a C caller built against the header alone, the kernels' scalar-FP32 code object, and the host-side
cutting of a feed into transforms (sdr-server_amd/csrc/xl_spectrum_cut.h, plain C, compiled here with gcc -- with the sanitizers when
XL_SANITIZE_CFLAGS names them, as tests/test_grid.py) against the row / transform positions of tests/spectrogram_ref.py."""
import ctypes as C
import errno
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import sdr_server_amd as xl
from conftest import ROOT

CSRC = os.path.join(ROOT, "sdr-server_amd", "csrc")
DEMO_SRC = os.path.join(ROOT, "tests", "c", "spectrum_bank_demo.c")
DEMO = os.path.join(ROOT, "sdr-server_amd", "build", "spectrum_bank_demo")
BANK_SYMBOLS = ["xlating_spectrum_bank_create", "xlating_spectrum_bank_add", "xlating_spectrum_bank_remove",
                "xlating_spectrum_bank_feed_device", "xlating_spectrum_bank_take_rows", "xlating_spectrum_bank_rows_pending",
                "xlating_spectrum_bank_last_feed_ops", "xlating_spectrum_bank_destroy"]


def _have_gpu():
    try:
        return "no usable device" not in xl.device_info()
    except Exception:
        return False


def test_bank_create_refusals():
    """xlating_spectrum_bank_create's -EINVAL cases are decided before the device is touched"""
    S = xl.spectrum_lib()
    h = C.c_void_p()
    for w, fmt in [(0, 0), (-1, 0), (8193, 0), (64, 1), (64, 4), (64, -1)]:
        assert S.xlating_spectrum_bank_create(w, fmt, C.byref(h)) == -errno.EINVAL, (w, fmt)
    assert S.xlating_spectrum_bank_create(64, 0, None) == -errno.EINVAL
    with pytest.raises(xl.XlatingError) as e:
        xl.SpectrumBank(64, "cs8")
    assert e.value.code == -errno.EINVAL
    # calls on no bank
    assert S.xlating_spectrum_bank_add(None, 48000) == -errno.EINVAL
    assert S.xlating_spectrum_bank_remove(None, 0) == -errno.EINVAL
    assert S.xlating_spectrum_bank_feed_device(None, 0, None, None, None, None) == -errno.EINVAL
    assert S.xlating_spectrum_bank_take_rows(None, 0, None, None, 1) == -errno.EINVAL
    assert S.xlating_spectrum_bank_rows_pending(None, 0) == -errno.EINVAL
    assert S.xlating_spectrum_bank_last_feed_ops(None, None, None) == -errno.EINVAL
    S.xlating_spectrum_bank_destroy(None)


def test_bank_valid_request_without_a_gpu_is_enodev(capfd):
    if _have_gpu():  # (asked here, not at import: tools/sanitize.sh imports this module beside a library without a device probe)
        pytest.skip("checks the no-device answer")
    S = xl.spectrum_lib()
    h = C.c_void_p()
    assert S.xlating_spectrum_bank_create(256, 3, C.byref(h)) == -errno.ENODEV
    assert "<3>" in capfd.readouterr().err
    assert not h.value
    with pytest.raises(xl.XlatingError) as e:
        xl.SpectrumBank(256, "cf32")
    assert e.value.code == -errno.ENODEV


def test_bank_symbols_are_exported_and_declared():
    """test_headers_symbols_are_exported's method, for the bank's functions"""
    src = open(os.path.join(ROOT, "include", "xlating_spectrum.h")).read()
    declared = set(re.findall(r"^(?:int|void)\s+(\w+)\(", src, re.M))
    assert set(BANK_SYMBOLS) <= declared, set(BANK_SYMBOLS) - declared
    assert set(BANK_SYMBOLS) <= set(xl.SPECTRUM_SYMBOLS)
    out = subprocess.run(["nm", "-D", "--defined-only", xl.spectrum_library_path()], capture_output=True, text=True).stdout
    defined = set(re.findall(r" T (\w+)$", out, re.M))
    assert set(BANK_SYMBOLS) <= defined, set(BANK_SYMBOLS) - defined
    S = xl.spectrum_lib()
    for name in BANK_SYMBOLS:
        assert hasattr(S, name), name
    for m in ("add", "remove", "feed", "feed_engine", "take_rows", "rows_pending", "last_feed_ops", "close"):
        assert callable(getattr(xl.SpectrumBank, m)), m
    assert callable(xl.BatchEngine.record_event)


def test_bank_c_caller_builds_against_the_header_alone():
    os.makedirs(os.path.dirname(DEMO), exist_ok=True)
    libdir = os.path.dirname(xl.spectrum_library_path())
    r = subprocess.run(["gcc", "-std=c11", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), DEMO_SRC, "-o", DEMO,
                        "-L", libdir, "-lxlating_spectrum", f"-Wl,-rpath,{libdir}"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    und = subprocess.run(["nm", "-u", DEMO], capture_output=True, text=True).stdout
    for name in BANK_SYMBOLS:
        assert name in und, name
    assert "hip" not in und.lower()
    # a refusal runs end to end without a device
    r = subprocess.run([DEMO, "8193", "0"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and r.stdout.strip() == str(-errno.EINVAL)
    hdr = open(os.path.join(ROOT, "include", "xlating_spectrum.h")).read()
    assert "hip/" not in hdr


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="needs hipcc")
def test_bank_kernels_issue_no_packed_fp32(tmp_path):
    """test_spectrum_kernels_issue_no_packed_fp32's method: xl_spectrum_bank.hip is compiled with SPEC_FLAGS, and its gfx950 code
    holds no v_pk_{mul,add,fma}_f32 and no matrix instruction"""
    mk = open(os.path.join(CSRC, "Makefile")).read()
    m = re.search(r"^SPEC_FLAGS\s*:=\s*(.+)$", mk, re.M)
    assert m and "-fno-slp-vectorize" in m.group(1)
    assert re.search(r"^\$\(BUILD\)/xl_spectrum_bank_dev\.o: HIPFLAGS \+= \$\(SPEC_FLAGS\)$", mk, re.M)
    assert re.search(r"^\$\(BUILD\)/xl_spectrum_bank_dev\.o: xl_spectrum_bank\.hip", mk, re.M)
    out = str(tmp_path / "k.s")
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fhip-fp32-correctly-rounded-divide-sqrt",
             "--cuda-device-only", "-S"]
    r = subprocess.run(["hipcc"] + flags + m.group(1).split() + [os.path.join(CSRC, "xl_spectrum_bank.hip"), "-o", out],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    asm = open(out).read()
    assert "xl_bank_kernel" in asm and "xl_bank_finish_kernel" in asm and "xl_bank_carry_kernel" in asm
    assert not re.search(r"^\s*v_pk_(mul|add|fma)_f32", asm, re.M)
    assert "v_mfma" not in asm


def test_bank_knob_goes_through_the_gate():
    src = open(os.path.join(CSRC, "xl_spectrum_bank.cpp")).read()
    assert 'xl_exp_getenv("XL_EXP_SPEC_BANK_SLOTS")' in src
    assert not re.findall(r'(?<!xl_exp_)getenv\(', src)


def test_bank_and_single_kernels_share_the_transform_arithmetic():
    """the bit-identity of bank rows and single-object rows rests on one definition of everything a workgroup does after its kernel's
    prologue: the pack body (load, transforms, power, row maximum and its flush) and the finishing of a bin are defined in
    xl_spectrum_dev.h only, both kernel files call them, and neither transforms or flushes a maximum on its own"""
    dev = open(os.path.join(CSRC, "xl_spectrum_dev.h")).read()
    for name in ("xl_fft_lds", "xl_spec_point", "xl_spec_blue_mid", "xl_spec_power", "xl_spec_max_bits", "xl_spec_db", "xl_spec_pixel",
                 "xl_spec_shift_src", "xl_spec_pack", "xl_spec_finish_bin"):
        assert len(re.findall(r"^XL_DEV \w+ %s\(" % name, dev, re.M)) == 1, name
    assert "atomicMax" in dev
    # a power's bits enter a maximum through xl_spec_max_bits only (the reference's fmaxf rule for a NaN power)
    assert len(re.findall(r"__float_as_uint\(", re.sub(r"//[^\n]*", "", dev))) == 1
    for f in ("xl_spectrum.hip", "xl_spectrum_bank.hip"):
        src = open(os.path.join(CSRC, f)).read()
        code = re.sub(r"//[^\n]*", "", src)  # (the headers' prose names what the shared body does)
        assert '#include "xl_spectrum_dev.h"' in src
        assert not re.search(r"XL_DEV \w+ xl_", src), f
        assert len(re.findall(r"\bxl_spec_pack<N, FMT, BLUE>\(", code)) == 1, f
        assert len(re.findall(r"\bxl_spec_finish_bin\(", code)) == 1, f
        assert len(re.findall(r"\bxl_spec_dispatch\(", code)) == 1, f
        for own in ("atomicMax", "xl_fft_lds", "xl_spec_point", "xl_spec_power", "xl_spec_db", "xl_spec_pixel", "case "):
            assert own not in code, (f, own)


# ------------------------------------------------------------------------------------------------------------ the cutting of a feed
SHIM = r"""
#include "xl_spectrum_cut.h"
void cut(int64_t sr, int64_t W, int64_t P0, int64_t n, int64_t *o) {
  XlSpecCut c = xl_spec_cut(sr, W, P0, n);
  o[0] = c.carry_have, o[1] = c.carry_app, o[2] = c.carry_done, o[3] = c.carry_g, o[4] = c.carry_t0;
  o[5] = c.g_first, o[6] = c.T, o[7] = c.save_off, o[8] = c.save_n, o[9] = c.rows_done;
}
int64_t round_limit(int64_t sr, int64_t P0, int64_t slots) { return xl_spec_round_limit(sr, P0, slots); }
"""
FIELDS = ["carry_have", "carry_app", "carry_done", "carry_g", "carry_t0", "g_first", "T", "save_off", "save_n", "rows_done"]


@pytest.fixture(scope="module")
def cutlib(tmp_path_factory):
    d = tmp_path_factory.mktemp("cut")
    src = d / "shim.c"
    src.write_text(SHIM)
    so = d / "libcut.so"
    extra = os.environ.get("XL_SANITIZE_CFLAGS", "").split()  # (tools/sanitize.sh: -fsanitize=address,undefined)
    subprocess.run(["gcc", "-O1", "-Wall", "-Werror", "-shared", "-fPIC"] + extra + ["-I", CSRC, str(src), "-o", str(so)], check=True)
    L = C.CDLL(str(so))
    L.cut.argtypes = [C.c_int64] * 4 + [C.POINTER(C.c_int64)]
    L.cut.restype = None
    L.round_limit.argtypes = [C.c_int64] * 3
    L.round_limit.restype = C.c_int64
    return L


def transform_starts(sr, W, samples):
    """the first sample of every transform of the first `samples` samples of a stream, in order, by the layout of
    spectrogram_ref.power_rows: rows of sr samples, of each the first F * W cut into F pieces of W (an index array through the same
    reshapes); plus the transforms of the unfinished last row, which a stream computes as its samples arrive"""
    F = sr // W
    H = samples // sr + 1
    idx = np.arange(H * sr).reshape(H, sr)[:, :F * W].reshape(H, F, W)
    return idx[:, :, 0].reshape(-1)


def cut_by_positions(sr, W, P0, n):
    """what a feed of samples P0 .. P0 + n - 1 holds, from the transform positions alone"""
    F, P1 = sr // W, P0 + n
    st = transform_starts(sr, W, P1 + sr)
    want = dict.fromkeys(FIELDS, 0)
    whole = np.nonzero((st >= P0) & (st + W <= P1))[0]
    want["T"] = whole.size
    # (g_first is only meaningful with T > 0, and then it is the first whole transform)
    want["g_first"] = int(whole[0]) if whole.size else None
    if n > 0:
        before = np.nonzero((st < P0) & (st + W > P0))[0]
        if before.size:
            g = int(before[0])
            want.update(carry_have=P0 - int(st[g]), carry_app=min(int(st[g]) + W, P1) - P0, carry_done=int(int(st[g]) + W <= P1),
                        carry_g=g, carry_t0=int(st[g]))
        after = np.nonzero((st >= P0) & (st < P1) & (st + W > P1))[0]
        if after.size:
            g = int(after[0])
            want.update(save_off=int(st[g]) - P0, save_n=P1 - int(st[g]))
    # row r is complete once its F-th transform is in
    ends = st.reshape(-1, F)[:, -1] + W
    want["rows_done"] = int((ends <= P1).sum())
    return want


def test_cut_matches_the_transform_positions(cutlib):
    rng = np.random.default_rng(2024)
    o = (C.c_int64 * 10)()
    checked = 0
    for case in range(300):
        W = int(rng.choice([1, 2, 3, 7, 16, 64, 100, 256, 1000]))
        kind = case % 5
        sr = [W, 3 * W + (W // 2 + 1 if W > 1 else 0), W * int(rng.integers(1, 40)), W * int(rng.integers(1, 9)) + int(rng.integers(0, W)),
              W + int(rng.integers(0, 3 * W + 1))][kind]
        P = 0
        for _ in range(25):
            n = int(rng.choice([0, 1, W - 1, W, W + 1, sr - 1, sr, sr + 1, 2 * sr + W // 2, int(rng.integers(0, 4 * sr + 2))]))
            n = max(n, 0)
            cutlib.cut(sr, W, P, n, o)
            got = dict(zip(FIELDS, list(o)))
            want = cut_by_positions(sr, W, P, n)
            if want["g_first"] is None:
                want["g_first"] = got["g_first"]
            assert got == want, (sr, W, P, n)
            P += n
            checked += 1
    assert checked == 300 * 25


def test_feeds_cover_every_transform_once(cutlib):
    """over a sequence of feeds, cut into rounds as the bank cuts them: the completed carries and the whole transforms are exactly the
    stream's transforms, each once and in order; the carry is continued consistently; a round touches at most `slots` rows, all
    distinct modulo `slots`"""
    rng = np.random.default_rng(7)
    o = (C.c_int64 * 10)()
    for case in range(120):
        W = int(rng.choice([1, 3, 8, 64, 100]))
        sr = W * int(rng.integers(1, 6)) + int(rng.integers(0, W))
        F = sr // W
        slots = int(rng.choice([1, 2, 3, 16]))
        P, seen, carry = 0, [], 0
        for _ in range(30):
            rem = int(rng.integers(0, 6 * sr))
            while rem > 0:
                lim = cutlib.round_limit(sr, P, slots)
                assert lim > 0
                c = min(rem, lim)
                cutlib.cut(sr, W, P, c, o)
                k = dict(zip(FIELDS, list(o)))
                touched = []
                if k["carry_app"] > 0:
                    assert k["carry_have"] == carry and carry > 0 and k["carry_have"] + k["carry_app"] <= W
                    carry += k["carry_app"]
                    if k["carry_done"]:
                        assert carry == W
                        seen.append(k["carry_g"])
                        touched.append(k["carry_g"])
                        carry = 0
                else:
                    assert carry == 0 or c == 0
                seen.extend(range(k["g_first"], k["g_first"] + k["T"]))
                touched.extend(range(k["g_first"], k["g_first"] + k["T"]))
                if k["save_n"] > 0:
                    assert carry == 0 and 0 < k["save_n"] < W and k["save_off"] + k["save_n"] == c
                    carry = k["save_n"]
                rows = sorted({g // F for g in touched})
                if rows:
                    assert rows[0] >= P // sr and rows[-1] < P // sr + slots, (sr, W, slots, P, c, rows)
                P += c
                rem -= c
                assert k["rows_done"] == (0 if P < F * W else (P - F * W) // sr + 1)
        st = transform_starts(sr, W, P)
        total = int(((st + W) <= P).sum())
        assert seen == list(range(total)), (sr, W, slots)
