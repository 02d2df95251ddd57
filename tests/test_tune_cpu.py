"""CPU tests (-m "not gpu") of the tuner bank (include/xlating_tune.h) and of tuning in the serve object: the rule header is plain C and
passes its sweep as a program of its own under ASan and UBSan -- xl_tune_cs against libm over all 2^32 phases, the phase arithmetic
against 128-bit integers, from_hz against the stated expression; the restatement's pieces against the library's; the exported symbols;
the refusals that need no device; the kernel's code object (scalar FP32 only, no matrix instruction, no scratch)."""
import ctypes as C
import errno
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import sdr_server_amd as xl
import tune_ref as TR
from conftest import ROOT

CSRC = os.path.join(ROOT, "sdr-server_amd", "csrc")
RULE = os.path.join(CSRC, "xl_tune_rule.h")
KERNEL = os.path.join(CSRC, "xl_tune.hip")


def _strip(path):
    return re.sub(r"/\*.*?\*/", "", re.sub(r"//[^\n]*", "", open(path).read()), flags=re.S)


def test_rule_header_is_plain_c(tmp_path):
    code = _strip(RULE)
    assert re.findall(r"#include\s*(\S+)", code) == ["<stdint.h>"], "no libm in what the device runs: the steps from Hz are xl_tune_hz.h's"
    assert "xl_tune_hz.h" not in _strip(KERNEL)
    assert "#include <hip" not in code and "asm" not in code and "__builtin" not in code and "[" not in code, "no intrinsic, no table"
    body = code[code.index("void xl_tune_cs("):code.index("xl_tune_rotate(")]
    assert not re.search(r"\b(sin|cos|sincos|fma)f?\s*\(", body) and "double" not in body, "float32 polynomials, no libm"
    src = tmp_path / "t.c"
    src.write_text('#include "xl_tune_rule.h"\nint main(void) { float c, s; xl_tune_cs(0x40000000u, &c, &s); return c == 0.0f && s == 1.0f ? 0 : 1; }\n')
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-pedantic", "-ffp-contract=off", "-I", CSRC, str(src), "-o", str(tmp_path / "t"), "-lm"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert subprocess.run([str(tmp_path / "t")]).returncode == 0


def test_rule_sweep_under_the_sanitizers():
    """all 2^32 phases, the exact points and both symmetries (asserted by the program), E <= 2^-22 (asserted there per part and here
    for the whole); the phase arithmetic and from_hz"""
    r = TR.sweep()
    print(f"E = {r['E'].hex()} = {r['E'] * 2 ** 24:.4f} * 2^-24; max |c^2 + s^2 - 1| = {r['circle'].hex()} = {r['circle'] * 2 ** 24:.4f} * 2^-24")
    assert r["phases"] == 1 << 32
    assert 0.0 < r["E"] <= 2.0 ** -22
    assert r["circle"] <= 4 * r["E"] + 2.0 ** -40  # (|c^2 + s^2 - 1| <= 2 E (|c| + |s|) + 2 E^2: an error of that size is no other's)
    assert r["phase_checks"] >= 1000000 and r["hz_checks"] >= 500


def test_design_states_the_measured_error():
    """DESIGN 3.11 carries E as the sweep printed it: the GPU accuracy test takes its E from there (tune_ref.design_E)"""
    assert TR.design_E() == TR.sweep()["E"]


def test_restatement_against_the_library():
    for k in range(8):
        c, s = xl.tune_cs(k << 30)
        assert (float(c), float(s)) == [(1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0)][k % 4]
    rng = np.random.default_rng(3)
    for p in [1, 2, (1 << 29) - 1, 1 << 29, (1 << 29) + 1, (1 << 31) - 1, (1 << 32) - 1] + [int(v) for v in rng.integers(0, 1 << 32, 200)]:
        c, s = xl.tune_cs(p)
        t = 2 * np.pi * p / 2.0 ** 32
        assert abs(float(c) - np.cos(t)) <= 2.0 ** -22 and abs(float(s) - np.sin(t)) <= 2.0 ** -22
        c1, s1 = xl.tune_cs(p + (1 << 30))
        c2, s2 = xl.tune_cs(-p)
        assert (c1, s1) == (-s, c) and (c2, s2) == (c, -s)
    rates = [48000.0, 44100.0, 2016000.0 / 42, 2016000.0 * 160 / (42.0 * 147)]
    for rate in rates:
        for sh, ra in [(0, 0), (1, 0), (-1, 0), (1234.5, -77.25), (-10000, 300), (0.1, 1e-3), (rate * 0.4999, 0)]:
            assert xl.tune_from_hz(sh, ra, rate) == TR.from_hz(sh, ra, rate), (sh, ra, rate)
    assert xl.tune_from_hz(12000, 0, 48000) == (1 << 62, 0)
    for sh, ra, rate in [(24000, 0, 48000), (-24000, 0, 48000), (0, 0.5, 1), (1, 0, 0), (float("nan"), 0, 48000), (0, float("inf"), 48000)]:
        with pytest.raises(xl.XlatingError) as e:
            xl.tune_from_hz(sh, ra, rate)
        assert e.value.code == -errno.EINVAL
    # the restatement's integers: wrap, split, sign
    P, F, R = (1 << 64) - 1, -(1 << 63), (1 << 63) - 1
    assert TR.phase(P, F, R, 0) == P and TR.phase(P, 1, 0, 1) == 0
    a = TR.advance(*TR.advance(P, F, R, 1000), 2049)
    assert a == TR.advance(P, F, R, 3049) and -(1 << 63) <= a[1] < (1 << 63)
    x = (np.arange(5) + 1j).astype(np.complex64)
    y, st = TR.rotate(x, 0, 1 << 62, 0)  # a quarter turn a sample
    assert np.array_equal(y, x * np.array([1, 1j, -1, -1j, 1], np.complex64)) and st == (1 << 62, 1 << 62, 0)


def test_symbols_are_exported():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "xlating_tune.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(xlating_tune_[a-z_0-9]+)\s*\(", hdr))
    assert declared == set(xl.TUNE_SYMBOLS), declared ^ set(xl.TUNE_SYMBOLS)
    out = subprocess.run(["nm", "-D", "--defined-only", xl.tune_library_path()], capture_output=True, text=True).stdout
    defined = {l.split()[-1] for l in out.splitlines() if l.strip()}
    assert set(xl.TUNE_SYMBOLS) <= defined, set(xl.TUNE_SYMBOLS) - defined
    T, V = xl.tune_lib(), xl.serve_lib()
    for name in xl.TUNE_SYMBOLS:
        assert hasattr(T, name), name
    for name in ("xlating_serve_set_tune", "xlating_serve_tune_log"):
        assert name in xl.SERVE_SYMBOLS and hasattr(V, name), name
    needed = subprocess.run(["readelf", "-d", xl.serve_library_path()], capture_output=True, text=True).stdout
    assert "libxlating_tune.so" in needed
    assert xl.tune_chunk_samples() == 2048


def test_refusals_need_no_device():
    T, V = xl.tune_lib(), xl.serve_lib()
    assert T.xlating_tune_bank_create(None) == -errno.EINVAL
    assert T.xlating_tune_bank_add(None, 0, 0, 0) == -errno.EINVAL
    assert T.xlating_tune_bank_remove(None, 0) == -errno.EINVAL and T.xlating_tune_bank_set(None, 0, 0, 0) == -errno.EINVAL
    one = (C.c_int * 1)(0)
    assert T.xlating_tune_bank_feed_device(None, 1, one, one, one, None) == -errno.EINVAL
    assert T.xlating_tune_bank_output_device(None, 0, None, None) == -errno.EINVAL
    assert T.xlating_tune_bank_state(None, 0, None, None, None, None) == -errno.EINVAL
    assert T.xlating_tune_bank_last_feed_ops(None, None, None) == -errno.EINVAL
    assert T.xlating_tune_from_hz(1.0, 0.0, 48000.0, None, None) == -errno.EINVAL
    T.xlating_tune_bank_destroy(None)
    assert V.xlating_serve_set_tune(None, 0, 0.0, 0.0) == -errno.EINVAL
    assert V.xlating_serve_tune_log(None, 0, 0, None, None, None) == -errno.EINVAL


def test_kernel_code_object(tmp_path):
    """compiled with the Makefile's flags, the gfx950 code of xl_tune.hip holds no packed FP32 arithmetic, no fused multiply-add, no
    matrix instruction, no LDS and no scratch access, and moves its samples through global (not flat) accesses"""
    mk = open(os.path.join(CSRC, "Makefile")).read()
    m = re.search(r"^TUNE_FLAGS\s*:=\s*(.+)$", mk, re.M)
    assert m and "-fno-slp-vectorize" in m.group(1)
    assert re.search(r"^\$\(BUILD\)/xl_tune_dev\.o: HIPFLAGS \+= \$\(TUNE_FLAGS\)$", mk, re.M)
    assert re.search(r"^\$\(BUILD\)/xl_tune_dev\.o: xl_tune\.hip", mk, re.M)
    assert re.search(r"^all:.*\$\(TUNE\)", mk, re.M)
    out = str(tmp_path / "k.s")
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fhip-fp32-correctly-rounded-divide-sqrt",
             "--cuda-device-only", "-S"]
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"  # (where build() looks for it)
    r = subprocess.run([hipcc] + flags + m.group(1).split() + [KERNEL, "-o", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    asm = open(out).read()
    assert "xl_tune_kernel" in asm
    ops = re.findall(r"^\s+([a-z][a-z0-9_]+)\s", asm, re.M)
    assert "v_mul_f32_e32" in ops and "global_load_dwordx2" in ops and "global_store_dwordx2" in ops
    assert not [o for o in ops if o.startswith(("v_pk_mul_f32", "v_pk_add_f32", "v_pk_fma_f32", "v_mfma", "v_smfma", "scratch_", "ds_", "flat_"))]
    assert not [o for o in ops if o.startswith(("v_fma_f32", "v_fmac_f32", "v_mad_f32", "v_mac_f32", "v_sin_", "v_cos_"))], "single, unfused operations"
    assert re.search(r"\.group_segment_fixed_size:\s*0\b", asm) and re.search(r"\.private_segment_fixed_size:\s*0\b", asm)
    assert re.search(r"\.vgpr_spill_count:\s*0\b", asm) and re.search(r"\.sgpr_spill_count:\s*0\b", asm)
