"""CPU tests (-m "not gpu") of the power meter (include/xlating_meter.h) and of the squelch of the serve object: the rule header is
plain C with one include; the exported symbols are the headers' declarations; the refusals that need no device; the kernels' code
object (scalar FP32 only, nothing fused, no matrix instruction, no scratch, global loads, subnormals kept); the squelch policy and its
log against a second statement, as a program of its own under ASan and UBSan; the restatement (tests/meter_ref.py) against float64
within the derived bound on the rows the GPU test measures."""
import ctypes as C
import errno
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import meter_cases as MC
import meter_ref as MR
import sdr_server_amd as xl
from conftest import ROOT

CSRC = os.path.join(ROOT, "sdr-server_amd", "csrc")
RULE = os.path.join(CSRC, "xl_meter_rule.h")
POLICY = os.path.join(CSRC, "xl_serve_squelch.h")
KERNEL = os.path.join(CSRC, "xl_meter.hip")
SWEEP_SRC = os.path.join(ROOT, "tests", "c", "squelch_policy_sweep.c")
SANITIZE = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def _strip(path):
    return re.sub(r"/\*.*?\*/", "", re.sub(r"//[^\n]*", "", open(path).read()), flags=re.S)


def test_rule_and_policy_headers_are_plain_c(tmp_path):
    for path in (RULE, POLICY):
        code = _strip(path)
        assert re.findall(r"#include\s*(\S+)", code) == ["<stdint.h>"], path
        assert "#include <hip" not in code and "asm" not in code and "__builtin" not in code, path
    assert not re.search(r"\bfmaf?\s*\(", _strip(RULE))
    src = tmp_path / "t.c"
    src.write_text('#include "xl_meter_rule.h"\n#include "xl_serve_squelch.h"\n'
                   "int main(void) {\n"
                   "  uint64_t p[2] = {0x3F800000u, 0x40400000u}, q[2] = {3u << 30, 1u << 30};\n"
                   "  XlServeSquelch s;\n"
                   "  xl_serve_squelch_init(&s, 2.0, 1.0, 0u);\n"
                   "  return xl_meter_mean_cf32(p, 2u, 4u) == 1.0 && xl_meter_mean_cs16(q, 2u, 2u) == 2.0 && xl_meter_pieces(2049u) == 2u &&\n"
                   "         xl_meter_p_cs16(0x80008000u) == 0x80000000u && xl_meter_p_cf32(3.0f, 4.0f) == 25.0f &&\n"
                   "         xl_serve_squelch_step(&s, 1.5) == 0 && xl_serve_squelch_step(&s, 2.0) == 1 ? 0 : 1;\n"
                   "}\n")
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-pedantic", "-ffp-contract=off", "-I", CSRC, str(src), "-o", str(tmp_path / "t")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert subprocess.run([str(tmp_path / "t")]).returncode == 0
    assert f"#define XL_METER_PIECE (XL_METER_THREADS * XL_METER_PER_THREAD)" in open(RULE).read()
    assert (MR.PIECE, MR.THREADS, MR.PER_THREAD, MR.LOG) == (2048, 256, 8, 64)


def test_policy_sweep_under_the_sanitizers(tmp_path):
    """every sequence of up to 8 calls over {below close, between, above open, NaN}, hang 0 .. 3, marks apart and equal, against a
    statement that steps no state; the log with calls of no samples; the ring at 64, 65 and 200 changes"""
    exe = str(tmp_path / "sweep")
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-pedantic", "-ffp-contract=off"] + SANITIZE + ["-I", CSRC, SWEEP_SRC, "-o", exe, "-lm"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.match(r"sequences (\d+) log_checks (\d+)", r.stdout)
    assert m and int(m.group(1)) == 2 * 4 * sum(4 ** n for n in range(1, 9)) and int(m.group(2)) > int(m.group(1))


def test_python_policy_is_the_header_s(tmp_path):
    """tests/meter_ref.py's policy and log (what the GPU scenario is held to) against the header's, call by call, on random sequences"""
    src = tmp_path / "p.c"
    src.write_text('#include <stdio.h>\n#include <stdlib.h>\n#include <string.h>\n#include "xl_serve_squelch.h"\n'
                   "int main(int argc, char **argv) {\n"
                   "  XlServeSquelch q; XlServeSquelchLog l; memset(&l, 0, sizeof l);\n"
                   "  xl_serve_squelch_init(&q, atof(argv[1]), atof(argv[2]), (uint32_t)atoi(argv[3]));\n"
                   "  uint64_t pr = 0, de = 0;\n"
                   "  for (int i = 4; i + 1 < argc; i += 2) {\n"
                   "    const int g = xl_serve_squelch_step(&q, atof(argv[i])); const uint64_t n = (uint64_t)atoll(argv[i + 1]);\n"
                   "    xl_serve_squelch_log_note(&l, pr, de, g); pr += n; if (g) de += n; printf(\"%d\", g);\n"
                   "  }\n"
                   "  uint64_t a[64], b[64]; uint8_t o[64];\n"
                   "  const uint32_t n = xl_serve_squelch_log_read(&l, 64u, a, b, o);\n"
                   "  for (uint32_t i = 0; i < n; ++i) printf(\" %llu,%llu,%u\", (unsigned long long)a[i], (unsigned long long)b[i], (unsigned)o[i]);\n"
                   "  printf(\"\\n\"); return 0;\n"
                   "}\n")
    exe = str(tmp_path / "p")
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    rng = np.random.default_rng(7)
    for trial in range(12):
        hang = trial % 4
        op, cl = (1e-3, 1e-3) if trial % 3 == 0 else (1e-3, 2.5e-4)
        calls = 300 if trial >= 10 else 40  # (the long ones pass the ring's 64 entries)
        P = [[cl / 2, (op + cl) / 2, 2 * op, float("nan")][int(v)] for v in rng.integers(0, 4, calls)]
        lens = [int(v) for v in rng.integers(0, 3, calls) * 1000]
        args = [repr(op), repr(cl), str(hang)] + [t for p, n in zip(P, lens) for t in (repr(p), str(n))]
        out = subprocess.run([exe] + args, capture_output=True, text=True).stdout.split()
        gates, log, withheld = MR.run_policy(P, lens, op, cl, hang)
        assert out[0] == "".join("1" if g else "0" for g in gates), trial
        assert [tuple(int(v) for v in e.split(",")) for e in out[1:]] == log, trial
        assert withheld == sum(n for g, n in zip(gates, lens) if not g)


def test_symbols_are_exported():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "xlating_meter.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(xlating_meter_[a-z_0-9]+)\s*\(", hdr))
    assert declared == set(xl.METER_SYMBOLS), declared ^ set(xl.METER_SYMBOLS)
    out = subprocess.run(["nm", "-D", "--defined-only", xl.meter_library_path()], capture_output=True, text=True).stdout
    defined = {l.split()[-1] for l in out.splitlines() if l.strip()}
    assert set(xl.METER_SYMBOLS) <= defined, set(xl.METER_SYMBOLS) - defined
    M, V = xl.meter_lib(), xl.serve_lib()
    for name in xl.METER_SYMBOLS:
        assert hasattr(M, name), name
    shdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "xlating_serve.h")).read(), flags=re.S)
    sdecl = set(re.findall(r"\b(xlating_serve_[a-z_0-9]+)\s*\(", shdr))
    assert sdecl == set(xl.SERVE_SYMBOLS), sdecl ^ set(xl.SERVE_SYMBOLS)
    for name in ("xlating_serve_set_squelch", "xlating_serve_clear_squelch", "xlating_serve_squelch_state", "xlating_serve_squelch_log"):
        assert name in xl.SERVE_SYMBOLS and hasattr(V, name), name
    needed = subprocess.run(["readelf", "-d", xl.serve_library_path()], capture_output=True, text=True).stdout
    assert "libxlating_meter.so" in needed
    assert xl.meter_piece_samples() == MR.PIECE
    # every library's handle is its own, whatever was loaded first
    assert xl.multi_lib() is not M and M._name == xl.meter_library_path() and V._name == xl.serve_library_path()
    # the C ABI includes no HIP header
    assert not [i for i in re.findall(r"#include\s*(\S+)", hdr) if "hip" in i]


def test_refusals_need_no_device():
    M, V = xl.meter_lib(), xl.serve_lib()
    assert M.xlating_meter_create(None) == -errno.EINVAL
    one = (C.c_uint64 * 1)(0)
    assert M.xlating_meter_measure_device(None, 0, 1, one, one, None) == -errno.EINVAL
    assert M.xlating_meter_query(None) == -errno.EINVAL and M.xlating_meter_wait(None) == -errno.EINVAL
    assert M.xlating_meter_power(None, 0, None, None) == -errno.EINVAL
    assert M.xlating_meter_partials(None, 0, 0, None) == -errno.EINVAL
    assert M.xlating_meter_last_ops(None, None, None) == -errno.EINVAL
    M.xlating_meter_destroy(None)
    assert V.xlating_serve_set_squelch(None, 0, 1.0, 0.5, 0) == -errno.EINVAL
    assert V.xlating_serve_clear_squelch(None, 0) == -errno.EINVAL
    assert V.xlating_serve_squelch_state(None, 0, None, None, None, None) == -errno.EINVAL
    assert V.xlating_serve_squelch_log(None, 0, 0, None, None, None) == -errno.EINVAL


def test_kernel_code_object(tmp_path):
    """compiled with the Makefile's flags, the gfx950 code of xl_meter.hip holds no packed FP32 arithmetic, no fused multiply-add, no
    matrix instruction and no scratch access, reads its rows through global (not flat) loads, and keeps float32 subnormals"""
    mk = open(os.path.join(CSRC, "Makefile")).read()
    m = re.search(r"^METER_FLAGS\s*:=\s*(.+)$", mk, re.M)
    assert m and "-fno-slp-vectorize" in m.group(1)
    assert re.search(r"^\$\(BUILD\)/xl_meter_dev\.o: HIPFLAGS \+= \$\(METER_FLAGS\)$", mk, re.M)
    assert re.search(r"^\$\(BUILD\)/xl_meter_dev\.o: xl_meter\.hip", mk, re.M)
    assert re.search(r"^all:.*\$\(METER\)", mk, re.M)
    assert "-ffp-contract=off" in re.search(r"^HIPFLAGS\s*:=\s*(.+)$", mk, re.M).group(1)
    assert not re.search(r"-f[a-z-]*denormal|-m[a-z-]*daz|ftz", mk, re.I), "no flush flag: the rule keeps float32 subnormals"
    out = str(tmp_path / "k.s")
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fhip-fp32-correctly-rounded-divide-sqrt",
             "--cuda-device-only", "-S"]
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"  # (where build() looks for it)
    r = subprocess.run([hipcc] + flags + m.group(1).split() + [KERNEL, "-o", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    asm = open(out).read()
    assert "xl_meter_cf32_kernel" in asm and "xl_meter_cs16_kernel" in asm
    ops = re.findall(r"^\s+([a-z][a-z0-9_]+)\s", asm, re.M)
    assert ops.count("v_mul_f32_e32") == 16 and "v_add_f32_e32" in ops, "two single squares a sample, eight samples a thread"
    assert "global_load_dwordx2" in ops and "global_load_dword" in ops and "global_store_dwordx2" in ops
    assert not [o for o in ops if o.startswith(("v_pk_mul_f32", "v_pk_add_f32", "v_pk_fma_f32", "v_mfma", "v_smfma", "scratch_", "flat_"))]
    assert not [o for o in ops if o.startswith(("v_fma_f32", "v_fmac_f32", "v_mad_f32", "v_mac_f32", "v_fma_mix", "v_pk_fma"))], "single, unfused operations"
    assert len(re.findall(r"\.private_segment_fixed_size:\s*0\b", asm)) == 2
    assert len(re.findall(r"\.vgpr_spill_count:\s*0\b", asm)) == 2 and len(re.findall(r"\.sgpr_spill_count:\s*0\b", asm)) == 2
    assert sorted(int(v) for v in re.findall(r"\.group_segment_fixed_size:\s*(\d+)", asm)) == [16, 32], "the four wave sums"
    assert re.findall(r"\.amdhsa_float_denorm_mode_32\s+(\d+)", asm) == ["3", "3"], "float32 subnormals are kept"


def test_restatement_within_the_bound():
    """the rows of the GPU test: the float32 order against float64, within gamma_17 and the double sum's share"""
    worst = 0.0
    for name, x, kind in MC.cf32_rows():
        parts = MR.partials_cf32(x)
        assert parts.size == -(-x.size // MR.PIECE) and not np.any(parts >> np.uint64(32)), name
        p = MR.mean_cf32(parts, x.size)
        if kind == "zero":
            assert p == 0.0 and math.copysign(1.0, p) == 1.0 and not np.any(parts), name
        elif kind == "nonfinite":
            assert not math.isfinite(p), name
            fin = [math.isfinite(float(v)) for v in parts.astype(np.uint32).view(np.float32)]
            if not name.startswith("overflow"):  # the one bad sample is alone in the last piece
                assert fin == [True] * (len(fin) - 1) + [False], name
        elif kind == "subnormal":
            sq = (x.real.astype(np.float32) ** 2).astype(np.float32)
            assert np.all(sq < 2.0 ** -126) and np.any(sq > 0), "the squares are subnormal, and some survive"
            e = MR.exact_power_cf32(x)
            assert p > 0.0 and abs(p - e) <= MR.bound(parts.size) * e + 17 * 2.0 ** -149, name  # (absolute: an ulp of the subnormals per level)
        else:
            e = MR.exact_power_cf32(x)
            assert e > 0.0
            if kind == "maybe" and not math.isfinite(p):  # an overflow is one only where the exact sum is at the range's end
                assert e * min(x.size, MR.PIECE) > 2.0 ** 127, name
                continue
            rel = abs(p - e) / e
            worst = max(worst, rel)
            assert rel <= MR.bound(parts.size), (name, rel / MR.U)
    print(f"worst relative error {worst / MR.U:.3f} u against the bound {MR.GAMMA17 / MR.U:.3f} u")
    assert 0.0 < worst
    for name, x, want in MC.cs16_rows():
        n = x.shape[0]
        p = MR.power_cs16(x)
        exact = float(np.sum(x.astype(np.float64) ** 2)) / n / 2.0 ** 30 if n else 0.0  # (exact in double: below 2^53)
        assert p == exact and (want is None or p == want), name
