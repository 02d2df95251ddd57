"""CPU tests (-m "not gpu") of the delivery's gain and level meter (xlating_delivery_pack_device_cs16_gain, xlating_delivery_row_level)
and of the serve calls built on them (xlating_serve_set_gain, _set_auto_gain, _enable_levels, _levels, _gain_log): the rule's header is
plain C in integers, equals xl_dlv_narrow.h at gain 0 on all 2^32 bit patterns and its libm statement, clamp flag included, on all 2^32
patterns at the gains -48, -1, 1 and 48 and on the edge fractions of every exponent field at every gain, part of it under ASan and
UBSan; the numpy restatement is pinned to exact cases; the plan function and the gain policy pass their sweeps under the sanitizers;
layout, rule and policy have one home each; the kernel's code object meets the narrow kernel's criteria; the refusals that need no
device."""
import ctypes as C
import errno
import os
import re
import shutil
import subprocess
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import delivery_gain_ref as GR
import delivery_narrow_ref as NR
import sdr_server_amd as xl
from conftest import ROOT

CSRC = os.path.join(ROOT, "sdr-server_amd", "csrc")
SWEEP_SRC = os.path.join(ROOT, "tests", "c", "delivery_gain_sweep.c")
KERNEL = os.path.join(CSRC, "xl_delivery_gain.hip")
SANITIZE = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
FULL_GAINS = (-48, -1, 1, 48)


def _strip(path):
    return re.sub(r"/\*.*?\*/", "", re.sub(r"//[^\n]*", "", open(path).read()), flags=re.S)


def _build_sweep(exe, flags):
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-pedantic"] + flags + ["-I", CSRC, SWEEP_SRC, "-o", exe, "-lm"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]


def _run(exe, *args, timeout=600):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0 and r.stdout.startswith("ok ") and r.stderr == "", (args, r.stdout[-300:], r.stderr[-2000:])
    return int(r.stdout.split()[1])


def test_rule_and_policy_headers_are_plain_c_in_integers(tmp_path):
    for name, call in (("xl_dlv_gain.h", "uint32_t c; return xl_dlv_gain_narrow(0x3f800000u, -1, &c) == 16384 && c == 0u ? 0 : 1;"),
                       ("xl_serve_gain.h", "XlServeGainState s = {0}; return xl_serve_gain_step(&s, 0x40000000u, 1u, 0, 0) == -2 ? 0 : 1;")):
        hdr = open(os.path.join(CSRC, name)).read()
        assert "#include <hip" not in hdr and "#include <math" not in hdr
        code = _strip(os.path.join(CSRC, name))
        assert not re.search(r"\b(float|double)\b", code) and not re.search(r"\d\.\d|\df\b", code), "integer arithmetic only"
        src = tmp_path / (name + ".c")
        src.write_text('#include "%s"\nint main(void) { %s }\n' % (name, call))
        exe = str(tmp_path / (name + ".exe"))
        r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-pedantic", "-I", CSRC, str(src), "-o", exe], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        assert subprocess.run([exe]).returncode == 0
    assert "#include <hip" not in open(os.path.join(CSRC, "xl_delivery_plan.h")).read()


def test_rule_sweep_over_all_bit_patterns(tmp_path):
    """gain 0 against xl_dlv_narrow (integers), and the gains -48, -1, 1, 48 against libm with the clamp flag: every float32 bit
    pattern each, split by exponent field over child processes.  Under the sanitizers: the fields where the rule does more than answer 0
    or saturate (e + g in 111 .. 127; taken as 108 .. 130) and the fields 0, 1, 254 and 255.  Then every other gain on the edge
    fractions of every field (the sweep's `edges`), under the sanitizers."""
    san, fast = str(tmp_path / "sweep_san"), str(tmp_path / "sweep")
    _build_sweep(san, SANITIZE)
    _build_sweep(fast, ["-O2"])
    t0 = time.time()
    jobs = []
    for g in (None,) + FULL_GAINS:  # None: the compare with xl_dlv_narrow at gain 0
        lo, hi = 108 - (g or 0), 130 - (g or 0)
        mode = ("zero",) if g is None else ("rule", g)
        mine = [(san,) + mode + (0, 1), (san,) + mode + (254, 255)] + [(san,) + mode + (e, min(e + 3, hi)) for e in range(lo, hi + 1, 4)]
        mine += [(fast,) + mode + (e, min(e + 15, lo - 1)) for e in range(2, lo, 16)]
        mine += [(fast,) + mode + (e, min(e + 15, 253)) for e in range(hi + 1, 254, 16)]
        fields = sorted(e for j in mine for e in range(j[-2], j[-1] + 1))
        assert fields == list(range(256)), (g, fields)
        assert {e for j in mine if j[0] == san for e in range(j[-2], j[-1] + 1)} == set(range(lo, hi + 1)) | {0, 1, 254, 255}
        jobs += mine
    with ThreadPoolExecutor(max_workers=max(1, min(16, os.cpu_count() or 1))) as pool:
        assert sum(pool.map(lambda j: _run(*j), jobs)) == (1 + len(FULL_GAINS)) << 32
    assert _run(san, "edges") == 97 * 256 * 2 * 11
    print(f"rule sweep: {(1 + len(FULL_GAINS))} x 2^32 patterns and the edges in {time.time() - t0:.1f} s")


def test_restatement_is_pinned_to_exact_cases():
    """at gain 0 the existing table; at +-1, +-9, +-48 the same table with the inputs scaled by 2^-g where that is exact"""
    assert np.array_equal(GR.narrow(NR.exact_values()), NR.exact_expected()) and np.array_equal(GR.narrow(NR.exact_values(), 0), NR.narrow(NR.exact_values()))
    assert GR.exact_table(0) == NR.EXACT
    for g in GR.PINNED_GAINS:
        table = GR.exact_table(g)
        vals = np.array([b for b, _ in table], np.uint32).view(np.float32)
        want = np.array([w for _, w in table], np.int16)
        scaled = sum(1 for b, _ in table if (b >> 23) & 0xFF not in (0, 0xFF))
        assert scaled >= 15 and np.isnan(vals).sum() == 7, (g, scaled)
        got = GR.narrow(vals, g)
        assert got.dtype == np.int16 and np.array_equal(got, want), (g, [(hex(b), int(x), int(w)) for (b, w), x in zip(table, got) if x != w])
        # the scaled inputs are the table's times 2^-g, exactly
        f32 = lambda b: float(np.array([b], np.uint32).view(np.float32)[0])
        moved = [(b0, w0) for b0, w0 in NR.EXACT if (b0 >> 23) & 0xFF not in (0, 0xFF) and 1 <= ((b0 >> 23) & 0xFF) - g <= 254]
        assert len(moved) == scaled
        for b0, w0 in moved:
            b = b0 - (g << 23)
            assert (b, w0) in table and f32(b) == f32(b0) * 2.0 ** -g, (g, hex(b0))
    # the levels, in integers
    z = np.array([0x3F800000, 0xBF800000, 0x7FC00000, 0xFF800000, 0x00000001, 0x80000000, 0x3F7FFFFF, 0xBF800001], np.uint32).view(np.float32)
    assert GR.level(z, 0) == (0x7F800000, 3, 1)  # +1.0, -Inf and 0.99999994 (rounds to 32768) clip; -1.0 and -1.0000001 (rounds to -32768) do not
    assert GR.level(z, -1) == (0x7F800000, 1, 1) and GR.level(z[:3], -1) == (0x3F800000, 0, 1)
    assert GR.level(z[2:3]) == (0, 0, 1) and GR.level(z[:0]) == (0, 0, 0) and GR.level(z[4:5], 48) == (1, 0, 0)
    assert GR.narrow(z[:2], -1).tolist() == [16384, -16384] and GR.undo([16384, -3], -1).tolist() == [1.0, -3 * 2.0 ** -14]


def test_plan_and_policy_sweeps_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "delivery_gain_sweep")
    _build_sweep(exe, SANITIZE)
    assert _run(exe, "plan", timeout=300) >= 3000
    assert _run(exe, "policy", timeout=300) >= 1000000


def test_layout_rule_and_policy_have_one_home():
    """the discipline test_layout_and_rule_have_one_home states for the existing pair, for the new files: the host calls the plan's
    function and the launch, the kernel the search helpers, the source-address helper and the rule's functions; neither places a row or
    touches a float's fields; the serve object calls the delivery's public functions and the policy header"""
    host, dev = _strip(os.path.join(CSRC, "xl_delivery.cpp")), _strip(KERNEL)
    for name in ("xl_dlv_plan_gain(", "xl_dlv_gain_launch(", "xl_dlv_chunks("):
        assert name in host, name
    for name in ("xl_ragged_find(", "xl_dlv_gain_first(", "xl_dlv_span(", "xl_dlv_narrow_src(", "xl_dlv_gain_narrow(", "xl_dlv_gain_mag(", "xl_dlv_gain_nan("):
        assert name in dev, name
    for text in (host, dev):
        assert "xl_dlv_place" not in text
        assert not re.search(r"[&%]\s*\(?\s*(31|7|0x1f|0x7)u?\b", text, re.I), "alignment arithmetic outside the layout's header"
        assert not re.search(r"\b(r\.|r->|\.)src\s*[+-]", text), "a source address computed outside the layout's header"
    assert not re.search(r">>\s*23|0x7f+u?\b|0x80+u?\b|32768|32767|\bfloat\b", dev, re.I), "the rule restated in the kernel"
    assert "xl_dlv_gain_narrow" not in host and not re.search(r">>\s*23|0x7f8|32768|32767|\bfloat\b", host, re.I)
    plan = _strip(os.path.join(CSRC, "xl_delivery_plan.h"))
    assert "XlDlvGainRun" in plan and "xl_dlv_plan_gain(" in plan
    serve = _strip(os.path.join(CSRC, "xl_serve.cpp"))
    for name in ("xlating_delivery_pack_device_cs16_gain(", "xlating_delivery_row_level(", "xl_serve_gain_step(", "xl_serve_gain_log_add("):
        assert name in serve, name
    assert "xl_dlv_" not in serve and "_fetch" not in serve and not re.search(r">>\s*23|0x7f8", serve, re.I)
    hdr = _strip(os.path.join(CSRC, "xl_serve_gain.h"))
    assert re.search(r"#define XL_SERVE_GAIN_QUIET_CALLS 8\b", hdr) and re.search(r"#define XL_SERVE_GAIN_LOW_TOP \(-3\)", hdr)


def test_gain_kernel_code_object(tmp_path):
    """the existing narrow kernel's criteria: compiled with the Makefile's flags, the gfx950 code of xl_delivery_gain.hip loads and
    stores 16 bytes at a time through global (not flat) accesses, uses no LDS and no scratch, and holds no floating-point, packed or
    matrix instruction"""
    mk = open(os.path.join(CSRC, "Makefile")).read()
    m = re.search(r"^DELIVERY_FLAGS\s*:=\s*(.+)$", mk, re.M)
    assert m and "-fno-slp-vectorize" in m.group(1)
    assert re.search(r"^\$\(BUILD\)/xl_delivery_gain_dev\.o: HIPFLAGS \+= \$\(DELIVERY_FLAGS\)$", mk, re.M)
    assert re.search(r"^\$\(BUILD\)/xl_delivery_gain_dev\.o: xl_delivery_gain\.hip .*xl_dlv_gain\.h", mk, re.M)
    assert re.search(r"^SERVE_OBJS\s*:=.*\$\(BUILD\)/xl_delivery_gain_dev\.o", mk, re.M)
    assert not re.search(r"^OBJS\s*:=.*delivery", mk, re.M)
    src = _strip(KERNEL)
    assert "asm" not in src and "__shared__" not in src
    out = str(tmp_path / "k.s")
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fhip-fp32-correctly-rounded-divide-sqrt",
             "--cuda-device-only", "-S"]
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"  # (where build() looks for it)
    r = subprocess.run([hipcc] + flags + m.group(1).split() + [KERNEL, "-o", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    asm = open(out).read()
    assert "xl_dlv_gain_kernel" in asm
    ops = re.findall(r"^\s+([a-z][a-z0-9_]+)\s", asm, re.M)
    assert "global_load_dwordx4" in ops and "global_store_dwordx4" in ops
    assert not [o for o in ops if o.startswith(("flat_", "ds_", "scratch_", "v_pk_", "v_mfma", "v_smfma"))]
    assert not [o for o in ops if re.search(r"_(f16|bf16|f32|f64)(_|$)", o)], "a floating-point instruction"
    assert re.search(r"\.group_segment_fixed_size:\s*0\b", asm) and re.search(r"\.private_segment_fixed_size:\s*0\b", asm)
    # the level table is reached by global atomics that return nothing
    atomics = {o for o in ops if "atomic" in o}
    assert atomics == {"global_atomic_umax", "global_atomic_add"}, atomics


def test_symbols_and_refusals_need_no_device(tmp_path):
    V = xl.serve_lib()
    for name in ("xlating_delivery_pack_device_cs16_gain", "xlating_delivery_row_level"):
        assert name in xl.DELIVERY_SYMBOLS and hasattr(V, name), name
    for name in ("xlating_serve_set_gain", "xlating_serve_set_auto_gain", "xlating_serve_enable_levels", "xlating_serve_levels", "xlating_serve_gain_log"):
        assert name in xl.SERVE_SYMBOLS and hasattr(V, name), name
    for name in ("pack_device_cs16_gain", "row_level"):
        assert hasattr(xl.Delivery, name), name
    for name in ("set_gain", "enable_levels", "levels", "set_auto_gain", "gain_log"):
        assert hasattr(xl.Serve, name), name
    one = (C.c_uint64 * 1)(8)
    key = (C.c_int * 1)(0)
    for g in (0, 49, -49):
        gain = (C.c_int8 * 1)(g)
        assert V.xlating_delivery_pack_device_cs16_gain(None, 1, key, one, one, gain, None) == -errno.EINVAL  # (a null object)
    assert V.xlating_delivery_pack_device_cs16_gain(None, 0, None, None, None, None, None) == -errno.EINVAL
    a, b, c = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
    assert V.xlating_delivery_row_level(None, 0, 0, C.byref(a), C.byref(b), C.byref(c)) == -errno.EINVAL
    # (gains of 49 and -49 on a live object are the plan's refusals, -EINVAL of the call: tests/c/delivery_gain_sweep.c holds
    # xl_dlv_plan_gain to them, test_delivery_gain_gpu.py the call)
    assert V.xlating_serve_set_gain(None, 0, 0) == -errno.EINVAL and V.xlating_serve_set_auto_gain(None, 0, 1) == -errno.EINVAL
    assert V.xlating_serve_enable_levels(None, 1) == -errno.EINVAL and V.xlating_serve_gain_log(None, 0, 0, None, None) == -errno.EINVAL
    assert V.xlating_serve_levels(None, 0, None, None, None, None, None, None) == -errno.EINVAL
    assert xl.SERVE_FAMILY == {"cf32": 0, "cs16": 1, "cf32-cs16": 2} and C.sizeof(xl.ServeConfig) == 72
