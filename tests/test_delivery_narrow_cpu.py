"""CPU tests (-m "not gpu") of the narrowing delivery (xlating_delivery_pack_device_cs16) and of the serve family built on it
(XL_SERVE_CF32_AS_CS16): the conversion rule's header is plain C and agrees with its libm restatement on all 2^32 bit patterns, part of
them under ASan and UBSan; the numpy restatement the GPU tests compare with is pinned to a table of exact cases; the narrowed layout
passes its sweep against brute force under the sanitizers; layout and rule have one home each; the kernel's code object holds no
floating-point instruction, no flat, LDS or scratch access; the refusals that need no device; and the scale is the Q15 family's."""
import ctypes as C
import errno
import os
import re
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import delivery_narrow_ref as NR
import sdr_server_amd as xl
from conftest import ROOT
from pyoracle import Oracle

CSRC = os.path.join(ROOT, "sdr-server_amd", "csrc")
SWEEP_SRC = os.path.join(ROOT, "tests", "c", "delivery_narrow_sweep.c")
KERNEL = os.path.join(CSRC, "xl_delivery_narrow.hip")
SANITIZE = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def _strip(path):
    return re.sub(r"/\*.*?\*/", "", re.sub(r"//[^\n]*", "", open(path).read()), flags=re.S)


def _build_sweep(exe, flags):
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-pedantic"] + flags + ["-I", CSRC, SWEEP_SRC, "-o", exe, "-lm"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]


def test_rule_header_is_plain_c_in_integers(tmp_path):
    hdr = open(os.path.join(CSRC, "xl_dlv_narrow.h")).read()
    assert "#include <hip" not in hdr and "#include <math" not in hdr
    code = _strip(os.path.join(CSRC, "xl_dlv_narrow.h"))
    assert not re.search(r"\b(float|double)\b", code) and not re.search(r"\d\.\d|\df\b", code), "integer arithmetic only"
    src = tmp_path / "t.c"
    src.write_text('#include "xl_dlv_narrow.h"\nint main(void) { return xl_dlv_narrow(0x3f800000u) == 32767 ? 0 : 1; }\n')
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-pedantic", "-I", CSRC, str(src), "-o", str(tmp_path / "t")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert subprocess.run([str(tmp_path / "t")]).returncode == 0


def test_rule_sweep_over_all_bit_patterns(tmp_path):
    """every float32 bit pattern, split by exponent field over child processes; the fields where the rule does anything but answer 0 or
    saturate (96 .. 140: the shift, the tie, the clamp's edge and well beyond both) and the special ones (0, 1, 254, 255) under the
    sanitizers"""
    san, fast = str(tmp_path / "sweep_san"), str(tmp_path / "sweep")
    _build_sweep(san, SANITIZE)
    _build_sweep(fast, ["-O2"])
    jobs = [(san, 0, 1), (san, 254, 255)] + [(san, e, min(e + 4, 140)) for e in range(96, 141, 5)]
    jobs += [(fast, e, min(e + 7, 95)) for e in range(2, 96, 8)] + [(fast, e, min(e + 7, 253)) for e in range(141, 254, 8)]
    fields = sorted(e for _, a, b in jobs for e in range(a, b + 1))
    assert fields == list(range(256))
    assert {e for exe, a, b in jobs if exe == san for e in range(a, b + 1)} >= set(range(96, 141)) | {0, 1, 254, 255}

    def run(job):
        exe, a, b = job
        r = subprocess.run([exe, "rule", str(a), str(b)], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and r.stdout.startswith("ok ") and r.stderr == "", (job, r.stdout[-300:], r.stderr[-1000:])
        return int(r.stdout.split()[1])

    with ThreadPoolExecutor(max_workers=max(1, min(16, os.cpu_count() or 1))) as pool:
        assert sum(pool.map(run, jobs)) == 1 << 32


def test_restatement_is_pinned_to_exact_cases():
    vals, want = NR.exact_values(), NR.exact_expected()
    assert vals.size == want.size >= 36
    got = NR.narrow(vals)
    assert got.dtype == np.int16 and np.array_equal(got, want), [(hex(b), int(g), int(w)) for (b, w), g in zip(NR.EXACT, got) if g != w]
    # the table holds what it says it holds
    bits = vals.view(np.uint32)
    assert np.isnan(vals).sum() == 7 and {0x7F800001, 0xFF800001, 0x7FC00000, 0xFFC00000} <= set(bits.tolist())
    assert {0x00000001, 0x007FFFFF, 0x7F7FFFFF, 0x7F800000, 0xFF800000, 0x80000000} <= set(bits.tolist())
    half = np.float32(2.0 ** -16)
    assert {float(np.nextafter(half, np.float32(1))), float(np.nextafter(half, np.float32(0))), float(half), float(-half)} <= set(vals[~np.isnan(vals)].tolist())
    # complex rows are read as their float pairs
    z = np.array([1.5 * NR.LSB - 2.5j * NR.LSB, -1.0 + 1.0j], np.complex64)
    assert NR.narrow(z).tolist() == [2, -2, -32768, 32767] and NR.narrow_bytes(z) == np.array([2, -2, -32768, 32767], np.int16).tobytes()


def test_layout_sweep_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "delivery_narrow_sweep")
    _build_sweep(exe, SANITIZE)
    r = subprocess.run([exe, "layout"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("ok ") and r.stderr == "", (r.stdout[-500:], r.stderr[-2000:])
    assert int(r.stdout.split()[1]) >= 10000


def test_layout_and_rule_have_one_home():
    """the narrowed offsets and source addresses come from xl_delivery_plan.h and the arithmetic from xl_dlv_narrow.h alone: the host
    calls the plan's functions, the kernel the search helpers, the source-address helper and the rule's function, and neither places a
    row, halves an offset or touches a float's fields itself"""
    host, dev = _strip(os.path.join(CSRC, "xl_delivery.cpp")), _strip(KERNEL)
    for name in ("xl_dlv_plan_narrow(", "xl_dlv_plan(", "xl_dlv_chunks(", "xl_dlv_narrow_launch"):
        assert name in host, name
    for name in ("xl_ragged_find(", "xl_dlv_first(", "xl_dlv_span(", "xl_dlv_narrow_src(", "xl_dlv_narrow("):
        assert name in dev, name
    for text in (host, dev):
        assert "xl_dlv_place" not in text
        assert not re.search(r"[&%]\s*\(?\s*(31|7|0x1f|0x7)u?\b", text, re.I), "alignment arithmetic outside the layout's header"
        assert not re.search(r"\b(r\.|r->|\.)src\s*[+-]", text), "a source address computed outside the layout's header"
    assert not re.search(r">>\s*23|0x7f+u?\b|0x80+u?\b|32768|32767|\bfloat\b", dev, re.I), "the rule restated in the kernel"
    plan = _strip(os.path.join(CSRC, "xl_delivery_plan.h"))
    assert "#include <hip" not in plan and "xl_dlv_place_narrow(" in plan and "xl_dlv_narrow_src(" in plan
    serve = _strip(os.path.join(CSRC, "xl_serve.cpp"))
    assert "xlating_delivery_pack_device_cs16(" in serve and "xl_dlv_" not in serve and "_fetch" not in serve


def test_narrow_kernel_code_object(tmp_path):
    """compiled with the Makefile's flags, the gfx950 code of xl_delivery_narrow.hip loads and stores 16 bytes at a time through global
    (not flat) accesses, uses no LDS and no scratch, and holds no floating-point, packed or matrix instruction"""
    mk = open(os.path.join(CSRC, "Makefile")).read()
    m = re.search(r"^DELIVERY_FLAGS\s*:=\s*(.+)$", mk, re.M)
    assert m and "-fno-slp-vectorize" in m.group(1)
    assert re.search(r"^\$\(BUILD\)/xl_delivery_narrow_dev\.o: HIPFLAGS \+= \$\(DELIVERY_FLAGS\)$", mk, re.M)
    assert re.search(r"^\$\(BUILD\)/xl_delivery_narrow_dev\.o: xl_delivery_narrow\.hip .*xl_dlv_narrow\.h", mk, re.M)
    assert re.search(r"^SERVE_OBJS\s*:=.*\$\(BUILD\)/xl_delivery_narrow_dev\.o", mk, re.M)
    assert not re.search(r"^OBJS\s*:=.*delivery", mk, re.M)  # (the engine's library is built as before)
    src = _strip(KERNEL)
    assert "asm" not in src and "__shared__" not in src
    out = str(tmp_path / "k.s")
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fhip-fp32-correctly-rounded-divide-sqrt",
             "--cuda-device-only", "-S"]
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"  # (where build() looks for it)
    r = subprocess.run([hipcc] + flags + m.group(1).split() + [KERNEL, "-o", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    asm = open(out).read()
    assert "xl_dlv_narrow_kernel" in asm
    ops = re.findall(r"^\s+([a-z][a-z0-9_]+)\s", asm, re.M)
    assert "global_load_dwordx4" in ops and "global_store_dwordx4" in ops
    assert not [o for o in ops if o.startswith(("flat_", "ds_", "scratch_", "v_pk_", "v_mfma", "v_smfma"))]
    assert not [o for o in ops if re.search(r"_(f16|bf16|f32|f64)(_|$)", o)], "a floating-point instruction"
    assert re.search(r"\.group_segment_fixed_size:\s*0\b", asm) and re.search(r"\.private_segment_fixed_size:\s*0\b", asm)


def test_symbol_family_and_refusals_need_no_device(tmp_path):
    V = xl.serve_lib()
    assert "xlating_delivery_pack_device_cs16" in xl.DELIVERY_SYMBOLS and hasattr(V, "xlating_delivery_pack_device_cs16")
    assert xl.SERVE_FAMILY == {"cf32": 0, "cs16": 1, "cf32-cs16": 2}
    one = (C.c_uint64 * 1)(8)
    key = (C.c_int * 1)(0)
    assert V.xlating_delivery_pack_device_cs16(None, 1, key, one, one, None) == -errno.EINVAL
    assert V.xlating_delivery_pack_device_cs16(None, 0, None, None, None, None) == -errno.EINVAL
    # (a source at 8k + 4 and a row above the maximum are the plan's refusals, -EINVAL of the call: tests/c/delivery_narrow_sweep.c
    # holds xl_dlv_plan_narrow to them, and test_delivery_narrow_gpu.py the call)
    h = C.c_void_p()
    cfg = xl.ServeConfig(192000, xl.FMT["cf32"], 65536, 1, -1, xl.SERVE_FAMILY["cf32-cs16"], 0, 1, 5, None, 0, 2, 0, 2, 0)
    assert V.xlating_serve_create(C.byref(cfg), C.byref(h)) == -errno.EINVAL and not h.value  # (no base path)
    for family in (3, 7, -1):
        cfg = xl.ServeConfig(192000, xl.FMT["cu8"], 65536, 1, -1, family, 0, 1, 5, str(tmp_path).encode(), 0, 2, 0, 2, 0)
        assert V.xlating_serve_create(C.byref(cfg), C.byref(h)) == -errno.EINVAL and not h.value  # (no such family)
    assert C.sizeof(xl.ServeConfig) == 72  # (the struct is the one it was: no field was added)


def test_scale_is_the_q15_familys():
    """the same cs16 noise block through the oracle's Q15 family and through its native cf32 family narrowed by the restatement, D = 42
    with the server's 505 taps: the least-squares gain between the two streams lies within 1 +- 2^-7 -- what a wrong power of two
    would miss; no claim on precision (the Q15 family truncates in four places), the largest difference is printed.
    The block is the first 128 outputs of a stream: the Q15 family's phasor is a truncating recurrence that is never renormalised
    (xlating.c:126-129) and loses up to an LSB of its 32767 with every output, about 3e-5 of the stream's gain per output -- 2^-7 after
    some 500 outputs, 6 % over one 262144-byte block.  That is the Q15 family's arithmetic, which the narrowed stream does not share, and
    not its scale; over 128 outputs it amounts to 0.2 % on average."""
    code, taps = xl.create_low_pass_filter(1.0, 2016000, 24000, 9600)
    assert code == 0 and taps.size == 505
    rng = np.random.default_rng(11)
    x = np.clip(np.rint(6000.0 * rng.standard_normal(2 * 42 * 128)), -32768, 32767).astype(np.int16)
    got = []
    for out in ("cs16", "cf32"):
        o = Oracle(42, taps, 100000, 2016000, x.size)
        got.append(o.process("cs16", x, out))
        o.close()
    q15 = got[0].reshape(-1).astype(np.float64)
    nar = NR.narrow(got[1]).reshape(-1).astype(np.float64)
    assert q15.size == nar.size == 256 and np.abs(q15).max() < 32767 and np.sqrt(np.mean(q15 ** 2)) > 100
    gain = float(np.dot(q15, nar) / np.dot(q15, q15))
    worst = float(np.abs(q15 - nar).max())
    print(f"narrowed cf32 against Q15, D = 42, 505 taps, {q15.size // 2} samples: gain {gain:.6f}, largest difference {worst:.0f} LSB, "
          f"rms {np.sqrt(np.mean((q15 - nar) ** 2)):.2f} LSB of a stream of rms {np.sqrt(np.mean(q15 ** 2)):.0f}")
    assert abs(gain - 1.0) <= 2.0 ** -7, gain
