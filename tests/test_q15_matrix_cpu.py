"""CPU tests (-m "not gpu") of the matrix-core Q15 FIR (engine option "q15_kernel"; csrc/q15mm/xl_q15_mm.hip): the host side against
int64 arithmetic in a stand-alone program under ASan and UBSan (tests/c/q15_digits_sweep.c over csrc/xl_q15_digits.h and the int64 entry
of xl_q15_narrow.h), the launch's host plan the same way (tests/c/q15mm_plan_sweep.cpp over xl_build_q15mm), which clients the launch
carries -- pinned from the library for every client of the GPU tests, so that a silent fallback to the float64 launch cannot pass
them --, and the kernel's code object."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import q15_extremes_cases as QC
import sdr_server_amd as xl
from conftest import ROOT

CSRC = os.path.join(ROOT, "sdr-server_amd", "csrc")
KERNEL = os.path.join(CSRC, "q15mm", "xl_q15_mm.hip")
HIPFLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fhip-fp32-correctly-rounded-divide-sqrt",
            "--cuda-device-only", "-S"]


def test_digits_sweep_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "q15_digits_sweep")
    r = subprocess.run(["gcc", "-std=c11", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                        os.path.join(ROOT, "tests", "c", "q15_digits_sweep.c"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("ok "), (r.stdout[-500:], r.stderr[-2000:])
    assert int(r.stdout.split()[1]) >= 1000000, r.stdout  # (the sweeps ran)


def test_matrix_plan_sweep_under_the_sanitizers(tmp_path):
    """xl_build_q15mm (csrc/xl_plan.cpp, linked alone as tests/test_plan_cpu.py links it): tiles, image, fallback counts"""
    cxx = shutil.which("g++") or "/opt/rocm/lib/llvm/bin/clang++"
    rocm_include = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")  # (hip_runtime.h's types only: nothing of HIP is linked)
    exe = str(tmp_path / "q15mm_plan_sweep")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                        "-I", rocm_include, "-D__HIP_PLATFORM_AMD__", os.path.join(ROOT, "tests", "c", "q15mm_plan_sweep.cpp"),
                        os.path.join(CSRC, "xl_plan.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("ok "), (r.stdout[-500:], r.stderr[-2000:])
    plans, checks = (int(v) for v in r.stdout.split()[1:3])
    assert plans == 180 and checks >= 50000, r.stdout


def _admits(shape, fc):
    return xl.q15_matrix_admits(QC.SHAPE_D[shape], QC.taps(shape), fc, QC.FS)


def test_which_clients_the_matrix_launch_carries():
    """every client of the GPU tests' populations and every (shape, fc) the churn can draw: edge7 -- taps of -1.0 and of the largest
    float32 below 1.0, Q15 -32768 and 32767 at fc = 0 and about 32759 at the small angles -- has no int8 digit pair and stays on the float64
    launch; everybody else rides the matrix launch (even16 reaches +-29491)"""
    listed = set(QC.SAT_CLIENTS) | set(QC.HEIGHT_CLIENTS) | set(QC.MIX_CLIENTS_BIG)
    listed |= {(s, fc) for s in QC.CHURN_SHAPES for fc in (QC.CHURN_FCS[:3] if s == "edge7" else QC.CHURN_FCS)}
    for seed, _ in QC.CHURN_RUNS:
        listed |= {(s, fc) for joins, _, _, _, _ in QC.churn_schedule(seed) for _, s, fc in joins}
    assert {s for s, _ in listed} == set(QC.CHURN_SHAPES)
    for shape, fc in sorted(listed):
        assert _admits(shape, fc) == (shape != "edge7"), (shape, fc)


def test_the_admission_edge():
    """a single tap at fc = 0 is its own Q15 value: 32639 = 127 * 256 + 127 is the largest entry with an int8 digit pair"""
    for q, want in ((32639, True), (32640, False), (-32768, True), (32767, False)):
        tap = np.array([q / 32768.0], np.float32)
        assert int(np.float32(tap[0]) * np.float32(32768.0)) == q
        assert xl.q15_matrix_admits(1, tap, 0, QC.FS) == want, q
    # not a shape of the launch at all: a wide client, no taps
    assert not xl.q15_matrix_admits(3000, QC.taps("d42"), 0, QC.FS)
    assert xl.lib().xlating_batch_q15_matrix_admits(1, None, 0, 0, QC.FS) == 0


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="needs hipcc")
def test_code_object(tmp_path):
    """compiled with Q15MM_FLAGS (no SLP vectoriser), the kernel issues v_mfma_i32 and no packed FP32, no float64, and uses no scratch"""
    mk = open(os.path.join(CSRC, "Makefile")).read()
    m = re.search(r"^Q15MM_FLAGS\s*:=\s*(.+)$", mk, re.M)
    assert m and "-fno-slp-vectorize" in m.group(1)
    rule = re.search(r"^(.*): HIPFLAGS \+= \$\(Q15MM_FLAGS\)$", mk, re.M)
    assert rule and "$(BUILD)/xl_q15_mm.o" in rule.group(1)
    assert re.search(r"^\$\(BUILD\)/xl_q15_mm\.o: q15mm/xl_q15_mm\.hip ", mk, re.M) and "$(BUILD)/xl_q15_mm.o" in re.search(r"^OBJS := (.*)$", mk, re.M).group(1)
    out = str(tmp_path / "k.s")
    r = subprocess.run(["hipcc"] + HIPFLAGS + m.group(1).split() + [KERNEL, "-o", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    asm = open(out).read()
    kernels = re.findall(r"^(_Z\S*xl_q15_mm_kernel\S*):", asm, re.M)
    assert len(kernels) == 2, kernels  # one and two digit planes
    assert len(re.findall(r"^\s*v_mfma_i32_32x32x32_i8", asm, re.M)) >= 12
    assert not re.findall(r"^\s*v_pk_(?:mul|add|fma)_f32", asm, re.M)
    assert not re.findall(r"^\s*v_\w+_f64", asm, re.M)
    assert not re.findall(r"^\s*scratch_", asm, re.M)
    sizes = re.findall(r"\.private_segment_fixed_size:\s*(\d+)", asm)
    assert len(sizes) == 2 and all(int(v) == 0 for v in sizes), sizes
    spills = re.findall(r"\.(?:vgpr|sgpr)_spill_count:\s*(\d+)", asm)
    assert spills and all(int(v) == 0 for v in spills), spills
