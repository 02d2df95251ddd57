"""CPU test (-m "not gpu") of the host logic of the batch engine's plan (csrc/xl_plan.h, xl_plan.cpp: class formation and the column
hand-out across re-plans, the measured size rules, the direct launch sets, the output rows, the end-of-call commit, tile height and CU
reservation): a stand-alone host program with its own main (tests/c/plan_sweep.cpp) that links xl_plan.cpp, built with ASan and UBSan
and run as a process of its own.  It asserts its checks after every plan of a fixed-seed churn and prints "ok <plans> <checks>"."""
import os
import re
import shutil
import ctypes
import subprocess

import sdr_server_amd as xl
from conftest import ROOT

CSRC = os.path.join(ROOT, "sdr-server_amd", "csrc")
SOURCES = [os.path.join(ROOT, "tests", "c", "plan_sweep.cpp"), os.path.join(CSRC, "xl_plan.cpp")]
CXX = shutil.which("g++") or "/opt/rocm/lib/llvm/bin/clang++"
ROCM_INCLUDE = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")  # (hip_runtime.h's types only: nothing of HIP is linked)
FLAGS = ["-std=c++17", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def test_plan_sweep_under_the_sanitizers(tmp_path):
    objs = [str(tmp_path / (os.path.basename(s) + ".o")) for s in SOURCES]
    procs = [subprocess.Popen([CXX] + FLAGS + ["-I", CSRC, "-I", ROCM_INCLUDE, "-D__HIP_PLATFORM_AMD__", "-c", s, "-o", o],
                              stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for s, o in zip(SOURCES, objs)]
    for p in procs:
        _, err = p.communicate()
        assert p.returncode == 0, err[-2000:]
    exe = str(tmp_path / "plan_sweep")
    r = subprocess.run([CXX, "-fsanitize=address,undefined"] + objs + ["-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok "), (r.stdout[-500:], r.stderr[-2000:])
    plans, checks = (int(v) for v in r.stdout.split()[1:3])
    assert plans >= 400 and checks >= 100000, r.stdout  # (the churn planned, and its checks ran)


def test_plan_files_call_no_hip_function():
    for name in ("xl_plan.cpp", "xl_plan.h"):
        assert re.search(r"hip[A-Z]", open(os.path.join(CSRC, name)).read()) is None, name


def test_sweeps_window_image_size_is_the_librarys():
    """tests/c/plan_sweep.cpp links xl_plan.cpp alone and carries its own xl_fir_lds_bytes_ota; the library's (xl_kernels.hip) must be
    the same function, or the sweep's tile heights and 160 KiB checks would hold for a formula the kernels no longer use."""
    fn = getattr(xl.lib(), "_Z20xl_fir_lds_bytes_otajjj")
    fn.restype, fn.argtypes = ctypes.c_size_t, [ctypes.c_uint32] * 3
    m = re.search(r"size_t xl_fir_lds_bytes_ota\(uint32_t D, uint32_t Tpad, uint32_t ota\) \{ return (.*?); \}", open(SOURCES[0]).read())
    assert m and m.group(1) == "((size_t)(ota - 1u) * D + Tpad) * 8u", m
    for D, Tpad, ota in ((42, 508, 64), (42, 516, 64), (400, 104, 32), (1, 4, 8), (2925, 12, 8), (504, 1008, 16)):
        assert fn(D, Tpad, ota) == ((ota - 1) * D + Tpad) * 8, (D, Tpad, ota)
