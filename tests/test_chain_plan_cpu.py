"""CPU test (-m "not gpu") of the chain wave's region cover (csrc/xl_chain_plan.h, used by xl_nco_chain_kernel): a stand-alone host
program with its own main (tests/c/chain_plan_sweep.cpp), built with ASan and UBSan and run as a process of its own, sweeps every
(e, e_stop) with 0 <= e <= e_stop <= 400: every entry covered exactly once and in order, 32-entry blocks only at ring slots 0 and 32
and never over the ring's end, head and tail at most 31 entries, an empty region an empty plan."""
import os
import shutil
import subprocess

from conftest import ROOT

CSRC = os.path.join(ROOT, "sdr-server_amd", "csrc")
SWEEP_SRC = os.path.join(ROOT, "tests", "c", "chain_plan_sweep.cpp")
CXX = shutil.which("g++") or "/opt/rocm/lib/llvm/bin/clang++"


def test_plan_sweep_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "chain_plan_sweep")
    r = subprocess.run([CXX, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I", CSRC, SWEEP_SRC, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok "), (r.stdout[-500:], r.stderr[-2000:])
    assert int(r.stdout.split()[1]) == 401 * 402 // 2

