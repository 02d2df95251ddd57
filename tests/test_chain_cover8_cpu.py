"""CPU test (-m "not gpu") of the chain wave's region cover with aligned 8-entry runs (xl_chain_plan8, csrc/xl_chain_plan.h, used by
xl_nco_chain_kernel): a stand-alone host program with its own main (tests/c/chain_cover8_sweep.cpp), built with ASan and UBSan and run
as a process of its own, sweeps every first entry 0 .. 191 and every length 0 .. 300: the five parts sum to the length, fewer than 8
any-slot entries and at most three 8-entry runs on either side, every run at a slot that is a multiple of 8 and every block at one that
is a multiple of 32, nothing over the ring's end, head and tail shorter than a block, every entry once and in order."""
import os
import shutil
import subprocess

from conftest import ROOT

CSRC = os.path.join(ROOT, "sdr-server_amd", "csrc")
SWEEP_SRC = os.path.join(ROOT, "tests", "c", "chain_cover8_sweep.cpp")
CXX = shutil.which("g++") or "/opt/rocm/lib/llvm/bin/clang++"


def test_cover8_sweep_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "chain_cover8_sweep")
    r = subprocess.run([CXX, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I", CSRC, SWEEP_SRC, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok "), (r.stdout[-500:], r.stderr[-2000:])
    assert int(r.stdout.split()[1]) == 192 * 301
