"""CPU test (-m "not gpu") of the float families' phase look-ahead (csrc/xl_ahead.h, every decision of xl_batch.cpp's look-ahead stages): a
stand-alone host program with its own main (tests/c/ahead_sweep.cpp), built with ASan and UBSan and run as a process of its own, drives the
header through call sequences in the order of the engine's stages against a model of streams, events and happens-before (tests/c/ahead_model.h): every
sequence of five symbols out of 18 (side / fused / Q15 calls, two shapes, two caller streams and the engine's, a join, a re-plan, a re-plan
that re-creates the masked stream pair) for each chain_calls, 6000 fixed-seed random sequences of 64, and the steady patterns' counts.  The
header must also compile as plain C without any HIP header."""
import os
import shutil
import subprocess

from conftest import ROOT

CSRC = os.path.join(ROOT, "sdr-server_amd", "csrc")
SWEEP_SRC = os.path.join(ROOT, "tests", "c", "ahead_sweep.cpp")
CXX = shutil.which("g++") or "/opt/rocm/lib/llvm/bin/clang++"
CC = shutil.which("gcc") or "/opt/rocm/lib/llvm/bin/clang"


def test_ahead_sweep_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "ahead_sweep")
    r = subprocess.run([CXX, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I", CSRC, SWEEP_SRC, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("ok "), (r.stdout[-500:], r.stderr[-2000:])
    # at least one check per call of the exhaustive part: 5 settings x 18^5 sequences
    assert int(r.stdout.split()[1]) > 5 * 18 ** 5


def test_header_is_plain_c_without_hip():
    src = open(os.path.join(CSRC, "xl_ahead.h")).read()
    includes = [ln.split()[1] for ln in src.splitlines() if ln.startswith("#include")]
    assert includes == ["<stdbool.h>", "<stdint.h>", "<string.h>"], includes
    r = subprocess.run([CC, "-std=c11", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-x", "c", os.path.join(CSRC, "xl_ahead.h")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
