"""CPU test (-m "not gpu") of the mixed-spectra image Y (sdr-server_amd/csrc/xl_y_layout.h, the header the four mix kernels take
their store address from, the three inverse kernels their tile and the engine the allocation): compiled for the host
(tests/c/test_y_layout.cpp) -- writers' address == readers' address for every (column group, segment, column, bin), a bijection onto
the image, every tile one contiguous run, xly_bytes the allocated size; M = 64 / 128 / 256, 1 and 3 column groups, 1 and 5 segments."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

CXX = shutil.which("g++") or "/opt/rocm/lib/llvm/bin/clang++"


@pytest.mark.skipif(not os.path.exists(CXX), reason="needs a C++ compiler")
def test_y_image_writers_and_readers_agree_and_cover_the_image_once(tmp_path):
    exe = str(tmp_path / "test_y_layout")
    r = subprocess.run([CXX, "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "c", "test_y_layout.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Y layout: ok" in r.stdout
