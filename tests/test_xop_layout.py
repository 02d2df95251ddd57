"""CPU test (-m "not gpu") of the operand-form image of the shared spectra (sdr-server_amd/csrc/xl_xop_layout.h, the header
xlp_forward_kernel<M, 4, true> takes its store index from and xlp_mix_mfma_kernel<NKB, false, true> its copy): compiled for the
host (tests/c/test_xop_layout.cpp) -- an image written slot by slot as the forward launch writes it and copied as the mix launch
stages it equals, byte for byte, what the converting staging writes into LDS for the same float32 spectra; 1 .. 8 k-blocks,
every branch count of each, +-0, subnormal second halves and the bound of the cu8 spectra among the inputs."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

CXX = shutil.which("g++") or "/opt/rocm/lib/llvm/bin/clang++"


@pytest.mark.skipif(not os.path.exists(CXX), reason="needs a C++ compiler")
def test_operand_image_equals_the_converting_staging_byte_for_byte(tmp_path):
    exe = str(tmp_path / "test_xop_layout")
    r = subprocess.run([CXX, "-std=c++17", "-O1", os.path.join(ROOT, "tests", "c", "test_xop_layout.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "operand image layout: ok" in r.stdout
