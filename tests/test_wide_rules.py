"""CPU tests (-m "not gpu") of the wide direct FIR's routing rule (sdr-server_amd/csrc/xl_wide.h, plain C) and of its code object:
xl_fir_needs_wide is true exactly where no LDS tile of the direct kernel fits (xl_fir_pick_ota returns 0), and xl_wide.hip, compiled
for gfx950 with its Makefile flag, issues no packed FP32 (the wide launch runs in the same calls as the matrix-core launches)."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "sdr-server_amd", "csrc")
SHIM = r"""
#include "xl_wide.h"
int needs(unsigned D, unsigned T, unsigned m) { return xl_fir_needs_wide(D, T, m); }
"""


def _lib(tmp_path):
    import ctypes

    src = tmp_path / "wide.c"
    src.write_text(SHIM)
    so = str(tmp_path / "wide.so")
    subprocess.run(["gcc", "-std=c11", "-O1", "-shared", "-fPIC", "-I", CSRC, str(src), "-o", so], check=True)
    return ctypes.CDLL(so)


def pick_ota(D, tpad):
    """xl_fir_pick_ota(D, Tpad, 160 KiB) of xl_kernels.hip, restated"""
    for ota in (64, 32, 16, 8):
        if ((ota - 1) * D + tpad) * 8 <= 160 * 1024:
            return ota
    return 0


def test_needs_wide_is_where_no_tile_fits(tmp_path):
    lib = _lib(tmp_path)
    for m in (4, 12):
        for D in list(range(1, 40)) + list(range(1000, 3100, 7)) + [2925, 2926, 2927, 2928, 2929, 2930]:
            for T in (1, 2, 57, 505, 1001, 12141, 13491, 15057, 20479, 20480, 20481, 24091):
                assert lib.needs(D, T, m) == (pick_ota(D, rnd(T, m)) == 0), (D, T, m)


def test_needs_wide_boundary_shapes(tmp_path):
    lib = _lib(tmp_path)
    # the server's filters at 2.016 Msps: D = 1008 (2 kHz) still fits, D = 1120 (1.8 kHz) does not
    assert not lib.needs(1008, 12141, 12) and not lib.needs(1008, 12141, 4)
    assert lib.needs(1120, 13491, 12) and lib.needs(1120, 13491, 4)
    # the issue's rows: 16 / 12.5 / 10 kHz on 20 Msps, 8 kHz on 10 Msps, 2 kHz on 2.4 Msps
    for D, T in ((1250, 15057), (1600, 19273), (2000, 24091), (1200, 14455)):
        assert lib.needs(D, T, 12) and lib.needs(D, T, 4), (D, T)
    # every shape the default batch engine admitted before (T - 1 + D <= 16384 and a tile fits) stays on the direct kernel
    for D in (1, 21, 42, 100, 504, 505, 1000, 1075):
        T = min(12 * D + 1, 16384 - D + 1)
        assert lib.needs(D, T, 12) == (pick_ota(D, rnd(T, 12)) == 0), (D, T)
        assert not lib.needs(D, T, 12) or D > 1000, (D, T)
    assert not lib.needs(42, 505, 12) and not lib.needs(1, 20000, 4) and lib.needs(1, 20473, 4)
    assert not lib.needs(2925, 1, 4) and lib.needs(2926, 1, 4)


def test_tap_multiples_4_and_12_band(tmp_path):
    """The drop-in decides at 4 taps, the batch engine at 12: a shape the drop-in sends wide is wide in the batch engine too (no T with
    needs(D, T, 4) and not needs(D, T, 12)), and the band between them is a few taps wide -- at D = 1000 exactly T = 13477 .. 13480
    (xl_fir_kernel with the LDS exactly full at 8 outputs per wave in the drop-in, the wide kernel in the batch engine)."""
    lib = _lib(tmp_path)
    for D in list(range(1, 60)) + list(range(900, 2927, 13)) + [1000, 1075, 2925, 2926]:
        edge = max(1, 20480 - 7 * D)  # (7 D + Tpad) * 8 > 160 KiB  <=>  Tpad > 20480 - 7 D
        for T in range(max(1, edge - 40), edge + 40):
            assert not (lib.needs(D, T, 4) and not lib.needs(D, T, 12)), (D, T)
    band = [T for T in range(13000, 14000) if lib.needs(1000, T, 12) and not lib.needs(1000, T, 4)]
    assert band == [13477, 13478, 13479, 13480], band
    assert pick_ota(1000, rnd(13480, 4)) == 8 and ((8 - 1) * 1000 + 13480) * 8 == 160 * 1024  # (exactly full)
    assert not lib.needs(1000, 13476, 12) and lib.needs(1000, 13481, 4)


def rnd(t, m):
    return -(-t // m) * m


FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fhip-fp32-correctly-rounded-divide-sqrt",
         "--cuda-device-only", "-S"]


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="needs hipcc")
def test_wide_kernels_issue_no_packed_fp32(tmp_path):
    mk = open(os.path.join(CSRC, "Makefile")).read()
    m = re.search(r"^WIDE_FLAGS\s*:=\s*(.+)$", mk, re.M)
    assert m and "-fno-slp-vectorize" in m.group(1)
    assert re.search(r"^\$\(BUILD\)/xl_wide\.o: HIPFLAGS \+= \$\(WIDE_FLAGS\)$", mk, re.M), "the Makefile must compile xl_wide.hip with WIDE_FLAGS"
    out = str(tmp_path / "w.s")
    r = subprocess.run(["hipcc"] + FLAGS + m.group(1).split() + [os.path.join(CSRC, "xl_wide.hip"), "-o", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    kernel, kernels, bad = None, set(), []
    for line in open(out):
        km = re.match(r"^(_Z\S+):", line)
        if km:
            kernel = km.group(1)
            kernels.add(kernel)
        elif kernel and re.match(r"\s*v_pk_(mul|add|fma)_f32", line):
            bad.append((kernel, line.strip()))
    assert any("xl_wide_kernel" in k for k in kernels) and any("xl_wide_q15_kernel" in k for k in kernels), sorted(kernels)[:4]
    assert not bad, bad[:5]
