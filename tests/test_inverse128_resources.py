"""CPU test (-m "not gpu"): what the LDS-staged inverse kernels (xlp_inverse_kernel, xl_polyphase.hip) ask of a compute unit, read from
the code object's own metadata as tools/kernel_resources.sh does (hipcc cross-compiles without a GPU, with the Makefile's flags).

xlp_inverse_kernel<128, XlpPosSwz>: a tile of exactly 32 KB, nothing in scratch, and the register count it ships with -- 104 allocated
VGPRs per lane (granule 8), four waves per SIMD.  A build at 93 registers without scratch exists (five workgroups per CU: the gather
addresses formed again in every round instead of held, the epilogue's operands loaded behind the staging barrier) and was measured:
the launch no shorter, the recurrence kernel beside it clocked lower, the call slower (profiles/inverse_epilogue_chain_runs8.txt,
DESIGN 9) -- so the bound here is the four-wave budget the kernel is built for, and a change that needs a fifth register block fails.
The 64- and 256-point instantiations hold four workgroups per CU by LDS (40448 / 40832 B) and have the 128-register budget of
four waves; they must not spill either."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fhip-fp32-correctly-rounded-divide-sqrt",
         "--cuda-device-only", "-S"]
KERNELS = {128: "_Z18xlp_inverse_kernelILi128E9XlpPosSwzEv7XlpArgs", 64: "_Z18xlp_inverse_kernelILi64E9XlpPosPadEv7XlpArgs",
           256: "_Z18xlp_inverse_kernelILi256E9XlpPosPadEv7XlpArgs"}


@pytest.fixture(scope="module")
def metadata(tmp_path_factory):
    """{kernel symbol: {field: int}} of xl_polyphase.hip's code object (the amdhsa.kernels notes in the assembly)"""
    if shutil.which("hipcc") is None:
        pytest.skip("needs hipcc")
    out = str(tmp_path_factory.mktemp("inv128") / "k.s")
    r = subprocess.run(["hipcc"] + FLAGS + [os.path.join(ROOT, "sdr-server_amd", "csrc", "xl_polyphase.hip"), "-o", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    notes = open(out).read().split("amdhsa.kernels:")[1]
    found = {}
    for blk in re.split(r"\n  - \.agpr_count:", notes)[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        found[name] = {k: int(v) for k, v in re.findall(r"\.(vgpr_count|vgpr_spill_count|sgpr_spill_count|private_segment_fixed_size|"
                                                        r"group_segment_fixed_size):\s+(\d+)", blk)}
        found[name]["agpr_count"] = int(blk.split()[0])
    return found


def test_inverse128_ships_at_four_waves_without_scratch(metadata):
    k = metadata[KERNELS[128]]
    print(k)
    assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0
    assert k["group_segment_fixed_size"] == 32768
    allocated = -(-(k["vgpr_count"] + k["agpr_count"]) // 8) * 8
    assert allocated <= 104, k
    assert 512 // allocated >= 4


@pytest.mark.parametrize("m", [64, 256])
def test_inverse_64_256_do_not_spill(metadata, m):
    k = metadata[KERNELS[m]]
    print(k)
    assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0
    assert -(-(k["vgpr_count"] + k["agpr_count"]) // 8) * 8 <= 128 and 4 * k["group_segment_fixed_size"] <= 160 * 1024
