"""CPU test (-m "not gpu") of the size rule for the operand image of the shared spectra (xlp_ximg_pays, csrc/xl_plan_rules.h): the
window it was measured ahead in (profiles/mix_operand_image.txt) -- 768 .. 1088 clients, engines whose calls cover four blocks or more."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

CC = shutil.which("gcc") or "/opt/rocm/lib/llvm/bin/clang"

SRC = r'''
#include <stdio.h>
#include "xl_plan_rules.h"
int main(void) {
  const unsigned q[][2] = {{767, 8}, {768, 8}, {1024, 8}, {1088, 8}, {1089, 8}, {1024, 3}, {1024, 4}, {1024, 64}, {32, 8}, {4096, 8}};
  for (unsigned i = 0; i < sizeof(q) / sizeof(q[0]); ++i) printf("%d", xlp_ximg_pays(q[i][0], q[i][1]));
  printf("\n");
  return 0;
}
'''


@pytest.mark.skipif(not os.path.exists(CC), reason="needs a C compiler")
def test_operand_image_size_rule_edges(tmp_path):
    src, exe = tmp_path / "rule.c", str(tmp_path / "rule")
    src.write_text(SRC)
    r = subprocess.run([CC, "-std=c11", "-I", os.path.join(ROOT, "sdr-server_amd", "csrc"), str(src), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.strip() == "0111001100", r.stdout + r.stderr
