"""CPU tests (-m "not gpu") of the Q15 phase look-ahead (engine option "q15_nco"; csrc/xl_kernels.hip: xl_nco_q15_ahead_kernel): the
kernel's code object, the yardstick kernel's instruction text against the parent commit's, the premises of the packed step (every
increment component in -32767 .. 32767; no saturating line of the recurrence ever acts on a reachable state), and the look-ahead's state and
decisions (csrc/xl_q15_ahead.h) in a stand-alone program under ASan and UBSan."""
import os
import re
import shutil
import subprocess

import numpy as np

import q15_extremes_cases as QC
import xlating_q15_ref as QR
from conftest import ROOT
from pyoracle import Oracle

CSRC = os.path.join(ROOT, "sdr-server_amd", "csrc")
KERNELS = os.path.join("sdr-server_amd", "csrc", "xl_kernels.hip")
ONLY_ASM = ["--cuda-device-only", "-S"]
CXX = shutil.which("g++") or "/opt/rocm/lib/llvm/bin/clang++"
CC = shutil.which("gcc") or "/opt/rocm/lib/llvm/bin/clang"


def _makefile_hipflags():
    """the Makefile's HIPFLAGS for xl_kernels.o (no per-file additions), without what only a host object needs"""
    mk = open(os.path.join(CSRC, "Makefile")).read()
    m = re.search(r"^HIPFLAGS := (.*\\\n.*)$", mk, re.M)
    assert m, "HIPFLAGS not found in the Makefile"
    flags = m.group(1).replace("\\\n", " ").split()
    arch = re.search(r"^ARCH\s*\?=\s*(\S+)$", mk, re.M).group(1)
    assert arch == "gfx950" and "-O3" in flags and "-ffp-contract=off" in flags
    assert not re.search(r"xl_kernels\.o[^\n]*: HIPFLAGS \+=", mk)
    return [f.replace("$(ARCH)", arch) for f in flags if f not in ("-fPIC", "-Wall", "-Wno-unused-function")]


def _asm(src, out):
    r = subprocess.run(["hipcc"] + _makefile_hipflags() + ONLY_ASM + ["-I", CSRC, src, "-o", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return open(out).read()


def _body(asm, kernel):
    """the instruction text of one kernel: label to s_endpgm, without comments, directives and the numbering of local labels"""
    m = re.search(r"^(_Z\d+%s\w*):.*?\n(.*?\n\s*s_endpgm)" % kernel, asm, re.M | re.S)
    assert m, kernel
    lines = []
    for ln in m.group(2).splitlines():
        ln = re.sub(r"\.LBB\d+_", ".LBB_", ln.split(";")[0]).strip()
        if ln and not ln.startswith("."):
            lines.append(ln)
        elif ln.startswith(".LBB_"):
            lines.append(ln)
    return m.group(1), lines


GOLDEN_BATCH = os.path.join(ROOT, "tests", "golden", "q15_nco_batch_kernel_gfx950.txt")


def _parent_source(tmp_path):
    """sdr-server_amd/csrc/xl_kernels.hip as the parent of the change that last touched it holds it: `git show HEAD~:...` in a checkout
    of that change; in a working tree that holds the change uncommitted, HEAD is that parent.  None where the tree has no history to
    ask (an export, a shallow checkout): the recorded text then stands in."""
    cfg = tmp_path / "gitconfig"
    cfg.write_text("[safe]\n\tdirectory = *\n")  # (a checkout owned by another user is still this project's)
    env = dict(os.environ, GIT_CONFIG_GLOBAL=str(cfg))

    def git(*a):
        try:
            r = subprocess.run(["git", "-C", ROOT] + list(a), capture_output=True, env=env)
        except OSError:
            return None
        return r.stdout if r.returncode == 0 else None
    last = git("log", "-1", "--format=%H", "--", KERNELS)
    if not last or not last.strip():
        return None
    last = last.decode().strip()
    here = open(os.path.join(ROOT, KERNELS), "rb").read()
    rev = last + "~" if git("show", f"{last}:{KERNELS}") == here else "HEAD"
    src = git("show", f"{rev}:{KERNELS}")
    return src.decode() if src else None


def test_code_object(tmp_path):
    """xl_nco_q15_ahead_kernel: 16 unrolled steps of two packed int16 dot products and one saturating pack each -- at least 32 and 16
    of them -- no packed FP32, no matrix instruction and no scratch anywhere in it, no v_med3_i32 and no multiply inside the unrolled stretch.  The dot product is
    v_dot2_i32_i16 in either encoding: the compiler picks v_dot2c_i32_i16, the two-operand form that adds into a zeroed destination.
    xl_nco_q15_batch_kernel, option 0 and the yardstick of every measurement, has the parent's instruction text: the parent's file
    compiled here, and the text recorded from it when the option was added (tests/golden/, the compiler of that day)."""
    asm = _asm(os.path.join(ROOT, KERNELS), str(tmp_path / "k.s"))
    sym, ahead = _body(asm, "xl_nco_q15_ahead_kernel")
    ops = [ln.split()[0] for ln in ahead]
    assert sum(bool(re.fullmatch(r"v_dot2c?_i32_i16(_e32|_e64)?", o)) for o in ops) >= 32, ops
    assert sum(o.startswith("v_cvt_pk_i16_i32") for o in ops) >= 16
    assert not [o for o in ops if re.match(r"v_pk_\w+_f32|v_mfma|v_smfmac|scratch_", o)], ops
    # the unrolled stretch -- from the table store to the loop's branch -- is one store and 16 whole steps, straight-line
    first = next(i for i, o in enumerate(ops) if o.startswith("global_store_dword"))
    stretch = ops[first:next(i for i in range(first, len(ops)) if ops[i].startswith("s_cbranch"))]
    assert sum(o.startswith("v_cvt_pk_i16_i32") for o in stretch) == 16 and sum(o.startswith("v_dot2") for o in stretch) == 32, stretch
    assert sum(o.startswith("global_store") for o in stretch) == 1 and not [o for o in stretch if o.startswith(("global_load", "s_load", ".LBB"))], stretch
    assert not [o for o in stretch if re.match(r"v_med3|v_mul_|v_mad_", o)], stretch  # (the output count in front of the loop divides: multiplies there)
    meta = re.search(r"\.amdhsa_kernel %s\n(.*?)\.end_amdhsa_kernel" % re.escape(sym), asm, re.S).group(1)
    assert re.search(r"\.amdhsa_private_segment_fixed_size 0\n", meta) and re.search(r"\.amdhsa_enable_private_segment 0\n", meta), meta
    # the yardstick
    _, now = _body(asm, "xl_nco_q15_batch_kernel")
    text = _parent_source(tmp_path)
    if text is not None:
        src = tmp_path / "parent_xl_kernels.hip"
        src.write_text(text)
        _, then = _body(_asm(str(src), str(tmp_path / "p.s")), "xl_nco_q15_batch_kernel")
        assert len(then) > 40 and now == then
    else:
        assert now == open(GOLDEN_BATCH).read().split("\n")[:-1]


def _increments():
    """the Q15 increment of every (fc, D) the GPU tests of the option use, and of fc = 0, +-fs/4, +-fs/2: {(ir, ii): (fc, D)}"""
    cases = set()
    for D, _ in ((1, 16), (3, 81), (7, 81), (42, 505), (64, 505)):
        cases |= {(fc, D) for fc in QC.FC_D42[:5]}
    cases |= {(fc, QC.SHAPE_D[s]) for s, fc in QC.SAT_CLIENTS}
    cases |= {(fc, QC.SHAPE_D[s]) for s in QC.CHURN_SHAPES for fc in QC.CHURN_FCS}
    cases |= {(QC.FC_D42[c % len(QC.FC_D42)] + 5 * (c // len(QC.FC_D42)), 42) for c in range(10)}
    cases |= {(QC.GOLDEN_WRAP["fc"], QC.GOLDEN_WRAP["D"]), (1234, 42)}
    cases |= {(-1000000 + 1953 * c, 42) for c in range(1024)}
    cases |= {(fc, 42) for fc in (0, QC.FS // 4, -QC.FS // 4, QC.FS // 2, -QC.FS // 2)}
    tap = np.array([1.0], np.float32)
    out = {}
    for fc, D in sorted(cases):
        o = Oracle(D, tap, fc, QC.FS, QC.MAXIN)
        out.setdefault(QR.increment(o.phase_incr), (fc, D))
        o.close()
    return out


def test_increment_components_fit_the_packed_operand():
    """a = (ir, -ii) is an int16 pair only if ii > -32768: the components are (int16)(c * 32767) of |c| <= 1 (xlating.c:548-549)"""
    incs = _increments()
    assert len(incs) > 1000
    for (ir, ii), case in incs.items():
        assert -32767 <= ir <= 32767 and -32767 <= ii <= 32767, (case, ir, ii)
    assert (32767, 0) in incs and (-32767, 0) in incs  # fc = 0 and fs / 2: the extremes are reached


def test_no_clamp_of_the_step_is_reachable():
    """The int64 restatement's recurrence (tests/xlating_q15_ref.py, xlating.c:126-129) from the reference's start phase (32767, 0), 300 000
    steps for every increment above: neither saturating line ever acts and no component leaves -32767 .. 32767.  So the GPU tests of
    the option do NOT exercise the saturation of v_cvt_pk_i16_i32 -- states that saturate are unreachable from the start phase; the
    packed step and the yardstick's v_med3_i32 agree on them by the instructions' definitions only.  (Checked apart from this test
    for 4006 random and special increments x 30 000 steps: zero clamps, largest component 32767.)"""
    incs = np.array(sorted(_increments()), np.int64)
    ir, ii = incs[:, 0], incs[:, 1]
    pr, pi = np.full(ir.shape, 32767, np.int64), np.zeros(ir.shape, np.int64)
    lo, hi = 0, 0
    for _ in range(300000):
        tr, ti = (pr * ir - pi * ii) >> 15, (pr * ii + pi * ir) >> 15
        lo, hi = min(lo, int(tr.min()), int(ti.min())), max(hi, int(tr.max()), int(ti.max()))
        pr, pi = tr, ti  # (unclamped: the assertion below says the clamp would have been the identity)
        if hi > 32767 or lo < -32767:
            break
    assert -32767 <= lo and hi <= 32767, (lo, hi)


def test_ahead_sweep_under_the_sanitizers(tmp_path):
    """tests/c/q15_ahead_sweep.cpp, a program of its own: the two predicates position by position, then the header's state and decisions
    through every sequence of five symbols out of 13 (from option 0 and 1, from trel = 0 and just short of 2^31), 6000 random sequences
    of 64 and the steady patterns, on the device model it shares with the float look-ahead's sweep (tests/c/ahead_model.h)."""
    exe = str(tmp_path / "q15_ahead_sweep")
    r = subprocess.run([CXX, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I", CSRC, os.path.join(ROOT, "tests", "c", "q15_ahead_sweep.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("ok "), (r.stdout[-500:], r.stderr[-2000:])
    positions, sequences = (int(v) for v in r.stdout.split()[1:3])
    assert positions >= 500000, r.stdout  # (the per-position sweeps ran)
    assert sequences > 4 * 13 ** 5, r.stdout  # at least one check per sequence of the exhaustive part: 4 settings x 13^5


def test_header_is_plain_c_without_hip():
    src = open(os.path.join(CSRC, "xl_q15_ahead.h")).read()
    includes = [ln.split()[1] for ln in src.splitlines() if ln.startswith("#include")]
    assert includes == ["<stdbool.h>", "<stdint.h>", '"xl_grid.h"', '"xl_ahead.h"'], includes
    r = subprocess.run([CC, "-std=c11", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-x", "c", os.path.join(CSRC, "xl_q15_ahead.h")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
