"""CPU tests (-m "not gpu") of the spectrum bank's wide entry (xlating_spectrum_bank_create_wide, SpectrumBank(wide=True)): every
refusal, decided before the device is touched and with *out left alone; the default entry's unchanged refusal of 8193; the no-device
answer; the wide bank's integer rules (sdr-server_amd/csrc/xl_spectrum_bank_plan.h) as a stand-alone program under ASan and UBSan; the
kernels' scalar-FP32 code object and their one shared body; the knobs' gate; a C caller built against the header alone."""
import ctypes as C
import errno
import os
import re
import shutil
import subprocess

import pytest

import sdr_server_amd as xl
from conftest import ROOT

CSRC = os.path.join(ROOT, "sdr-server_amd", "csrc")
SWEEP_SRC = os.path.join(ROOT, "tests", "c", "spectrum_bank_plan_sweep.c")
DEMO_SRC = os.path.join(ROOT, "tests", "c", "spectrum_bank_wide_demo.c")
MAX_WIDE = 1048576
SENTINEL = 0x5A5A5A5A


def _have_gpu():
    try:
        return "no usable device" not in xl.device_info()
    except Exception:
        return False


def test_bank_create_wide_refusals(capfd):
    """widths 0, -1 and 1048577 and formats 1, 4 and -1: -EINVAL with *out untouched and not a word on stderr (the device probe's "<3>"
    line would be one: nothing looked for a device); NULL out"""
    S = xl.spectrum_lib()
    capfd.readouterr()
    for w, fmt in [(0, 0), (-1, 0), (MAX_WIDE + 1, 0), (20000, 1), (20000, 4), (20000, -1), (64, 1), (MAX_WIDE + 1, 1)]:
        h = C.c_void_p(SENTINEL)
        assert S.xlating_spectrum_bank_create_wide(w, fmt, C.byref(h)) == -errno.EINVAL, (w, fmt)
        assert h.value == SENTINEL, (w, fmt)
    assert S.xlating_spectrum_bank_create_wide(20000, 0, None) == -errno.EINVAL
    assert S.xlating_spectrum_bank_create_wide(64, 0, None) == -errno.EINVAL
    assert capfd.readouterr().err == ""
    with pytest.raises(xl.XlatingError) as e:
        xl.SpectrumBank(MAX_WIDE + 1, "cf32", wide=True)
    assert e.value.code == -errno.EINVAL
    with pytest.raises(xl.XlatingError) as e:
        xl.SpectrumBank(20000, "cs8", wide=True)
    assert e.value.code == -errno.EINVAL


def test_default_bank_entry_still_refuses_8193():
    S = xl.spectrum_lib()
    h = C.c_void_p(SENTINEL)
    assert S.xlating_spectrum_bank_create(8193, 0, C.byref(h)) == -errno.EINVAL
    assert S.xlating_spectrum_bank_create(MAX_WIDE, 3, C.byref(h)) == -errno.EINVAL
    assert h.value == SENTINEL
    with pytest.raises(xl.XlatingError) as e:
        xl.SpectrumBank(8193, "cf32")
    assert e.value.code == -errno.EINVAL
    with pytest.raises(xl.XlatingError) as e:
        xl.SpectrumBank(8193, "cf32", wide=False)
    assert e.value.code == -errno.EINVAL


def test_valid_wide_bank_without_a_gpu_is_enodev(capfd):
    if _have_gpu():
        pytest.skip("checks the no-device answer")
    S = xl.spectrum_lib()
    for w, fmt in [(8193, 0), (48000, 3), (MAX_WIDE, 2), (256, 3)]:
        h = C.c_void_p(SENTINEL)
        capfd.readouterr()
        assert S.xlating_spectrum_bank_create_wide(w, fmt, C.byref(h)) == -errno.ENODEV, (w, fmt)
        err = capfd.readouterr().err
        assert "<3>" in err and "xlating_spectrum_bank_create_wide" in err
        assert not h.value
    with pytest.raises(xl.XlatingError) as e:
        xl.SpectrumBank(48000, "cf32", wide=True)
    assert e.value.code == -errno.ENODEV


def test_wide_symbol_is_exported_and_declared():
    src = open(os.path.join(ROOT, "include", "xlating_spectrum.h")).read()
    assert re.search(r"^int xlating_spectrum_bank_create_wide\(int width, int format, xlating_spectrum_bank \*\*out\);$", src, re.M)
    assert "xlating_spectrum_bank_create_wide" in xl.SPECTRUM_SYMBOLS
    out = subprocess.run(["nm", "-D", "--defined-only", xl.spectrum_library_path()], capture_output=True, text=True).stdout
    assert " T xlating_spectrum_bank_create_wide" in out
    assert "hip/" not in src
    import inspect

    assert inspect.signature(xl.SpectrumBank.__init__).parameters["wide"].default is False


# ------------------------------------------------------------------------------------------------------------ the rules
def test_bank_plan_header_is_plain_c(tmp_path):
    hdr = open(os.path.join(CSRC, "xl_spectrum_bank_plan.h")).read()
    assert "#include <hip" not in hdr and "hipLaunch" not in hdr and "__device__" not in hdr
    src = tmp_path / "t.c"
    src.write_text('#include "xl_spectrum_bank_plan.h"\nint main(void) { return (int)xl_bankw_chunks(0, 1); }\n')
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-pedantic", "-I", CSRC, str(src), "-o", str(tmp_path / "t")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_bank_plan_sweep_under_the_sanitizers(tmp_path):
    """chunks cover a round's transforms exactly once for scratch sizes holding 1, 2, 3, ... transforms; the rows-per-round bound never
    yields an empty round: a program of its own with ASan and UBSan"""
    exe = str(tmp_path / "spectrum_bank_plan_sweep")
    r = subprocess.run(["gcc", "-std=c11", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I", CSRC, SWEEP_SRC, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok ") and r.stderr == "", (r.stdout[-500:], r.stderr[-2000:])
    assert int(r.stdout.split()[1]) >= 20000


def test_the_bank_takes_its_rules_from_the_plan_headers():
    host = re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, "xl_spectrum_bank.cpp")).read())
    for name in ("xl_specw_chunk(", "xl_bankw_chunks(", "xl_bankw_chunk_len(", "xl_bankw_stage_rows(", "xl_bankw_round_limit(",
                 "xl_bankw_first_streams(", "xl_specw_scratch_bytes("):
        assert name in host, name
    assert "XLATING_SPECTRUM_MAX_WIDE_WIDTH" in host


# ------------------------------------------------------------------------------------------------------------ build and source
def test_wide_passes_have_one_body():
    """the bit-identity of wide bank rows and single wide rows rests on one definition of what a workgroup does in each pass: defined in
    xl_spectrum_wide_dev.h only; both kernel files call each once and neither transforms, takes a power or flushes a maximum itself.
    The dB of a finished column and the bits that enter a maximum are the narrow object's: one definition of each, in
    xl_spectrum_dev.h, and no logarithm or bit cast of a power here"""
    dev = open(os.path.join(CSRC, "xl_spectrum_wide_dev.h")).read()
    for name in ("xl_specw_col_in", "xl_specw_row", "xl_specw_col_out", "xl_specw_finish_col"):
        assert len(re.findall(r"^XL_DEV \w+ %s\(" % name, dev, re.M)) == 1, name
    narrow = open(os.path.join(CSRC, "xl_spectrum_dev.h")).read()
    for name in ("xl_spec_db", "xl_spec_max_bits"):
        assert len(re.findall(r"^XL_DEV \w+ %s\(" % name, narrow, re.M)) == 1, name
    code = re.sub(r"//[^\n]*", "", dev)
    assert "xl_specw_db" not in dev and "log10" not in code and "__float_as_uint" not in code
    assert len(re.findall(r"\bxl_spec_db\(", code)) == 1 and len(re.findall(r"atomicMax\([^;]*xl_spec_max_bits\(pw\)\);", code)) == 2
    assert len(re.findall(r"atomicMax\(", code)) == 2
    for f in ("xl_spectrum_wide.hip", "xl_spectrum_bank_wide.hip"):
        src = open(os.path.join(CSRC, f)).read()
        code = re.sub(r"//[^\n]*", "", src)
        assert '#include "xl_spectrum_wide_dev.h"' in src
        for call in (r"\bxl_specw_col_in<N1, N2, FMT, BLUE>\(", r"\bxl_specw_row<N1, N2, BLUE>\(", r"\bxl_specw_col_out<N1, N2>\(",
                     r"\bxl_specw_finish_col\(", r"\bxl_specw_dispatch\("):
            assert len(re.findall(call, code)) == 1, (f, call)
        for own in ("atomicMax", "xl_fft_lds", "xl_spec_point", "xl_spec_power", "xl_spec_blue_mid", "log10", "xl_spec_db", "xl_spec_max_bits", "xl_spec_pixel", "case "):
            assert own not in code, (f, own)
    bank = re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, "xl_spectrum_bank_wide.hip")).read())
    assert "xl_ragged_find(" in bank and "xl_specw_col_pos(" in bank and "XL_SPECW_N2(" in bank


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="needs hipcc")
def test_wide_bank_kernels_issue_no_packed_fp32(tmp_path):
    """compiled with SPEC_FLAGS, and the gfx950 code holds no v_pk_{mul,add,fma}_f32 and no matrix instruction; every transform length
    has its kernels"""
    mk = open(os.path.join(CSRC, "Makefile")).read()
    m = re.search(r"^SPEC_FLAGS\s*:=\s*(.+)$", mk, re.M)
    assert m and "-fno-slp-vectorize" in m.group(1)
    assert re.search(r"^\$\(BUILD\)/xl_spectrum_bank_wide_dev\.o: HIPFLAGS \+= \$\(SPEC_FLAGS\)$", mk, re.M)
    assert re.search(r"^\$\(BUILD\)/xl_spectrum_bank_wide_dev\.o: xl_spectrum_bank_wide\.hip", mk, re.M)
    assert re.search(r"^SPEC_OBJS :=.*\$\(BUILD\)/xl_spectrum_bank_wide_dev\.o", mk, re.M)
    assert re.search(r"^HIPFLAGS :=.*-ffp-contract=off", mk, re.M)
    out = str(tmp_path / "k.s")
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fhip-fp32-correctly-rounded-divide-sqrt",
             "--cuda-device-only", "-S"]
    r = subprocess.run(["hipcc"] + flags + m.group(1).split() + [os.path.join(CSRC, "xl_spectrum_bank_wide.hip"), "-o", out],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    asm = open(out).read()
    names = set(re.findall(r"^(_Z\w*xl_bankw_\w+):", asm, re.M))
    count = lambda part: sum(part in n for n in names)  # noqa: E731
    # 7 plain + 7 Bluestein lengths: three formats of the column-in pass, one row pass each; the column-out pass for Bluestein only
    assert count("xl_bankw_col_in_kernel") == 14 * 3 and count("xl_bankw_row_kernel") == 14 and count("xl_bankw_col_out_kernel") == 7, names
    assert count("xl_bankw_carry_kernel") == 3 and count("xl_bankw_finish_kernel") == 1
    assert not re.search(r"^\s*v_pk_(mul|add|fma)_f32", asm, re.M)
    assert "v_mfma" not in asm
    src = open(os.path.join(CSRC, "xl_spectrum_bank_wide.hip")).read()
    assert not re.search(r"\b(sinf?|cosf?|sincosf?|__sinf|__cosf)\s*\(", re.sub(r"//[^\n]*", "", src))
    assert "hipfft" not in src.lower() and "rocfft" not in src.lower() and "__builtin_amdgcn_mfma" not in src


def test_wide_bank_knobs_go_through_the_gate():
    src = open(os.path.join(CSRC, "xl_spectrum_bank.cpp")).read()
    assert 'xl_exp_getenv("XL_EXP_SPEC_BANK_STAGE")' in src
    assert not re.findall(r'(?<!xl_exp_)getenv\(', src)
    one = open(os.path.join(CSRC, "xl_spectrum.cpp")).read()  # the scratch knob is read in one place, for both objects
    assert one.count('xl_exp_getenv("XL_EXP_SPEC_SCRATCH")') == 1 and "uint64_t xl_specw_scratch_bytes(void)" in one


def test_wide_bank_c_caller_builds_against_the_header_alone(tmp_path):
    exe = str(tmp_path / "spectrum_bank_wide_demo")
    libdir = os.path.dirname(xl.spectrum_library_path())
    r = subprocess.run(["gcc", "-std=c11", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), DEMO_SRC, "-o", exe,
                        "-L", libdir, "-lxlating_spectrum", f"-Wl,-rpath,{libdir}"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    und = subprocess.run(["nm", "-u", exe], capture_output=True, text=True).stdout
    assert "xlating_spectrum_bank_create_wide" in und and "hip" not in und.lower()
    # refusals run end to end without a device: width 1048577 through both entries
    r = subprocess.run([exe, str(MAX_WIDE + 1), "3", "2000000"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and r.stdout.split() == [str(-errno.EINVAL), str(-errno.EINVAL)], (r.stdout, r.stderr)
    if not _have_gpu():
        r = subprocess.run([exe, "48000", "3", "48000"], capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and r.stdout.split() == [str(-errno.EINVAL), str(-errno.ENODEV)] and "<3>" in r.stderr
