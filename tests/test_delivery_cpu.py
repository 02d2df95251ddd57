"""CPU tests (-m "not gpu") of the delivery object and the serve object (include/xlating_delivery.h, include/xlating_serve.h): the layout
header is plain C and passes its sweep as a program of its own under ASan and UBSan; the refusals that need no device; the exported
symbols; the pack kernel's code object (no floating-point instruction, 16-byte global accesses, no LDS, no scratch); the engine's bulk
row lookup refuses as the single one does; the new code calls the layout header and never the fetches."""
import ctypes as C
import errno
import os
import re
import shutil
import subprocess

import sdr_server_amd as xl
from conftest import ROOT

CSRC = os.path.join(ROOT, "sdr-server_amd", "csrc")
SWEEP_SRC = os.path.join(ROOT, "tests", "c", "delivery_plan_sweep.c")


def _strip(path):
    return re.sub(r"/\*.*?\*/", "", re.sub(r"//[^\n]*", "", open(path).read()), flags=re.S)


def test_plan_header_is_plain_c(tmp_path):
    hdr = open(os.path.join(CSRC, "xl_delivery_plan.h")).read()
    assert "#include <hip" not in hdr and "hipLaunch" not in hdr
    src = tmp_path / "t.c"
    src.write_text('#include "xl_delivery_plan.h"\nint main(void) { return (int)xl_dlv_chunks(0); }\n')
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-pedantic", "-I", CSRC, str(src), "-o", str(tmp_path / "t")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_plan_sweep_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "delivery_plan_sweep")
    r = subprocess.run(["gcc", "-std=c11", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I", CSRC, SWEEP_SRC, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok ") and r.stderr == "", (r.stdout[-500:], r.stderr[-2000:])
    assert int(r.stdout.split()[1]) >= 10000


def test_layout_has_one_home():
    """offsets, chunk count and the run table come from xl_delivery_plan.h alone: the host calls its functions, the kernel its search
    helpers, and neither aligns an offset itself"""
    host, dev = _strip(os.path.join(CSRC, "xl_delivery.cpp")), _strip(os.path.join(CSRC, "xl_delivery.hip"))
    for name in ("xl_dlv_plan(", "xl_dlv_chunks("):
        assert name in host, name
    for name in ("xl_ragged_find(", "xl_dlv_first(", "xl_dlv_span("):
        assert name in dev, name
    assert "xl_dlv_place" not in host and "xl_dlv_place" not in dev
    assert "xl_ring_acquire(" in host and "xl_ring_upload(" in host  # (the banks' pinned ring)
    assert xl.delivery_chunk_bytes() == int(re.search(r"#define XL_DLV_CHUNK (\d+)u", open(os.path.join(CSRC, "xl_delivery_plan.h")).read()).group(1))


def test_serve_never_fetches():
    serve = _strip(os.path.join(CSRC, "xl_serve.cpp"))
    assert "xlating_batch_fetch" not in serve and "_bank_fetch" not in serve and "output_host" not in serve
    for name in ("xlating_batch_outputs_device(", "xlating_batch_record_event(", "xlating_delivery_pack_device(", "xlating_sinks_write_bytes("):
        assert name in serve, name


def test_pack_kernel_code_object(tmp_path):
    """compiled with the Makefile's flags, the gfx950 code of xl_delivery.hip moves 16 bytes at a time through global (not flat)
    accesses, uses no LDS and no scratch, and holds no floating-point, packed or matrix instruction"""
    mk = open(os.path.join(CSRC, "Makefile")).read()
    m = re.search(r"^DELIVERY_FLAGS\s*:=\s*(.+)$", mk, re.M)
    assert m and "-fno-slp-vectorize" in m.group(1)
    assert re.search(r"^\$\(BUILD\)/xl_delivery_dev\.o: HIPFLAGS \+= \$\(DELIVERY_FLAGS\)$", mk, re.M)
    assert re.search(r"^\$\(BUILD\)/xl_delivery_dev\.o: xl_delivery\.hip", mk, re.M)
    assert re.search(r"^all:.*\$\(SERVE\)", mk, re.M)
    assert "asm" not in _strip(os.path.join(CSRC, "xl_delivery.hip"))
    out = str(tmp_path / "k.s")
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fhip-fp32-correctly-rounded-divide-sqrt",
             "--cuda-device-only", "-S"]
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"  # (where build() looks for it)
    r = subprocess.run([hipcc] + flags + m.group(1).split() + [os.path.join(CSRC, "xl_delivery.hip"), "-o", out],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    asm = open(out).read()
    assert "xl_dlv_pack_kernel" in asm
    ops = re.findall(r"^\s+([a-z][a-z0-9_]+)\s", asm, re.M)
    assert "global_load_dwordx4" in ops and "global_store_dwordx4" in ops
    assert not [o for o in ops if o.startswith(("flat_", "ds_", "scratch_", "v_pk_", "v_mfma", "v_smfma"))]
    assert not [o for o in ops if re.search(r"_(f16|bf16|f32|f64)(_|$)", o)], "a floating-point instruction"
    assert re.search(r"\.group_segment_fixed_size:\s*0\b", asm) and re.search(r"\.private_segment_fixed_size:\s*0\b", asm)


def test_symbols_are_exported():
    V = xl.serve_lib()
    for name in xl.DELIVERY_SYMBOLS + xl.SERVE_SYMBOLS:
        assert hasattr(V, name), name
    L = xl.lib()
    for name in ("xlating_batch_outputs_device", "xlating_sinks_attach_file_as", "xlating_sinks_write_bytes"):
        assert hasattr(L, name) and name in xl.EXPORTED_SYMBOLS, name


def test_refusals_need_no_device(tmp_path):
    V = xl.serve_lib()
    h = C.c_void_p()
    assert V.xlating_delivery_create(2, None) == -errno.EINVAL
    for slots in (0, 1, 17):
        assert V.xlating_delivery_create(slots, C.byref(h)) == -errno.EINVAL and not h.value
    one = (C.c_int * 1)(0)
    assert V.xlating_delivery_pack_device(None, 1, one, one, one, None) == -errno.EINVAL
    for name in ("xlating_delivery_query", "xlating_delivery_wait", "xlating_delivery_release"):
        assert getattr(V, name)(None, 0) == -errno.EINVAL
    assert V.xlating_delivery_last_ops(None, None, None, None) == -errno.EINVAL
    V.xlating_delivery_destroy(None)
    assert V.xlating_serve_create(None, C.byref(h)) == -errno.EINVAL
    cfg = xl.ServeConfig(192000, xl.FMT["cu8"], 65536, 1, -1, 7, 0, 1, 5, str(tmp_path).encode(), 0, 2, 0, 2, 0)
    assert V.xlating_serve_create(C.byref(cfg), C.byref(h)) == -errno.EINVAL  # (no such family)
    cfg.family, cfg.input_format = xl.SERVE_FAMILY["cs16"], xl.FMT["cf32"]
    assert V.xlating_serve_create(C.byref(cfg), C.byref(h)) == -errno.EINVAL  # (the cs16 family has no cf32 input)
    cfg.input_format, cfg.base_path = xl.FMT["cu8"], None
    assert V.xlating_serve_create(C.byref(cfg), C.byref(h)) == -errno.EINVAL
    assert V.xlating_serve_blocks_host(None, None, 0, 1) == -errno.EINVAL
    assert V.xlating_serve_flush(None) == -errno.EINVAL and V.xlating_serve_remove(None, 0) == -errno.EINVAL
    assert V.xlating_serve_dropped(None, None, 0) == 0 and not V.xlating_serve_engine(None)
    V.xlating_serve_destroy(None)
    assert xl.lib().xlating_batch_outputs_device(None, 0, None, None, None) == -errno.EINVAL
