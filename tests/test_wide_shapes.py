"""GPU tests (-m gpu) of the wide direct FIR (sdr-server_amd/csrc/xl_wide.hip): the shapes whose window image fits no LDS tile of the
direct kernel (D > ~1075 with the server's own low-pass filter), on both boundaries, against the oracle, which has no shape limit.
native cf32: BIT-EXACT; optimized (and the x86 flavours against the oracle with the same phase rules): max|d| / max|y| <= 1e-5; cs16:
exact.  Before the wide kernel existed, create_frequency_xlating_filter and xlating_batch_add_client returned -EINVAL (-22) here."""
import os
import subprocess
import sys

import numpy as np
import pytest

import siggen
import sdr_server_amd as xl
from conftest import ROOT
from pyoracle import Oracle

pytestmark = pytest.mark.gpu

REL_TOL = 1e-5


def lpf(fs, rate):
    """the server's own taps for a client of `rate` samples per second (create_low_pass_filter(1, fs, rate / 2, rate / 5))"""
    code, t = xl.create_low_pass_filter(1.0, fs, rate // 2, rate // 5)
    assert code == 0
    return t


def rel_err(got, want):
    return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-30)) if len(want) else 0.0


def bits_equal(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def signal(fmt, seed, n):
    """n scalar elements (I, Q interleaved) of a pseudo-random stream in input format fmt"""
    if fmt == "cu8":
        return siggen.xs_u8(seed, n)
    if fmt == "cs8":
        return siggen.xs_s8(seed, n)
    if fmt == "cs16":
        return siggen.xs_s16(seed, n)
    return (siggen.xs_s16(seed, n).astype(np.float32) / 32768.0).astype(np.float32)


# (fs, fmt, D, taps) -- the issue's rows and two shapes that overflow in one dimension only
def _dropin_shapes():
    return {
        "hackrf_16k": (20000000, "cs8", 1250, lambda: lpf(20000000, 16000)),
        "hackrf_10k": (20000000, "cs8", 2000, lambda: lpf(20000000, 10000)),
        "airspy_8k": (10000000, "cs16", 1250, lambda: lpf(10000000, 8000)),
        "rtl_2k": (2400000, "cu8", 1200, lambda: lpf(2400000, 2000)),
        "d1_t24001": (2016000, "cf32", 1, lambda: siggen.hamming_sinc(24001, 0.2)),
        "d3000_t3001": (2016000, "cf32", 3000, lambda: siggen.hamming_sinc(3001, 0.0002)),
    }


@pytest.mark.parametrize("name", list(_dropin_shapes()))
def test_dropin_wide_shapes_vs_oracle(name):
    fs, fmt, D, mk = _dropin_shapes()[name]
    taps = mk()
    fc = 123456 if fs > 3000000 else -54321
    max_input = 262144
    if name == "d1_t24001":
        max_input = 16384  # (every sample an output: keep the oracle quick)
    calls = [max_input, min(50002, max_input // 2 + 2), 0, max_input]  # full, partial, empty, full (never above max_input)
    variants = [("native", None), ("optimized", None), ("x86", 1), ("x86_fma", 2)]
    for variant, x86 in variants:
        f = xl.XlatingFilter(D, taps, fc, fs, max_input)
        if x86:
            f.set_optimized_x86(x86)
        o = Oracle(D, taps, fc, fs, max_input, renorm=x86 is None, fma_step=x86 == 2)
        for k, n in enumerate(calls):
            x = signal(fmt, 4100 + k, n)
            got = f.process("native" if variant == "native" else "optimized", fmt, "cf32", x)
            want = o.process(fmt, x)
            assert got.shape == want.shape, (name, variant, k, got.shape, want.shape)
            if variant == "native":
                assert bits_equal(got, want), (name, k, rel_err(got, want))
            else:
                assert rel_err(got, want) <= REL_TOL, (name, variant, k, rel_err(got, want))
        f.close()
        o.close()
    if fmt != "cf32":  # the Q15 family: exact integers
        f = xl.XlatingFilter(D, taps, fc, fs, max_input)
        o = Oracle(D, taps, fc, fs, max_input)
        for k, n in enumerate(calls):
            x = signal(fmt, 4200 + k, n)
            got, want = f.process("native", fmt, "cs16", x), o.process(fmt, x, "cs16")
            assert got.shape == want.shape and np.array_equal(got, want), (name, k)
        f.close()
        o.close()


def _run_batch(eng, ids, x, G, variant):
    if G == 1:
        eng.process_host(x, variant)
    else:
        eng.process_host_group(x, G, variant)
    eng.fetch()
    return {c: (eng.output_cs16(c) if variant == "q15" else eng.output(c)).copy() for c in ids}


def _check(variant, got, want, what):
    if variant == "native":
        assert bits_equal(got, want), (what, rel_err(got, want))
    elif variant == "q15":
        assert got.shape == want.shape and np.array_equal(got, want), what
    else:
        assert got.shape == want.shape and rel_err(got, want) <= REL_TOL, (what, rel_err(got, want))


def test_batch_default_engine_wide_beside_narrow():
    """2.016 Msps cu8: 256 clients at D = 42 and 8 at D = 1120 (the 1.8 kHz row, refused by the LDS rule before), one- and eight-block
    calls in every mode.  Each wide client against the oracle per block; each D = 42 client bit-identical to an engine without the
    wide clients."""
    fs, n = 2016000, 262144
    t42, t1120 = lpf(fs, 48000), lpf(fs, 1800)
    assert len(t1120) == 13491
    fc42 = [-900000 + 7000 * c for c in range(256)]
    fcw = [-700000 + 170000 * c for c in range(8)]
    for G in (1, 8):
        for variant in ("native", "optimized", "q15"):
            eng = xl.BatchEngine(fs, "cu8", n, group_blocks=G)
            ref = xl.BatchEngine(fs, "cu8", n, group_blocks=G)
            ids = [eng.add_client(42, t42, fc) for fc in fc42]
            rids = [ref.add_client(42, t42, fc) for fc in fc42]
            wids = [eng.add_client(1120, t1120, fc) for fc in fcw]
            assert "wide: 8 clients" in eng.describe(), eng.describe()
            assert "wide" not in ref.describe()
            ors = {c: Oracle(1120, t1120, fc, fs, n) for c, fc in zip(wids, fcw)}
            for k in range(2):
                x = siggen.xs_u8(5100 + 10 * G + k, G * n)
                got = _run_batch(eng, ids + wids, x, G, variant)
                base = _run_batch(ref, rids, x, G, variant)
                for a, b in zip(ids, rids):
                    assert bits_equal(got[a], base[b]), (G, variant, k, a)
                for c, o in ors.items():
                    want = [o.process("cu8", bl, "cs16" if variant == "q15" else "cf32") for bl in np.split(x, G)]
                    want = np.concatenate(want)
                    _check(variant, got[c], want, (G, variant, k, c))
            eng.close()
            ref.close()
            for o in ors.values():
                o.close()


def test_batch_max_window_wide_history():
    """20 Msps cs8 with max_window = 32768: the 12.5 kHz and 10 kHz rows (T - 1 + D > 16384), a client that joins after five calls
    (zero history), remove and re-add, eight-block calls; a default engine still refuses the shape; the option is an admission
    setting (-EBUSY with clients)."""
    fs, n, G = 20000000, 262144, 8
    t125, t10 = lpf(fs, 12500), lpf(fs, 10000)
    assert len(t125) - 1 + 1600 > 16384 and len(t10) - 1 + 2000 > 16384
    dflt = xl.BatchEngine(fs, "cs8", n)
    with pytest.raises(xl.XlatingError) as e:
        dflt.add_client(1600, t125, 0)
    assert e.value.code == -22
    dflt.close()

    eng = xl.BatchEngine(fs, "cs8", n, group_blocks=G)
    eng.set_option("max_window", 32768)
    a = eng.add_client(1600, t125, 2500000)
    b = eng.add_client(2000, t10, -3100000)
    with pytest.raises(xl.XlatingError) as e:
        eng.set_option("max_window", 65536)
    assert e.value.code == -16
    ors = {a: Oracle(1600, t125, 2500000, fs, n), b: Oracle(2000, t10, -3100000, fs, n)}
    late = None
    for k in range(9):
        if k == 5:  # joins mid-stream: its windows reach below its join point
            late = eng.add_client(2000, t10, 700000)
            ors[late] = Oracle(2000, t10, 700000, fs, n)
        if k == 7:  # remove and re-add (the id may be recycled: a fresh filter)
            eng.remove_client(a)
            ors.pop(a).close()
            a = eng.add_client(1600, t125, -1500000)
            ors[a] = Oracle(1600, t125, -1500000, fs, n)
        x = signal("cs8", 6100 + k, G * n)
        variant = "native" if k % 2 == 0 else "optimized"
        got = _run_batch(eng, list(ors), x, G, variant)
        for c, o in ors.items():
            want = np.concatenate([o.process("cs8", bl) for bl in np.split(x, G)])
            _check(variant, got[c], want, (k, c, variant))
    assert "window<=32768" in eng.describe(), eng.describe()
    eng.close()
    for o in ors.values():
        o.close()


_FORCED = r"""
import sys, numpy as np
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import siggen, sdr_server_amd as xl
out = {}
for D, T in ((42, 505), (100, 301)):
    taps = siggen.hamming_sinc(T, 0.4 / D)
    for variant in ("native", "optimized"):
        f = xl.XlatingFilter(D, taps, -77777, 2016000, 262144)
        for k, n in enumerate((262144, 50002, 262144)):
            out["d_%%d_%%s_%%d" %% (D, variant, k)] = f.process(variant, "cu8", "cf32", siggen.xs_u8(7100 + k, n))
        f.close()
        e = xl.BatchEngine(2016000, "cu8", 262144, group_blocks=2)
        ids = [e.add_client(D, taps, -900000 + 37000 * c) for c in range(5)]
        for k in range(2):
            e.process_host_group(siggen.xs_u8(7200 + k, 2 * 262144), 2, variant)
            e.fetch()
            for c in ids:
                out["b_%%d_%%s_%%d_%%d" %% (D, variant, k, c)] = e.output(c)
        out["plan_%%d_%%s" %% (D, variant)] = np.frombuffer(e.describe().encode(), np.uint8)
        e.close()
np.savez(sys.argv[1], **out)
"""


def test_forced_wide_path_matches_direct_kernel(tmp_path):
    """XL_TESTING=1 XL_EXP_WIDE=1 sends ordinary shapes through the wide kernel: native outputs bit-identical to xl_fir_kernel's,
    optimized within 1e-5 (drop-in and batch)."""
    code = _FORCED % {"root": ROOT, "tests": os.path.join(ROOT, "tests")}
    base = {k: v for k, v in os.environ.items() if not k.startswith("XL_")}
    res = {}
    for tag, extra in (("direct", {}), ("wide", {"XL_TESTING": "1", "XL_EXP_WIDE": "1"})):
        p = str(tmp_path / (tag + ".npz"))
        r = subprocess.run([sys.executable, "-c", code, p], env=dict(base, **extra), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        res[tag] = dict(np.load(p))
    d, w = res["direct"], res["wide"]
    assert set(d) == set(w)
    for k in d:
        if k.startswith("plan_"):
            assert b"wide: 5 clients" in w[k].tobytes() and b"wide" not in d[k].tobytes(), (k, w[k].tobytes())
        elif "_native_" in k:
            assert bits_equal(w[k], d[k]), (k, rel_err(w[k], d[k]))
        else:
            assert w[k].shape == d[k].shape and rel_err(w[k], d[k]) <= REL_TOL, (k, rel_err(w[k], d[k]))


def test_wire_admits_narrow_client_on_wide_band():
    """A 16 kHz client on a 20 Msps band through the wire boundary (xlating_wire_add_client): admitted, first blocks as the oracle."""
    fs, band, n = 20000000, 433000000, 262144
    code, req = xl.wire_parse_request(xl.wire_build_request(433500000, 16000, band, 1)[2:])
    assert code == 0
    code, adm, _ = xl.wire_admit(req, fs, band, 5)
    assert code == 0 and adm.decimation == 1250
    eng = xl.BatchEngine(fs, "cs8", n)
    cid = xl.wire_add_client(eng, adm, fs)
    assert cid >= 0
    o = Oracle(1250, lpf(fs, 16000), 500000, fs, n)
    for k in range(3):
        x = signal("cs8", 8100 + k, n)
        got = _run_batch(eng, [cid], x, 1, "native")[cid]
        assert bits_equal(got, o.process("cs8", x)), k
    eng.close()
    o.close()
