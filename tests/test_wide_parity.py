"""GPU tests (-m gpu) of the wide direct FIR (sdr-server_amd/csrc/xl_wide.hip) at its admission edges and beside every launch it shares a
call with: every input format and mode of the batch engine, ragged and short calls, the exact edges of the admission rules, a mixed wide
population in one launch, a soak beside the config-5 polyphase plan, and the other entry points (device pointers, xlating_multi, sinks).
Every wide client against the oracle: native BIT-EXACT, optimized and the x86 flavours max|d| / max|y| <= 1e-5 per call (per block for
grouped calls), Q15 exact integers, committed phases bit for bit.
The optimized variants are measured against the oracle with float64 accumulation (its sum_mode 1, same float32 NCO): with thousands of
taps and a block of one or two outputs, the reference's own float32 running sum is off by up to 3e-5 of max|y| (D = 65536, T = 983041),
so it cannot be the yardstick of another summation order at 1e-5.  Shapes with D > T stream only calls of whole multiples of D: the
reference's history count underflows at any other call end (xlating.c:76)."""
import numpy as np
import pytest

import siggen
import sdr_server_amd as xl
from pyoracle import Oracle, population
from test_wide_shapes import _check, _run_batch, bits_equal, lpf, rel_err, signal

pytestmark = pytest.mark.gpu

FS10, FS20 = 10000000, 20000000


def taps_of(T, D):
    """an explicit low-pass prototype of T taps for decimation D (T = 1: a single unit tap)"""
    return np.ones(1, np.float32) if T == 1 else siggen.hamming_sinc(T, 0.4 / D)


def wide_clients_10m():
    """three clients of a 10 Msps engine on the default ring: 8 kHz (D = 1250, even, 15057 taps), an odd decimation (D = 1111, 13001
    taps: wide at the batch engine's 12-tap multiple, window 14111 <= XL_HCAP) and a narrow config-5 client (D = 100, 257 taps)"""
    t8k = lpf(FS10, 8000)
    assert len(t8k) == 15057
    return [(1250, t8k, 1234567), (1111, taps_of(13001, 1111), -2345678), (100, siggen.hamming_sinc(257, 0.004), 3000000)]


def wide_clients_20m():
    """clients of a 20 Msps engine with max_window = 32768: 10 kHz (D = 2000, 24091 taps: window 26090 > XL_HCAP), 16 kHz (D = 1250,
    15057 taps) and a narrow one (D = 100, 257 taps)"""
    t10k = lpf(FS20, 10000)
    assert len(t10k) == 24091
    return [(2000, t10k, -3100000), (1250, lpf(FS20, 16000), 2500000), (100, siggen.hamming_sinc(257, 0.004), 700000)]


class Ref:
    """one client's oracles on the same stream: the reference's float32 arithmetic (native: bit for bit; Q15) and float64
    accumulation (the yardstick of the optimized variants)"""

    def __init__(self, D, taps, fc, fs, n, **kw):
        self.o32 = Oracle(D, taps, fc, fs, n, **kw)
        self.o64 = Oracle(D, taps, fc, fs, n, sum_mode=1, **kw)

    def process(self, fmt, x, variant="native"):
        out = "cs16" if variant == "q15" else "cf32"
        a, b = self.o32.process(fmt, x, out), self.o64.process(fmt, x, out)
        return a if variant in ("native", "q15") else b

    def set_x86(self, renorm, fma_step):
        for o in (self.o32, self.o64):
            Oracle.lib().orc_xlating_set_renorm(o.h, 1 if renorm else 0)
            Oracle.lib().orc_xlating_set_fma_step(o.h, 1 if fma_step else 0)

    @property
    def phase(self):
        assert self.o32.phase == self.o64.phase
        return self.o32.phase

    def close(self):
        self.o32.close()
        self.o64.close()


def engine(fs, fmt, n, clients, G=1, max_window=0, renorm=True, fma_step=False):
    eng = xl.BatchEngine(fs, fmt, n, group_blocks=G)
    if max_window:
        eng.set_option("max_window", max_window)
    ors = {}
    for D, t, fc in clients:
        ors[eng.add_client(D, t, fc)] = Ref(D, t, fc, fs, n, renorm=renorm, fma_step=fma_step)
    return eng, ors


def call_and_check(eng, ors, fmt, x, G, variant, what=()):
    """one call of G blocks (x: G equal blocks back to back) -> every client against its oracle, PER BLOCK"""
    got = _run_batch(eng, list(ors), x, G, variant)
    for c, o in ors.items():
        want = [o.process(fmt, bl, variant) for bl in np.split(x, G)]
        assert [eng.output_len_block(c, g) for g in range(G)] == [len(w) for w in want], (what, c)
        off = 0
        for g, w in enumerate(want):
            _check(variant, got[c][off:off + len(w)], w, what + (c, g))
            off += len(w)
        assert off == len(got[c]), (what, c)


def assert_phases(eng, ors, what=()):
    for c, o in ors.items():
        got, want = eng.phase(c), o.phase
        assert tuple(np.float32(v).tobytes() for v in got) == tuple(np.float32(v).tobytes() for v in want), (what, c, got, want)


def close(eng, ors):
    eng.close()
    for o in ors.values():
        o.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. Formats x modes on the batch engine

@pytest.mark.parametrize("fmt", ["cu8", "cs8", "cs16", "cf32"])
def test_batch_wide_every_format_and_mode(fmt):
    """xl_batch.cpp xl_batch_wide_launch -> xl_wide.hip xl_wide_kernel (native / optimized) and xl_wide_q15_kernel (Q15) per input
    format: two wide clients (even and odd D) and a narrow one in one engine, calls of 8 and 1 blocks in turn, every client against the
    oracle per block; committed phases bit for bit at the end."""
    n = 65536
    variants = ["native", "optimized"] + (["q15"] if fmt != "cf32" else [])
    for variant in variants:
        eng, ors = engine(FS10, fmt, n, wide_clients_10m(), G=8)
        assert "wide: 2 clients" in eng.describe(), eng.describe()
        for k, G in enumerate((8, 1, 8, 1, 8)):
            call_and_check(eng, ors, fmt, signal(fmt, 6300 + 10 * k + G, G * n), G, variant, (fmt, variant, k))
        if variant != "q15":
            assert_phases(eng, ors, (fmt, variant))
        close(eng, ors)


@pytest.mark.parametrize("flavour", ["optimized_x86", "optimized_x86_fma"])
@pytest.mark.parametrize("fmt", ["cu8", "cs8", "cs16", "cf32"])
def test_batch_wide_x86_modes_drift_and_renormalising_call(fmt, flavour):
    """XL_MODE_OPTIMIZED_X86 / _X86_FMA with wide clients: the wide launch's phases (xl_wide.hip xl_wide_phase) must follow the flags that
    xl_batch.cpp xl_call_begin puts into pos.pad (XL_POS_NORENORM / XL_POS_FMA_STEP).  53 blocks in calls of 8 and 1, the phase never
    renormalised, against Oracle(renorm=False, fma_step=...); a renormalising native call in between (bit-exact); phases bit for bit."""
    n = 65536
    fma = flavour.endswith("fma")
    eng, ors = engine(FS10, fmt, n, wide_clients_10m(), G=8, renorm=False, fma_step=fma)
    for k, G in enumerate((8, 1, 8, 1, 8, 1, 8, 1, None, 8, 1, 8)):
        if G is None:  # the reference's native call renormalises once and steps without FMA
            for o in ors.values():
                o.set_x86(True, False)
            call_and_check(eng, ors, fmt, signal(fmt, 6500 + k, n), 1, "native", (fmt, flavour, k))
            for o in ors.values():
                o.set_x86(False, fma)
            continue
        call_and_check(eng, ors, fmt, signal(fmt, 6500 + k, G * n), G, flavour, (fmt, flavour, k))
    # (the unrenormalised recurrence has drifted off the unit circle: the check below is not vacuous)
    assert any(abs(float(np.hypot(*o.phase)) - 1.0) > 1e-7 for o in ors.values())
    assert_phases(eng, ors, (fmt, flavour))
    close(eng, ors)


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. Block geometry

RAGGED = [262144, 262144, 100002, 2000, 262144, 18000, 8, 262144, 262144, 100002, 3400, 262144]
FETCH = {1, 2, 3, 5, 6, 8, 10, 11}


def _geometry(shape):
    if shape == "20m_max_window":
        return FS20, "cs8", 32768, wide_clients_20m(), (2000, lpf(FS20, 10000), 4100000)
    return FS10, "cs16", 0, wide_clients_10m(), (1250, lpf(FS10, 8000), -4200000)


@pytest.mark.parametrize("variant", ["native", "optimized"])
@pytest.mark.parametrize("shape", ["20m_max_window", "10m_default_ring"])
def test_batch_wide_ragged_device_blocks_late_fetch(shape, variant):
    """xl_batch.cpp look-ahead in xl_call_table (the next call's phase table tabulated for the previous call's length), xl_grid.h
    xl_grid_dyn_cap and xl_wide.hip xl_wide_load4 on single blocks of ragged lengths -- full, 100002, below D, below T, 8 bytes -- fed
    as device buffers on the caller's (torch) stream, fetched only now and then; a wide client joins mid-stream."""
    import torch

    fs, fmt, mw, clients, late = _geometry(shape)
    eng, ors = engine(fs, fmt, 262144, clients, max_window=mw)
    dt = torch.int8 if fmt == "cs8" else torch.int16
    recv = [torch.empty(262144, dtype=dt, device="cuda") for _ in range(2)]
    stream = torch.cuda.current_stream().cuda_stream
    for k, n in enumerate(RAGGED):
        if k == 4:
            ors[eng.add_client(*late)] = Ref(*late, fs, 262144)
        x = signal(fmt, 6700 + k, n)
        buf = recv[k % 2]
        buf[:n].copy_(torch.from_numpy(x))
        eng.process_device(buf.data_ptr(), n, variant, stream)
        want = {c: o.process(fmt, x, variant) for c, o in ors.items()}
        if k in FETCH:
            eng.fetch()
            for c in ors:
                _check(variant, eng.output(c), want[c], (shape, variant, k, c))
    assert "wide: 3 clients" in eng.describe(), eng.describe()
    close(eng, ors)


@pytest.mark.parametrize("shape", ["20m_max_window", "10m_default_ring"])
def test_batch_wide_windows_span_many_short_calls(shape):
    """xl_grid.h xl_grid_dyn_cap / xl_wide.hip zero_below masking: 40 single blocks of 600 .. 1500 samples (mostly below every wide
    client's D, all far below its T), so that each window is assembled from the ring and many earlier calls and most calls give a
    client no output; native and optimized calls in turn, every call against the oracle."""
    fs, fmt, mw, clients, _ = _geometry(shape)
    eng, ors = engine(fs, fmt, 262144, clients, max_window=mw)
    for k in range(40):
        n = 2 * (600 + (k * 389) % 901)
        call_and_check(eng, ors, fmt, signal(fmt, 6900 + k, n), 1, "optimized" if k % 3 == 2 else "native", (shape, k))
    assert_phases(eng, ors, shape)
    close(eng, ors)


@pytest.mark.parametrize("D", [1250, 1251])
def test_dropin_wide_history_over_many_short_calls(D):
    """xl_filter.cpp xl_run_cf32 -> xl_wide.hip (explicit dyn1): 40 cf32 calls of 397 .. 607 samples with 15057 taps, so that most calls
    produce no output and the work image's history builds up over many calls past a whole window; an even D (16-byte V16 loads) and an
    odd D (scalar loads), call lengths that end mid-window (the end-of-call fallback of xl_wide_load4).  Native bit-exact, optimized
    <= 1e-5 per call."""
    t = lpf(FS10, 8000)
    for variant in ("native", "optimized"):
        f = xl.XlatingFilter(D, t, 1234567, FS10, 4096)
        o = Ref(D, t, 1234567, FS10, 4096)
        produced = 0
        for k in range(40):
            x = signal("cf32", 7100 + k, 2 * (397 + (k * 131) % 211))
            got, want = f.process(variant, "cf32", "cf32", x), o.process("cf32", x, variant)
            _check(variant, got, want, (D, variant, k))
            produced += len(want)
        assert 0 < produced < 20
        f.close()
        o.close()


def test_batch_wide_device_group_equals_host_group():
    """xl_batch.cpp xlating_batch_process_device_group (xl_batch_wide_launch reads the caller's blocks in place: in1 = d_blocks) against
    xlating_batch_process_host_group: bit for bit, grouped calls of 4, 2 and 4 ragged blocks in native and optimized mode, max_window
    ring; the host path against the oracle."""
    import torch

    n = 65536
    e1, ors = engine(FS20, "cs8", n, wide_clients_20m(), G=4, max_window=32768)
    e2, _ = engine(FS20, "cs8", n, wide_clients_20m(), G=4, max_window=32768)
    stream = torch.cuda.current_stream().cuda_stream
    for k, (G, m, variant) in enumerate(((4, n, "native"), (2, n, "optimized"), (4, 50002, "native"), (4, n, "optimized"))):
        x = signal("cs8", 7300 + k, G * m)
        call_and_check(e1, ors, "cs8", x, G, variant, (k,))
        d = torch.from_numpy(x).cuda()
        e2.process_device_group(d.data_ptr(), m, G, variant, stream)
        e2.fetch()
        for c in ors:
            assert bits_equal(e2.output(c), e1.output(c)), (k, c)
    close(e1, ors)
    e2.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. Admission edges

def _short_calls(eng, ors, fmt):
    for k, (n, variant) in enumerate(((8192, "native"), (3002, "optimized"), (8192, "native"))):
        call_and_check(eng, ors, fmt, signal(fmt, 7500 + k, n), 1, variant, (k,))


def test_admission_edge_window_16384_and_max_window():
    """xl_batch.cpp xlating_batch_add_client at T - 1 + D = XL_HCAP: D = 1, T = 16384 is admitted on a default engine and stays on the
    direct kernel; T = 16385 is refused (-EINVAL) there, admitted with max_window = 16385 and then wide; max_window = 16384 + 100 refuses
    windows of 16485 (D = 1 and D = 101) and admits 16484.  Every admitted shape against the oracle."""
    fs = 2016000
    eng, ors = engine(fs, "cu8", 8192, [(1, taps_of(16384, 1), 12345)])
    assert "wide" not in eng.describe(), eng.describe()
    with pytest.raises(xl.XlatingError) as e:
        eng.add_client(1, taps_of(16385, 1), 0)
    assert e.value.code == -22
    _short_calls(eng, ors, "cu8")
    close(eng, ors)

    eng, ors = engine(fs, "cu8", 8192, [(1, taps_of(16385, 1), -23456)], max_window=16385)
    d = eng.describe()
    assert "wide: 1 clients" in d and "window<=16385" in d, d
    _short_calls(eng, ors, "cu8")
    close(eng, ors)

    eng = xl.BatchEngine(fs, "cu8", 8192)
    eng.set_option("max_window", 16484)
    for D, T in ((1, 16485), (101, 16385)):
        with pytest.raises(xl.XlatingError) as e:
            eng.add_client(D, taps_of(T, D), 0)
        assert e.value.code == -22, (D, T)
    ors = {eng.add_client(100, taps_of(16385, 100), 34567): Ref(100, taps_of(16385, 100), 34567, fs, 8192)}
    assert "wide: 1 clients" in eng.describe()
    _short_calls(eng, ors, "cu8")
    close(eng, ors)


def test_admission_edge_max_window_1048576():
    """option max_window at its largest value (1 << 20; one more is -EINVAL) with a client whose window is exactly that long (D = 65536,
    T = 983041, cs8; T = 983042 is refused): xl_wide.hip reads the window across the max_window ring (xl_batch.cpp d_whist) and the
    call's blocks.  Grouped and single calls of two outputs per block until the windows lie wholly in the stream, every output against
    the oracle -- native calls only: no float32 accumulation holds 1e-5 of max|y| over a million taps (measured here: the reference's
    own sum 3e-5 off the float64 one on noise, 4e-4 on an in-band tone; the optimized kernel 1.06e-5 on noise), while the native kernel
    must reproduce the reference's sum bit for bit whatever T is.  The optimized arithmetic reads the same ring through the same
    xl_wide_load4 at T <= 30001 in the tests above and below."""
    n = 262144
    t = taps_of(983041, 65536)
    eng = xl.BatchEngine(FS20, "cs8", n, group_blocks=8)
    with pytest.raises(xl.XlatingError) as e:
        eng.set_option("max_window", (1 << 20) + 1)
    assert e.value.code == -22
    eng.set_option("max_window", 1 << 20)
    with pytest.raises(xl.XlatingError) as e:
        eng.add_client(65536, np.concatenate([t, t[:1]]), 0)
    assert e.value.code == -22
    ors = {eng.add_client(65536, t, 1777777): Ref(65536, t, 1777777, FS20, n)}
    d = eng.describe()
    assert "wide: 1 clients" in d and "window<=1048576" in d, d
    for k, G in enumerate((8, 8, 1, 8, 1)):
        call_and_check(eng, ors, "cs8", signal("cs8", 7700 + k, G * n), G, "native", (k,))
    assert_phases(eng, ors)
    close(eng, ors)


@pytest.mark.parametrize("T", [13476, 13477, 13480, 13481])
def test_admission_edge_tap_multiples_4_and_12(T):
    """D = 1000: the batch engine (xl_wide.h xl_fir_needs_wide at 12 taps) sends T = 13477 on to the wide kernel and keeps 13476 on
    xl_fir_kernel; the drop-in (xl_filter.cpp, 4 taps) keeps T <= 13480 on xl_fir_kernel with its LDS exactly full at 8 outputs per
    wave and sends 13481 wide.  Both boundaries against the oracle on each side of both edges."""
    fs, n, fc = 2016000, 131072, -77777
    t = taps_of(T, 1000)
    eng, ors = engine(fs, "cu8", n, [(1000, t, fc)])
    d = eng.describe()
    assert ("wide: 1 clients" in d) == (T >= 13477) and ("wide" in d) == (T >= 13477), d
    for k, (m, variant) in enumerate(((n, "native"), (50002, "optimized"), (n, "native"), (n, "optimized"))):
        call_and_check(eng, ors, "cu8", siggen.xs_u8(7900 + k, m), 1, variant, (T, k))
    close(eng, ors)
    for variant in ("native", "optimized"):
        f = xl.XlatingFilter(1000, t, fc, fs, n)
        o = Ref(1000, t, fc, fs, n)
        for k, m in enumerate((n, 50002, 0, n)):
            x = siggen.xs_u8(8000 + k, m)
            _check(variant, f.process(variant, "cu8", "cf32", x), o.process("cu8", x, variant), (T, variant, k))
        f.close()
        o.close()


def test_grouped_call_shorter_than_wide_decimation_is_refused():
    """xl_batch.cpp xl_call_begin: a call of G >= 2 blocks needs blocks of at least the largest decimation (plan_maxD, the wide clients'
    included; xl_grid.h xl_bnd_next needs S >= D) -- G = 4 blocks of 1500 samples next to a D = 2000 wide client return -EINVAL, also
    right after a client joined (the plan is rebuilt inside the refused call), and leave every stream intact: the next calls match the
    oracle, a single block of 1500 samples is accepted, phases bit for bit at the end."""
    n = 8192
    clients = [(2000, taps_of(14001, 2000), 3300000), (42, taps_of(505, 42), -1500000)]
    eng, ors = engine(FS20, "cs8", n, clients, G=4)
    assert "wide: 1 clients" in eng.describe(), eng.describe()
    call_and_check(eng, ors, "cs8", signal("cs8", 8100, 4 * n), 4, "native", (0,))
    with pytest.raises(xl.XlatingError) as e:
        eng.process_host_group(signal("cs8", 8101, 4 * 3000), 4, "native")
    assert e.value.code == -22
    ors[eng.add_client(2000, taps_of(14001, 2000), -700000)] = Ref(2000, taps_of(14001, 2000), -700000, FS20, n)
    with pytest.raises(xl.XlatingError) as e:
        eng.process_host_group(signal("cs8", 8102, 4 * 3000), 4, "optimized")
    assert e.value.code == -22
    call_and_check(eng, ors, "cs8", signal("cs8", 8103, 4 * n), 4, "optimized", (1,))
    call_and_check(eng, ors, "cs8", signal("cs8", 8104, 3000), 1, "native", (2,))
    call_and_check(eng, ors, "cs8", signal("cs8", 8105, 2 * n), 2, "native", (3,))
    assert_phases(eng, ors)
    close(eng, ors)


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. A mixed wide population in one launch

def test_batch_mixed_wide_population_one_launch():
    """xl_wide.hip xl_wide_kernel with 31 wide clients of 13 shapes in one launch: `parts` from the largest Tpad of all
    (xl_batch.cpp xl_batch_wide_launch), xtiles from the most outputs of any client (xl_batch_wide_maxk) -- short-T clients (D = 2926,
    T = 1 .. 57: wide at any T) split as finely as T = 30001, clients with no output in calls where others have some.  Midway the client
    with the largest Tpad leaves and a fresh one of the same shape joins.  Every client, every call, per block; every block a whole
    number of D = 2926 periods (D > T: see the module's docstring)."""
    shapes = [(2926, 1, 2), (2926, 2, 1), (2926, 3, 1), (2926, 5, 2), (2926, 57, 2), (2000, 24091, 3), (1600, 19273, 3),
              (1250, 15057, 4), (1111, 13001, 3), (1500, 16001, 3), (4000, 20000, 2), (2500, 30001, 1), (1077, 15361, 4)]
    server = {24091: lpf(FS20, 10000), 19273: lpf(FS20, 12500), 15057: lpf(FS20, 16000)}
    clients, largest = [], None
    for j, (D, T, cnt) in enumerate(shapes):
        t = server[T] if T in server else taps_of(T, D)
        assert len(t) == T
        for i in range(cnt):
            clients.append((D, t, -9000000 + 570000 * len(clients) + 1111 * j))
            if T == 30001:
                largest = len(clients) - 1
    n = 262144
    eng, ors = engine(FS20, "cs8", n, clients, G=4, max_window=32768)
    ids = list(ors)
    assert "wide: %d clients" % len(clients) in eng.describe(), eng.describe()
    # (blocks of 2926 u samples: u = 1 gives the D = 4000 clients no output in some calls; G = 4 needs blocks >= the largest D)
    calls = [(1, 44, "native"), (4, 2, "optimized"), (1, 1, "native"), (1, 2, "optimized"), (4, 11, "native"), (1, 44, "optimized"),
             (4, 2, "native"), (1, 17, "optimized"), (4, 11, "optimized"), (1, 1, "native"), (1, 44, "native")]
    for k, (G, u, variant) in enumerate(calls):
        if k == 4:
            eng.remove_client(ids[largest])
            ors.pop(ids[largest]).close()
        if k == 5:
            D, t, fc = clients[largest]
            ors[eng.add_client(D, t, fc + 3)] = Ref(D, t, fc + 3, FS20, n)
        call_and_check(eng, ors, "cs8", signal("cs8", 8300 + k, G * 2 * 2926 * u), G, variant, (k,))
    assert_phases(eng, ors)
    close(eng, ors)


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. Soak beside config 5

def _soak_engine(side, c5, wide):
    eng = xl.BatchEngine(FS10, "cf32", 262144, group_blocks=8)
    if side is not None:
        eng.set_option("nco_side_stream", side)
    ids = [eng.add_client(D, t, fc) for D, t, fc in c5 + wide]
    return eng, ids


def test_soak_wide_beside_config5_polyphase_plan():
    """1024 config-5 clients (cf32 10 Msps, D = 100, 257 taps: the two-half wide mix xl_mixh2.hip, M = 64, no CUs reserved for the side
    stream) and 16 wide 8 kHz clients in one engine: the wide launch (xl_batch.cpp xl_batch_wide_launch, behind the polyphase launches)
    reads the phase table that the side-stream chain kernel (xl_kernels.hip xl_nco_chain_kernel) rolls.  200 one-block optimized calls,
    then six 8-block calls and a last one-block call, the host running ahead (a fetch every 7th call only).  Every 50 calls all 1040
    committed phases bit for bit against oracles fast-forwarded with skip_calls; a second engine with nco_side_stream = 0 (the scalar
    role steps inside the launches) on the same blocks, interleaved, has the same phases bit for bit; the last call's outputs of every
    client against the oracle (population for config 5)."""
    S = 131072
    t257, t8k = siggen.hamming_sinc(257, 0.004), lpf(FS10, 8000)
    c5 = [(100, t257, -4900000 + 9570 * c) for c in range(1024)]
    wide = [(1250, t8k, -4000000 + 500000 * j + 1234) for j in range(16)]
    blocks = [(siggen.xs_s16(8500 + b, 2 * S).astype(np.float32) / np.float32(32768)).astype(np.float32) for b in range(4)]
    engs = [_soak_engine(None, c5, wide), _soak_engine(0, c5, wide)]
    phase_orc = [Oracle(D, t, fc, FS10, 2) for D, t, fc in c5 + wide]  # (skip_calls only: no buffers needed)
    stream, done = [], 0  # block index per stream block; blocks the phase oracles have been advanced over

    def check_phases(tag):
        nonlocal done
        for o in phase_orc:
            o.skip_calls(S, len(stream) - done)
        done = len(stream)
        want = np.array([o.phase for o in phase_orc], dtype=np.float32)
        got = []
        for e, ids in engs:
            e.sync()
            got.append(np.array([e.phase(i) for i in ids], dtype=np.float32))
        for j, g in enumerate(got):
            bad = np.flatnonzero((g.view(np.uint32) != want.view(np.uint32)).any(axis=1))
            assert len(bad) == 0, (tag, j, bad[:16])

    plan = [1] * 200 + [8] * 6 + [1]
    for k, G in enumerate(plan):
        idx = [(len(stream) + i) % 4 for i in range(G)]
        x = blocks[idx[0]] if G == 1 else np.concatenate([blocks[i] for i in idx])
        for e, _ in engs:
            if G == 1:
                e.process_host(x, "optimized")
            else:
                e.process_host_group(x, G, "optimized")
        stream += idx
        if k == 1:
            d = engs[0][0].describe()
            assert "polyphase: cls0 D100 T257 cols1024 " in d and "mix=mfma" in d and " V62 M64 " in d and "CUs reserved" not in d, d
            assert "wide: 16 clients" in d, d
        if k % 7 == 6:
            for e, _ in engs:
                e.fetch()
        if k % 50 == 49 or k == len(plan) - 2:
            check_phases(k)
    for e, _ in engs:
        e.fetch()
    check_phases("end")
    # the last call's outputs: fast-forward to the block before it (the warm block fills the history), then the last block
    warm, last = blocks[stream[-2]], blocks[stream[-1]]
    want5 = population(100, t257, [fc for _, _, fc in c5], FS10, 2 * S, "cf32", np.concatenate([warm, last]), 1, nwarm=1, skip_fresh=S,
                       skip_calls=len(stream) - 2, sum_mode=1)
    for e, ids in engs:
        for c in range(1024):
            got = e.output(ids[c])
            assert len(got) == len(want5[c]) and rel_err(got, want5[c]) <= 1e-5, (c, rel_err(got, want5[c]))
    for j, (D, t, fc) in enumerate(wide):
        o = Oracle(D, t, fc, FS10, 2 * S, sum_mode=1)
        o.skip_calls(S, len(stream) - 2)
        o.process("cf32", warm)
        want = o.process("cf32", last)
        o.close()
        for e, ids in engs:
            _check("optimized", e.output(ids[1024 + j]), want, ("wide", j))
    for e, _ in engs:
        e.close()
    for o in phase_orc:
        o.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. Other entry points

def test_multi_host_loopback_with_wide_clients():
    """include/xlating_multi.h on one GPU with a one-rank RCCL communicator (xl_multi.cpp xlating_multi_add_client / xlating_multi_feed:
    the broadcast path into receive buffers, then the engine's grouped call on its own stream): two wide clients and a narrow one, 4-block
    feeds from device memory, native bit-exact and optimized <= 1e-5 per block."""
    import torch

    n, G = 65536, 4
    m = xl.MultiHost(FS10, "cs16", n, group_blocks=G, rank=0, world=1, uid=xl.MultiHost.unique_id())
    eng = m.engine(0)
    ors = {}
    for g, (D, t, fc) in enumerate(wide_clients_10m()):
        ors[m.add_client(g, D, t, fc)] = Ref(D, t, fc, FS10, n)
    assert "wide: 2 clients" in eng.describe(), eng.describe()
    for k, variant in enumerate(("native", "optimized", "native")):
        x = signal("cs16", 8700 + k, G * n)
        d = torch.from_numpy(x).cuda()
        m.feed(d.data_ptr(), n, G, variant)
        m.sync()
        eng.fetch()
        for c, o in ors.items():
            want = [o.process("cs16", bl, variant) for bl in np.split(x, G)]
            got, off = eng.output(c), 0
            for g, w in enumerate(want):
                _check(variant, got[off:off + len(w)], w, (k, c, g))
                off += len(w)
            assert off == len(got)
    m.close()
    for o in ors.values():
        o.close()


def test_sinks_deliver_wide_clients_streams(tmp_path):
    """xl_sinks.cpp xlating_sinks_submit after xlating_batch_fetch with wide clients: each file holds exactly the oracle's stream (raw and
    gzip sinks), native."""
    import gzip

    n = 65536
    eng, ors = engine(FS10, "cs16", n, wide_clients_10m())
    sinks = xl.Sinks(writer_threads=2, queue_bytes=16 * 25600)
    gz = {c: (j == 1) for j, c in enumerate(ors)}
    for c in ors:
        assert sinks.attach_file(c, tmp_path, use_gzip=gz[c]) == 0
    want = {c: b"" for c in ors}
    for k, m in enumerate((n, 30002, n, n)):
        x = signal("cs16", 8900 + k, m)
        eng.process_host(x, "native")
        eng.fetch()
        assert sinks.submit(eng) == len(ors)
        for c, o in ors.items():
            want[c] += o.process("cs16", x).tobytes()
    sinks.flush()
    assert sinks.failed() == []
    for c in ors:
        assert sinks.detach(c) == 0
        path = tmp_path / (f"{c}.cf32.gz" if gz[c] else f"{c}.cf32")
        raw = gzip.open(path, "rb").read() if gz[c] else path.read_bytes()
        assert len(want[c]) > 0 and raw == want[c], c
    sinks.close()
    close(eng, ors)
