"""GPU tests (-m gpu) of the direct FIR kernel, xl_fir_kernel<CT, MODE, WIDE> (csrc/xl_kernels.hip), over the case table of
tests/direct_fir_cases.py: every tall tile height (8, 9, 10, 12, forced by XL_EXP_H) with both read widths, both tap steps, both
accumulators (native: the unfused one, bit for bit; optimized with the polyphase path off: the FMA one) and every lane count (64, 32,
16, 8 outputs per wave), on ragged calls -- no block is a multiple of a decimation --, classes inside their zero history, a call that
leaves most classes without output, a grouped call whose block ends fall inside a tile's phase walk, and an empty call.
tests/test_direct_fir_cases_cpu.py asserts without a GPU that the table holds those cases and that the planner gives each its launch;
here describe() must name that launch (height, groups, " lanes<n>", " reads8"), so an ignored setting cannot shrink the coverage.

References: one pyoracle.Oracle per client, fed block by block.  Native calls are compared bit for bit, optimized calls per call to
max|d| <= 1e-5 max|y| (REL_TOL: the project's bar for the optimized variant), committed phases bit for bit.

Each test prints its worst error and the outputs it compared (pytest -s; profiles/direct_fir_matrix.txt)."""
import functools

import numpy as np
import pytest

import direct_fir_cases as dc
import sdr_server_amd as xl
from conftest import bits_equal

pytestmark = pytest.mark.gpu
REL_TOL = 1e-5
ALL_CALLS = dc.ALL_CALLS


def _phase_bits(p):
    return tuple(np.float32(v).tobytes() for v in p)


def _seed(case, H, ci):
    return 41000 + 1000 * dc.CASES.index(case) + 100 * dc.HEIGHTS.index(H) + ci


@functools.lru_cache(maxsize=None)
def _reference(case, H, which=ALL_CALLS):
    """The oracle over the calls `which` of the case, computed once for both modes: -> (fmt, [Call], [input per call],
    [{client index: ([outputs per block], phase bits)} per call])"""
    fmt, n = dc.fmt_of(case, H), dc.max_input(case, H)
    calls = [dc.calls(case, H)[i] for i in which]
    oracles = [dc.make_oracle(D, taps, fc, 2 * n) for _, D, taps, fc in dc.clients(case, H)]
    inputs, want = [], []
    for ci, c in zip(which, calls):
        x = dc.call_input(fmt, _seed(case, H, ci), c.S * c.G)
        x.setflags(write=False)
        inputs.append(x)
        rec = {}
        for idx, o in enumerate(oracles):
            blocks = [o.process(fmt, xb) for xb in np.split(x, c.G)]
            rec[idx] = (blocks, _phase_bits(o.phase))
        want.append(rec)
    for o in oracles:
        o.close()
    return fmt, calls, inputs, want


def _engine(case, H, fmt, monkeypatch, flat=False, side=None):
    monkeypatch.setenv("XL_EXP_H", str(H))
    if flat:
        monkeypatch.setenv("XL_EXP_FLATPRIO", "1")
    eng = xl.BatchEngine(dc.FS, fmt, 2 * dc.max_input(case, H), group_blocks=dc.GROUP_BLOCKS)
    eng.set_option("polyphase", 0)
    if side is not None:
        eng.set_option("nco_side_stream", side)
    return eng


def _err(got, want):
    return float(np.abs(got.astype(np.complex128) - want.astype(np.complex128)).max()) if len(want) else 0.0


def _check_call(eng, c, mode, ids, rec, tag):
    """every client of `ids` ({client index: engine id}) against its record of the call -> (worst relative error, outputs compared)"""
    worst, count = 0.0, 0
    for idx, cid in ids.items():
        blocks, phase = rec[idx]
        got = eng.output(cid)
        lens = [eng.output_len_block(cid, g) for g in range(c.G)]
        assert lens == [len(w) for w in blocks] and len(got) == sum(lens), (tag, idx, lens, [len(w) for w in blocks], len(got))
        whole = np.concatenate(blocks)
        count += len(whole)
        if mode == "native":
            assert bits_equal(got, whole), (tag, idx, _err(got, whole))
        elif len(whole):
            scale = float(np.abs(whole).max())
            assert scale > 0.0, (tag, idx)
            e = _err(got, whole) / scale
            worst = max(worst, e)
            assert e <= REL_TOL, (tag, idx, e)
        assert _phase_bits(eng.phase(cid)) == phase, (tag, idx)
    return worst, count


def _direct_text(case, H, extra=()):
    return dc.describe_direct([(c.D, c.T, c.count) for c in dc.classes(case, H)] + list(extra), H)


def _run(case, H, mode, monkeypatch, which=ALL_CALLS, flat=False, side=None):
    fmt, calls, inputs, want = _reference(case, H, which)
    eng = _engine(case, H, fmt, monkeypatch, flat=flat, side=side)
    worst, count, d = 0.0, 0, ""
    try:
        ids = {idx: eng.add_client(D, taps, fc) for idx, (_, D, taps, fc) in enumerate(dc.clients(case, H))}
        for k, (ci, c) in enumerate(zip(which, calls)):
            eng.process_host_group(inputs[k], c.G, mode)
            eng.fetch()
            if k == 0:  # the plan is the one the CPU probe expects: heights, group counts, lane and read tags
                d = eng.describe()
                assert "| direct:" + _direct_text(case, H) + " | polyphase: none" in d, (d, _direct_text(case, H))
                # ... and the tuning switch and the option reached the engine: the one-piece tap loop is named, and an engine told to
                # keep the NCO recurrence off the side stream reserves no CUs for a side kernel (the role then runs inside the launches)
                assert ("| tap loop: flat priority" in d) == flat, d
                if side == 0:
                    assert "side kernel" not in d, d
            w, n = _check_call(eng, c, mode, ids, want[k], (case, H, mode, ci))
            worst, count = max(worst, w), count + n
    finally:
        eng.close()
    print("direct_fir %-10s h%-2d %-9s %s%s%s calls %s worst %.3g outputs %d" % (
        case, H, mode, fmt, " flat" if flat else "", " side-kernel" if "side kernel" in d else "", "".join(str(i + 1) for i in which),
        worst, count))
    return worst, count


@pytest.mark.parametrize("mode", ["native", "optimized"])
@pytest.mark.parametrize("H", dc.HEIGHTS)
@pytest.mark.parametrize("case", dc.CASES)
def test_matrix(case, H, mode, monkeypatch):
    """All seven calls, every client, every call; phases bit for bit after every call (so also at the end)."""
    _, count = _run(case, H, mode, monkeypatch)
    assert count > 0


@pytest.mark.parametrize("H", dc.HEIGHTS)
@pytest.mark.parametrize("case", dc.SPARSE_CASES)
def test_sparse_block_is_exact_in_optimized_mode(case, H, monkeypatch):
    """Every client of a tall class at fc = 0, distinct taps; one optimized call whose block holds impulses (powers of two in both
    parts) spaced more than the largest T apart.  Every window then holds at most one non-zero sample: each FMA sum has a single
    non-zero term, the rounded product the unfused path forms, and at fc = 0 the phase is exactly (1, 0), so the FMA rotate returns
    its operand.  The outputs must EQUAL the oracle's (np.array_equal: a signed zero may differ; no tolerance).  Client j of a tile has
    taps no other client has: a tap or an output that lands on a neighbour fails here whatever its size.
    tests/test_direct_fir_cases_cpu.py checks the single-term property on the CPU.  (The format rotates over cs8, cs16, cf32: cu8 has
    no sample that is exactly zero.)  The clients of the small classes keep their centre frequencies: held to REL_TOL."""
    fmt, x = dc.sparse_input(case, H)
    n = dc.max_input(case, H)
    clients = dc.clients(case, H, tall_fc0=True)
    eng = _engine(case, H, fmt, monkeypatch)
    exact = count = 0
    try:
        ids = [eng.add_client(D, taps, fc) for _, D, taps, fc in clients]
        eng.process_host(x, "optimized")
        eng.fetch()
        d = eng.describe()
        assert "| direct:" + _direct_text(case, H) + " | polyphase: none" in d, d
        for cid, (k, D, taps, fc) in zip(ids, clients):
            o = dc.make_oracle(D, taps, fc, 2 * n)
            want, got = o.process(fmt, x), eng.output(cid)
            assert got.shape == want.shape and len(want) > 0 and np.count_nonzero(want) > 0, (case, H, k, cid)
            if fc == 0:
                assert np.array_equal(got, want), (case, H, k, cid, _err(got, want), np.nonzero(got != want)[0][:8])
                exact += 1
                count += len(want)
            else:
                assert _err(got, want) <= REL_TOL * float(np.abs(want).max()), (case, H, k, cid)
            assert _phase_bits(eng.phase(cid)) == _phase_bits(o.phase), (case, H, k, cid)
            o.close()
    finally:
        eng.close()
    assert exact == sum(c.count for c in dc.classes(case, H) if c.count >= 8)
    print("direct_fir %-10s h%-2d sparse    %s exact clients %d outputs %d" % (case, H, fmt, exact, count))


@pytest.mark.parametrize("H", [9, 12])
def test_tall_class_joins_mid_stream(H, monkeypatch):
    """Case even, native.  Behind call 2, H + 2 further (42, 505) clients join at once: a class of their own (another grid than the
    old class's, whose stream position is no multiple of 42; no history: a tall tile with zero_below masking), each compared with a
    fresh oracle from its join point through calls 3 to 7 -- in call 3 they own a fraction of their first window, during the grouped
    call 4 they mature -- and through two more full calls."""
    case = "even"
    fmt, n = dc.fmt_of(case, H), dc.max_input(case, H)
    seq = [(c, dc.call_input(fmt, _seed(case, H, ci), c.S * c.G)) for ci, c in enumerate(dc.calls(case, H))]
    seq += [(dc.Call(n, 1), dc.call_input(fmt, _seed(case, H, 50 + extra), n)) for extra in range(2)]
    joiners = [(42, dc.taps_of(505, j, H + 2, 42) * np.float32(0.5), -300000 + 41003 * j) for j in range(H + 2)]
    eng = _engine(case, H, fmt, monkeypatch)
    olds, news = {}, {}
    count = 0
    try:
        ids, jids = {}, {}
        for idx, (_, D, taps, fc) in enumerate(dc.clients(case, H)):
            ids[idx], olds[idx] = eng.add_client(D, taps, fc), dc.make_oracle(D, taps, fc, 2 * n)
        for k, (c, x) in enumerate(seq):
            if k == 2:
                for j, (D, taps, fc) in enumerate(joiners):
                    jids[j], news[j] = eng.add_client(D, taps, fc), dc.make_oracle(D, taps, fc, 2 * n)
            eng.process_host_group(x, c.G, "native")
            eng.fetch()
            if k == 2:
                d = eng.describe()
                assert "| direct:" + _direct_text(case, H, [(42, 505, H + 2)]) + " | polyphase: none" in d, d
                assert (" h%d x 3 groups" % H) in d, d
            for who, oracles in ((ids, olds), (jids, news)):
                rec = {}
                for i, o in oracles.items():
                    blocks = [o.process(fmt, xb) for xb in np.split(x, c.G)]
                    rec[i] = (blocks, _phase_bits(o.phase))
                count += _check_call(eng, c, "native", who, rec, ("join", H, k, who is jids))[1]
    finally:
        eng.close()
        for o in list(olds.values()) + list(news.values()):
            o.close()
    print("direct_fir even       h%-2d join      %s outputs %d" % (H, fmt, count))


@pytest.mark.parametrize("mode", ["native", "optimized"])
@pytest.mark.parametrize("H", [8, 10])
@pytest.mark.parametrize("case", dc.FLAT_CASES)
def test_flat_priority_loop(case, H, mode, monkeypatch):
    """XL_EXP_FLATPRIO=1: the tap loop in one piece (a.flags & 2), which launches of more than two rounds of workgroups take; the
    matrix's assertions over calls 1, 2 and 4."""
    _, count = _run(case, H, mode, monkeypatch, which=dc.FLAT_CALLS, flat=True)
    assert count > 0


@pytest.mark.parametrize("H", [9, 12])
def test_role_inside_the_tall_launch(H, monkeypatch):
    """nco_side_stream = 0: the tall launch (the first one with groups) carries the NCO role -- its FIR workgroups are shifted by
    nco_blocks, or the role rides in the spare waves.  Native, calls 1, 2, 4 and 5, bit for bit; phases bit for bit."""
    _, count = _run(dc.ROLE_CASE, H, "native", monkeypatch, which=dc.ROLE_CALLS, side=0)
    assert count > 0
