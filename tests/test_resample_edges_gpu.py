"""GPU tests (-m gpu) of the resampler banks' two window paths (xl_resample.hip, xl_resample_q15.hip): a tile whose window fits
XL_RS_LDS_SPAN is staged in LDS, a wider one is read in place, and the streams of tests/test_resample_gpu.py and
tests/test_resample_q15_gpu.py (M / L <= 3 but for one) hardly leave the first.  The streams here are tests/resample_edges.py's: a span
of exactly the limit and of one more, both paths in one launch, a path that depends on the split of the input, M % L != 0 in place,
the Q15 bank's tap table and window both in place with either accumulator, M at 2^31 - 1, a feed that produces nothing.

WHICH PATH A TILE TAKES IS NOT OBSERVED HERE: the library counts nothing of the kind, by intent.  The evidence is the restatement of
the tile arithmetic in tests/resample_edges.py, whose verdict for exactly the piece lists fed below tests/test_resample_edges_cpu.py
asserts tile by tile.

The checks are the existing ones, nothing is measured: the float bank against the float64 restatement within the derived bound
(resample_ref.check: gamma_Q S + Q 2^-126) and bit for bit between the splits; the Q15 bank bit for bit against the integer
restatement.  The helpers are the two existing files', imported."""
import functools

import numpy as np
import pytest

import resample_edges as E
import resample_q15_ref as QR
import resample_ref as RR
import sdr_server_amd as xl
import test_resample_gpu as F
import test_resample_q15_gpu as Q
from conftest import bits_equal

pytestmark = pytest.mark.gpu


def seed_of(name):
    return 900 + [c.name for c in E.CASES].index(name)


# ------------------------------------------------------------------------------------------------------------ the float bank
@functools.lru_cache(maxsize=None)
def float_input(name):
    x = F.noise(E.CASE[name].N, seed_of(name))
    x.setflags(write=False)
    return x


def float_run(case, x, pieces):
    """the case's stream alone in a bank of its own, fed x in the given pieces -> its outputs"""
    keep, addr = F.to_device(x)
    bank = xl.ResamplerBank()
    sid = bank.add(case.L, case.M, case.taps)
    y = F.feed_pieces(bank, sid, case.L, case.M, addr, pieces)
    assert y.size == RR.counts(case.L, case.M, case.N) == bank.produced(sid)
    bank.close()
    y.setflags(write=False)
    return y


@functools.lru_cache(maxsize=None)
def float_outputs(name, pieces):
    """computed once, shared by the tests that need them, left unchanged"""
    return float_run(E.CASE[name], float_input(name), E.CASE[name].pieces[pieces])


@pytest.mark.parametrize("name", E.FLOAT_CASES)
def test_float_within_the_derived_bound_under_every_split(name):
    c = E.CASE[name]
    whole = float_outputs(name, "whole")
    RR.check(whole, c.L, c.M, c.taps, float_input(name), f"{name} whole")
    for pieces in c.pieces:
        y = float_outputs(name, pieces)
        diff = np.nonzero(y.view(np.uint64) != whole.view(np.uint64))[0]
        assert diff.size == 0, (name, pieces, diff[:5], whole[diff[:5]], y[diff[:5]])
        assert bits_equal(y, whole)


def levels(N, seed):
    """complex64 [N]: every component +- 2^e, e uniform in [-140, 100] -- denormals among them, and no product near overflow"""
    rng = np.random.default_rng(seed)
    v = rng.choice([-1.0, 1.0], (N, 2)) * 2.0 ** rng.integers(-140, 101, (N, 2))
    x = (v[:, 0] + 1j * v[:, 1]).astype(np.complex64)
    assert np.array_equal(x.real.astype(np.float64), v[:, 0]) and np.array_equal(x.imag.astype(np.float64), v[:, 1])  # (exact in float32)
    return x


@pytest.mark.parametrize("name", ["1/16 Q17", "3/50 Q40"])
def test_float_levels(name):
    c = E.CASE[name]
    x = levels(c.N, 50 + seed_of(name))
    assert np.abs(c.taps).max() <= c.L and (np.abs(x.real) < 2.0 ** -126).any() and np.abs(x.real).max() == 2.0 ** 100
    y64, sr, si = RR.restate(c.L, c.M, c.taps, x)
    assert np.isfinite(y64.real).all() and np.isfinite(y64.imag).all() and np.isfinite(sr).all() and np.isfinite(si).all()
    outs = [float_run(c, x, c.pieces[p]) for p in ("whole", "edge")]
    RR.check(outs[0], c.L, c.M, c.taps, x, f"{name} levels")
    assert bits_equal(outs[0], outs[1])


@pytest.mark.parametrize("where,seed", E.POISON, ids=[w for w, _ in E.POISON])
@pytest.mark.parametrize("name", ["1/16 Q17", "3/50 Q40"])
def test_float_poisoned_sample(name, where, seed):
    """one NaN sample: the outputs that are NaN are exactly those whose window holds it -- zero-padded taps included, 0 * NaN is NaN by
    the definition -- and every other output is the clean run's, bit for bit: a window that reads a sample outside its range shows,
    which finite data and zero taps hide.  Fed whole, and cut so that the first reader takes the sample from the source and the
    others from the carry (tests/test_resample_edges_cpu.py: in tiles of the path `where` both times)"""
    c = E.CASE[name]
    Qp = E.taps_per_phase(c)
    n_bad, cut = E.poison_plan(c, where, seed)
    n_m = RR.positions(c.L, c.M, np.arange(RR.counts(c.L, c.M, c.N)))[0]
    want = (n_m - (Qp - 1) <= n_bad) & (n_bad <= n_m)
    assert want.sum() >= 2 and np.array_equal(np.nonzero(want)[0], E.readers(c.L, c.M, Qp, c.N, n_bad)[0])
    clean = float_outputs(name, "whole")
    assert not np.isnan(clean.view(np.float32)).any()
    x = float_input(name).copy()
    x[n_bad] = complex(np.nan, np.nan)
    for pieces in ([c.N], cut):
        y = float_run(c, x, pieces)
        nan_re, nan_im = np.isnan(y.real), np.isnan(y.imag)
        bad = np.nonzero((nan_re != want) | (nan_im != want))[0]
        assert bad.size == 0, (name, pieces, n_bad, "outputs", bad[:5], "want NaN", want[bad[:5]], "got", y[bad[:5]])
        other = np.nonzero(~want & (y.view(np.uint64) != clean.view(np.uint64)))[0]
        assert other.size == 0, (name, pieces, n_bad, "outputs", other[:5], "want", clean[other[:5]], "got", y[other[:5]])


# ------------------------------------------------------------------------------------------------------------ the Q15 bank
@functools.lru_cache(maxsize=None)
def q15_input(name):
    x = Q.full_range(E.CASE[name].N, seed_of(name))
    x.setflags(write=False)
    return x


def q15_run(case, x, pieces):
    keep, addr = Q.to_device(x)
    bank = xl.ResamplerBankQ15()
    sid = bank.add(case.L, case.M, case.taps)
    y = Q.feed_pieces(bank, sid, case.L, case.M, addr, pieces)
    assert y.shape[0] == RR.counts(case.L, case.M, case.N) == bank.produced(sid)
    bank.close()
    y.setflags(write=False)
    return y


@functools.lru_cache(maxsize=None)
def q15_outputs(name, pieces):
    return q15_run(E.CASE[name], q15_input(name), E.CASE[name].pieces[pieces])


@pytest.mark.parametrize("name", E.Q15_CASES)
def test_q15_equals_the_restatement_under_every_split(name):
    c = E.CASE[name]
    whole = q15_outputs(name, "whole")
    for pieces in c.pieces:
        y = q15_outputs(name, pieces)
        Q.exact(y, c.L, c.M, c.taps, q15_input(name), f"{name} {pieces}")
        assert np.array_equal(y, whole), (name, pieces)


# ------------------------------------------------------------------------------------------------------------ company
def near_one(q15):
    """three streams of the ratios the banks exist for: (name, L, M, taps, N)"""
    one = np.full(1, 0.5, np.float32) if q15 else np.ones(1, np.float32)
    return [("3/5", *F.admission(10000000, 48000)[2:], 3000), ("7/8", *F.admission(2016000, 44100)[2:], 3000), ("1/1", 1, 1, one, 3000)]


def company(q15):
    """the bank's cases and three near-1 streams, in-place and LDS streams interleaved -> [(name, L, M, taps, c0, c1, x)]: two
    feeds of unequal counts per stream"""
    names = E.Q15_CASES if q15 else E.FLOAT_CASES
    by_kind = {"mem": [], "lds": []}
    for name in names:
        c = E.CASE[name]
        kinds = {t[2] for t in E.tile_paths(c.L, c.M, E.taps_per_phase(c), 0, c.N, E.span_limit("q" if q15 else "f"))}
        by_kind["mem" if "mem" in kinds else "lds"].append(name)
    assert len(by_kind["lds"]) == 3 and "1/(2^31-1) Q5" in by_kind["lds"]
    order, extra = [], near_one(q15)
    while by_kind["mem"] or by_kind["lds"] or extra:
        for pool in (by_kind["mem"], by_kind["lds"], extra):
            if pool:
                order.append(pool.pop(0))
    out = []
    for i, s in enumerate(order):
        if isinstance(s, str):
            c = E.CASE[s]
            c0 = 1000 if c.M == E.M_MAX and c.L == 1 else c.N // 3 + 7 * i + 1
            out.append((s, c.L, c.M, c.taps, c0, c.N - c0, (q15_input if q15 else float_input)(s)))
        else:
            name, L, M, taps, N = s
            x = Q.full_range(N, 70 + i) if q15 else F.noise(N, 70 + i)
            out.append((name, L, M, taps, 1100 + i, N - 1100 - i, x))
    return out


@pytest.mark.parametrize("q15", [False, True], ids=["float", "q15"])
def test_company_changes_no_bit(q15):
    """in-place tiles, LDS tiles and a run without workgroups (the second feed of 1 / (2^31 - 1): it consumes 5000 samples and
    produces nothing, between runs that do -- what xl_ragged_find's "never found" rule exists for) in one ragged launch: every
    stream's outputs are those of the same stream alone in a bank of its own"""
    pop = company(q15)
    H = Q if q15 else F
    esz = 4 if q15 else 8
    new_bank = xl.ResamplerBankQ15 if q15 else xl.ResamplerBank
    same = np.array_equal if q15 else bits_equal
    names = [p[0] for p in pop]
    silent = names.index("1/(2^31-1) Q5")
    assert 0 < silent < len(pop) - 1 and len(pop) == len(E.Q15_CASES if q15 else E.FLOAT_CASES) + 3
    assert RR.counts(1, E.M_MAX, 6000) - RR.counts(1, E.M_MAX, 1000) == 0
    dev = [H.to_device(p[6]) for p in pop]
    bank, alone = new_bank(), new_bank()
    sids = [bank.add(L, M, taps) for _, L, M, taps, *_ in pop]
    got = [[] for _ in pop]
    for f in range(2):
        counts = [p[4 + f] for p in pop]
        assert all(c > 0 for c in counts) and (f == 0 or counts != [p[4] for p in pop])
        bank.feed(sids, [d[1] + (esz * p[4] if f else 0) for d, p in zip(dev, pop)], counts, H.stream())
        assert bank.last_feed_ops() == (2, 1)
        bank.fetch()
        for i, sid in enumerate(sids):
            got[i].append(bank.output(sid))
    assert got[silent][1].shape[0] == 0 and got[silent][0].shape[0] == 1
    assert all(g[1].shape[0] > 0 for i, g in enumerate(got) if i != silent)
    for i, (name, L, M, taps, c0, c1, x) in enumerate(pop):
        y = np.concatenate(got[i])
        sid = alone.add(L, M, taps)
        want = H.feed_pieces(alone, sid, L, M, dev[i][1], [c0, c1])
        alone.remove(sid)
        assert same(y, want), (i, name)
        if name in E.CASE:  # ... which are the outputs held to the restatement above
            assert same(y, (q15_outputs if q15 else float_outputs)(name, "whole")), (i, name)
        elif q15:
            Q.exact(y, L, M, taps, x, f"company {name}")
        else:
            RR.check(y, L, M, taps, x, f"company {name}")
    bank.close()
    alone.close()
