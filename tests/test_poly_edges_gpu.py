"""GPU tests (-m gpu) of the polyphase overlap-save path at every call-length edge of its segment grid: xlp_forward_kernel, the mix
kernels and the inverse kernels on calls whose lengths tests/poly_edges.py chose from the grid arithmetic (Kq = 0, 1, 2, V - 1 mod V;
a last pass of one segment of one point that some members own, or none; nseg = 0, 1, 15 mod 16 and both parities; the engine's
capacity and a sample less; 512 outputs -- polyphase -- and 511 -- direct -- in one stream; a second class whose whole call is a
fraction of one segment; block ends on the first and last point of a segment and on a phase group; calls of four and five passes, where
a cf32 stream's forward launch runs groups of four branches).  tests/test_poly_edges_cpu.py
asserts, without a GPU, that the sequences hold those cases; here small engines with the plan forced run them.

Clients (poly_edges: the protocol): 18 join before the first call, 17 behind it -- its length is no multiple of D, so the class has
members at two offsets --, one leaves mid-sequence.  After EVERY call, for EVERY client: the output length per block is the
oracle's; max|d| <= 1e-5 max|y| per call and per block (REL_TOL: the project's bar for the optimized variant); the committed phase
equals the oracle's bit for bit; the one native call of a sequence is bit-exact; no call returns an error (-EIO would be a call
beyond the segment capacity); and the class's "calls=" count in describe() advances exactly on the calls the arithmetic sends down
the polyphase launches, so no edge silently runs on the direct kernel.

cf32 shapes: the two-half mix scales the shared spectra per segment and reads the scales in pairs.  Some calls end with two
segments 2^10 below the rest of the call, and the call behind such a one begins with one quiet segment in front of a loud one: an
even pair entry that is quiet beside an odd one that is loud.  A scale taken from the wrong entry of the pair then overflows the
half-precision operands instead of costing a few bits.  The rule for such passages is DESIGN 5's, as in
test_cf32_two_half_mix_adversarial_levels_in_one_call: a block is held to 1e-5 of its own max|y| unless a neighbouring block is more
than 100 x louder, then to 1e-5 of that; every quiet passage here lies inside a block that also holds loud samples, so the passage
is held to its louder neighbourhood's scale.

Each test prints its worst error (pytest -s; profiles/poly_call_edges.txt)."""
import functools
import re

import numpy as np
import pytest

import poly_edges as pe
import siggen
import sdr_server_amd as xl
from conftest import bits_equal
from pyoracle import Oracle

pytestmark = pytest.mark.gpu
REL_TOL = 1e-5
QUIET = np.float32(2.0 ** -10)
CLASS_RE = re.compile(r" cls(\d+) D(\d+) T(\d+) cols(\d+) V(\d+) M(\d+)(?: offsets<=(\d+))? mix=(\S+)(?: inv=(\S+))? calls=(\d+)")
INV_NAME = {3: "lds", 5: "lanes8", 6: "cut32"}


def _classes(desc):
    """describe() -> [dict per polyphase class]"""
    keys = ("cls", "D", "T", "cols", "V", "M", "offsets", "mix", "inv", "calls")
    out = []
    for m in CLASS_RE.finditer(desc.split("| polyphase:")[1].split("|")[0]):
        out.append({k: (v if k in ("mix", "inv") else int(v or 0)) for k, v in zip(keys, m.groups())})
    return out


def _clients(shape, with_second):
    """-> [(D, taps, fc)] by client index: cohort A, cohort B, then the second class"""
    n = pe.NA + pe.NB
    taps = siggen.hamming_sinc(shape.T, shape.cutoff)
    out = [(shape.D, taps, int(-0.4 * shape.fs + 0.8 * shape.fs * i / (n - 1)) - 7 * i) for i in range(n)]
    if with_second:
        D2, T2, cut2 = shape.second
        taps2 = siggen.hamming_sinc(T2, cut2)
        out += [(D2, taps2, int(0.11 * shape.fs * (j - 1)) + 1234) for j in range(pe.N2)]
    return out


def _alive(idx, call_index):
    if idx == pe.LEAVER:
        return call_index <= pe.LEAVE_AFTER
    if pe.NA <= idx < pe.NA + pe.NB:
        return call_index >= 1
    return True


def _input(shape, M, seq, call_index, rec):
    n = rec.call.S * rec.call.G
    seed = 7000 + 1000 * "ABCD".index(shape.name) + 100 * pe.SEQUENCE_NAMES.index(seq) + 10 * (M // 64) + call_index
    if shape.fmt == "cu8":
        return siggen.xs_u8(seed, 2 * n)
    x = (siggen.xs_s16(seed, 2 * n).astype(np.float32) / np.float32(32768)).astype(np.float32)
    span = pe.quiet_span(shape, M, rec)
    if span:
        x[2 * span[0]:2 * span[1]] *= QUIET
    return x


def _phase_bits(p):
    return tuple(np.float32(v).tobytes() for v in p)


@functools.lru_cache(maxsize=None)
def _reference(name, M, seq):
    """The oracle over a sequence, computed once for every mix and inverse kernel that runs it: -> (recs, inputs per call,
    {call index: {client index: ([outputs per block], phase bits)}})"""
    shape = pe.SHAPES[name]
    with_second = seq == "thresh" and shape.second is not None
    recs = pe.walk(shape, M, pe.sequences(shape, M)[seq], second=with_second)
    cap_s, _ = pe.engine_limits([r.call for r in recs])
    clients = _clients(shape, with_second)
    oracles, inputs, want = {}, [], {}
    for ci, rec in enumerate(recs):
        x = _input(shape, M, seq, ci, rec)
        inputs.append(x)
        want[ci] = {}
        for idx, (D, taps, fc) in enumerate(clients):
            if not _alive(idx, ci):
                if idx in oracles:
                    oracles.pop(idx).close()
                continue
            if idx not in oracles:
                oracles[idx] = Oracle(D, taps, fc, shape.fs, 2 * cap_s)
            blocks = [oracles[idx].process(shape.fmt, xb) for xb in np.split(x, rec.call.G)]
            want[ci][idx] = (blocks, _phase_bits(oracles[idx].phase))
    for o in oracles.values():
        o.close()
    return recs, inputs, want


def _err(got, want):
    return float(np.abs(got.astype(np.complex128) - want.astype(np.complex128)).max()) if len(want) else 0.0


def _scale(w):
    return float(np.abs(w).max()) if len(w) else 0.0


def _bar_scale(own, neighbours):
    """a block's own max|y| -- unless a neighbouring block's is more than 100 x larger, then that one"""
    near = max(neighbours) if neighbours else 0.0
    return own if near <= 100.0 * own else near


def run_sequence(name, M, seq, mix=1, inv=0):
    """One engine over one sequence; every assertion of the module's docstring after every call.  -> {call name: whether the main
    class's count advanced}, worst relative error"""
    shape = pe.SHAPES[name]
    with_second = seq == "thresh" and shape.second is not None
    recs, inputs, want = _reference(name, M, seq)
    cap_s, gcap = pe.engine_limits([r.call for r in recs])
    V = pe.valid_points(M, shape.T, shape.D, shape.r)
    clients = _clients(shape, with_second)
    eng = xl.BatchEngine(shape.fs, shape.fmt, 2 * cap_s, group_blocks=gcap)
    eng.set_option("polyphase", 1)
    eng.set_option("polyphase_m", M)
    eng.set_option("mix_kernel", mix)
    eng.set_option("inverse_kernel", inv)
    want_mix = "mf32" if (mix == 3 or shape.D > 112) else "mfma"
    ids, counts, advanced = {}, {}, {}
    worst, worst_at = 0.0, None
    last_scale = {}  # client index -> max|y| of its latest block
    try:
        for ci, rec in enumerate(recs):
            c = rec.call
            for idx, (D, taps, fc) in enumerate(clients):
                if _alive(idx, ci) and idx not in ids and (ci == 0 or (ci == 1 and idx >= pe.NA)):
                    ids[idx] = eng.add_client(D, taps, fc)
            if ci == pe.LEAVE_AFTER + 1:
                eng.remove_client(ids.pop(pe.LEAVER))
            assert sorted(ids) == sorted(want[ci]), (ci, sorted(ids))
            eng.process_host_group(inputs[ci], c.G, c.variant)  # (an error code raises: -EIO would be a call beyond the capacity)
            eng.fetch()
            # ---- the plan, and which path the call took
            desc = eng.describe()
            classes = _classes(desc)
            assert classes and "re-plan pending" not in desc, desc
            main = max((k for k in classes if k["D"] == shape.D), key=lambda k: k["cols"])
            assert (main["V"], main["M"]) == (V, M) and main["mix"].startswith(want_mix), desc
            if M == 128 and inv:
                assert main["inv"] == INV_NAME[inv], desc
            if with_second:  # the second class is a polyphase class: its window stays on the LDS tile, it is no wide client
                second = [k for k in classes if k["D"] == shape.second[0]]
                assert len(second) == 1 and second[0]["cols"] == pe.N2 and second[0]["T"] == shape.second[1] and "wide:" not in desc, desc
            if rec.poly:
                assert all(k["calls"] >= 1 for k in classes), (c.name, desc)
            if ci >= 2:  # both cohorts are one class: one class per decimation, kept by every later plan
                assert len(classes) == (2 if with_second else 1), desc
                assert main["cols"] == len([i for i in ids if i < pe.NA + pe.NB]) and main["offsets"] == shape.r, desc
                for k in classes:
                    assert k["calls"] == counts[k["D"]] + (1 if rec.poly else 0), (c.name, "polyphase" if rec.poly else "direct", counts, desc)
                advanced[c.name] = main["calls"] == counts[shape.D] + 1
            counts = {}
            for k in sorted(classes, key=lambda k: k["cols"]):
                counts[k["D"]] = k["calls"]  # (the class of most columns per decimation: cohort A's in call 1)
            # ---- every client against the oracle
            for idx, cid in ids.items():
                blocks, phase = want[ci][idx]
                got = eng.output(cid)
                lens = [eng.output_len_block(cid, g) for g in range(c.G)]
                assert lens == [len(w) for w in blocks] and len(got) == sum(lens), (c.name, idx, lens, [len(w) for w in blocks], len(got))
                if idx < pe.NA + pe.NB:
                    assert len(got) == (rec.k_a if idx < pe.NA else rec.k_b), (c.name, idx, len(got), rec.k_a, rec.k_b)
                whole = np.concatenate(blocks)
                if c.variant == "native":
                    assert bits_equal(got, whole), (c.name, idx, _err(got, whole))
                else:
                    scales = [_scale(w) for w in blocks]
                    assert min(scales) > 0.0, (c.name, idx)
                    e = _err(got, whole) / _bar_scale(max(scales), [last_scale[idx]] if idx in last_scale else [])
                    if e > worst:
                        worst, worst_at = e, (c.name, idx)
                    assert e <= REL_TOL, (name, M, seq, c.name, idx, e, "per call")
                    off = 0
                    for g in range(c.G):
                        near = ([scales[g - 1]] if g else ([last_scale[idx]] if idx in last_scale else [])) + scales[g + 1:g + 2]
                        e = _err(got[off:off + lens[g]], blocks[g]) / _bar_scale(scales[g], near)
                        off += lens[g]
                        assert e <= REL_TOL, (name, M, seq, c.name, idx, g, e, "per block")
                last_scale[idx] = _scale(blocks[-1])
                assert _phase_bits(eng.phase(cid)) == phase, (c.name, idx)
    finally:
        eng.close()
    print("poly_edges %s M%d V%d %-6s mix=%s inv=%s worst %.3g at %s" % (name, M, V, seq, want_mix, INV_NAME.get(inv, "auto"), worst, worst_at))
    return advanced, worst


def _cases():
    out = []
    for name in sorted(pe.SHAPES):
        sh = pe.SHAPES[name]
        for M in sh.Ms:
            for seq in pe.SEQUENCES_OF[name]:
                for mix in ((1, 3) if name == "A" else (1,)):  # shape A: the two-half mix (constant scale) and the float32 mix
                    out.append((name, M, seq, mix))
    return out


@pytest.mark.parametrize("name,M,seq,mix", _cases(), ids=lambda v: str(v))
def test_call_length_edges(name, M, seq, mix):
    """Shapes A (cu8, D = 8), B (cf32, D = 8: per-segment scales), C (cf32, D = 100: the wide two-half kernel, 13 k-blocks) and D (cu8,
    D = 200: the streamed float32 mix) at every transform length of the shape, over the sequences of poly_edges.sequences."""
    advanced, _ = run_sequence(name, M, seq, mix=mix)
    assert advanced == {r.call.name: r.poly for r in _reference(name, M, seq)[0][2:]} and not advanced["native"], advanced
    if seq == "thresh":  # 512 outputs take the polyphase launches, 511 the direct kernel, 511 and 512 in one class the polyphase launches
        assert advanced["k512"] and not advanced["k511"] and advanced["k512-some"] and advanced["k512-again"], advanced
    else:
        assert all(v for n, v in advanced.items() if n != "native"), advanced


@pytest.mark.parametrize("inv", [3, 5, 6], ids=["lds", "lanes8", "cut32"])
def test_inverse_kernels_on_the_edges_sequence(inv):
    """Shape A at M = 128 on the three inverse kernels (xlp_inverse_kernel<128>, xl_inv8.hip, xl_inv32.hip): the one-point last segment
    that cohort A owns and cohort B does not, the one nobody owns, the last segment of V - 1 points, nseg = 15, 16, 17."""
    run_sequence("A", 128, "edges", mix=1, inv=inv)
