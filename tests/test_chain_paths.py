"""GPU tests (-m gpu) of the paths inside the side-stream chain kernel (xl_kernels.hip xl_nco_chain_kernel): where a block of a call
ends relative to the 32-entry blocks of the chain wave and to its ring (64 entries, checked against the drainers every 32), calls
joined inside one look-ahead launch, lanes whose block ends differ, and the FMA step, which keeps the per-step path.

Small engines: 65 clients (two chain workgroups, the second with a single client), D = 8 with 17 taps, polyphase plan with the
chain on the side stream.  One table entry = 16 outputs, so a call of K outputs writes ceil(K / 16) entries; the block lengths
below are chosen from the grid arithmetic (csrc/xl_grid.h, restated in `events`) and the choice is asserted.
After EVERY call: every client's committed phase bit for bit, every client's output within 1e-5 of the oracle.

What this does not reach: whether the chain wave actually WAITS for the drainers cannot be forced from Python.  Entry 96 is where a
kernel that checks the ring every 32 entries has its check; a kernel that reads the drainers' counters during its blocks waits only
when they have fallen behind, so with drainers that keep up neither the wait in front of the event entry nor the early exit of the
block loop is taken in these tests -- they cover the entry / ring arithmetic of every path, not the waits."""
import numpy as np
import pytest

import siggen
import sdr_server_amd as xl
from pyoracle import Oracle

pytestmark = pytest.mark.gpu
REL_TOL = 1e-5
D, NTAPS, FS, NCLIENTS = 8, 17, 384000, 65
STRIDE, RING = 16, 64  # outputs per table entry; ring entries of the chain wave (a drain check every RING / 2 from RING on)


def events(consumed, S, G):
    """(entries of the call, [entry that holds the end of block g, g = 1 .. G - 1], [output index after which the phase is
    renormalised there]) for a client that has seen `consumed` samples, in a call of G blocks of S samples (xl_grid.h:
    xl_grid_dyn / xl_grid_mstart / xl_bnd_next)."""
    j0 = (-consumed) % D
    N = S * G
    K = (N - j0 + D - 1) // D if N > j0 else 0
    nbs = [min((g * S - j0 + D - 1) // D if g * S > j0 else 0, K) for g in range(1, G)]
    return (K + STRIDE - 1) // STRIDE, [(nb - 1) // STRIDE for nb in nbs], nbs


# samples per block -> calls of 2, 3 and 8 blocks whose inner block ends cover the entry residues 0, 1, 15, 16, 31 (mod 32)
SHAPES = {2: 8 * 1537, 3: 8 * 768, 8: 8 * 272}


def test_chosen_lengths_hit_the_residues():
    """(arithmetic only) the three shapes together put a block end at every residue asked for, one of them in an entry where
    the ring is checked against the drainers, and every call wraps the ring twice."""
    seen, at_check = set(), False
    for G, S in SHAPES.items():
        for call in range(3):  # S = 0 mod D: the grid does not move from call to call
            E, ents, _ = events(call * G * S, S, G)
            assert E >= 130
            seen |= {e % 32 for e in ents}
            at_check |= any(e % (RING // 2) == 0 and e >= RING for e in ents)
    assert {0, 1, 15, 16, 31} <= seen and at_check, (seen, at_check)
    assert events(0, SHAPES[2], 2)[1] == [96] and events(0, SHAPES[3], 3)[1] == [47, 95]
    assert [e % 32 for e in events(0, SHAPES[8], 8)[1][:2]] == [16, 1]


def taps():
    return siggen.hamming_sinc(NTAPS, 0.05)


def rel_err(a, b):
    return float(np.abs(a.astype(np.complex128) - b.astype(np.complex128)).max() / max(np.abs(b).max(), 1e-30))


def make_engine(max_samples, gcap, nclients=NCLIENTS, **okw):
    eng = xl.BatchEngine(FS, "cu8", 2 * max_samples, group_blocks=gcap)
    eng.set_option("polyphase", 1)
    eng.set_option("nco_side_stream", 1)
    ors = {}
    add_clients(eng, ors, 0, nclients, 2 * max_samples, **okw)
    return eng, ors


def add_clients(eng, ors, first, count, max_bytes, **okw):
    t = taps()
    for c in range(first, first + count):
        fc = -180000 + 5500 * c
        ors[eng.add_client(D, t, fc)] = Oracle(D, t, fc, FS, max_bytes, **okw)


def run_call(eng, ors, seed, S, G, variant="optimized"):
    x = siggen.xs_u8(seed, 2 * S * G)
    eng.process_host_group(x, G, variant)
    eng.fetch()
    blocks = np.split(x, G)
    for cid, o in ors.items():
        want = np.concatenate([o.process("cu8", bl) for bl in blocks])
        got = eng.output(cid)
        assert len(got) == len(want), (cid, len(got), len(want))
        assert rel_err(got, want) <= REL_TOL, (cid, rel_err(got, want))
        assert tuple(np.float32(v).tobytes() for v in eng.phase(cid)) == tuple(np.float32(v).tobytes() for v in o.phase), cid


@pytest.mark.parametrize("G", [2, 3, 8])
def test_block_ends_at_the_residues(G):
    """Five equal calls of 2 / 3 / 8 blocks (one launch for the first look-ahead, then launches of two and of four calls):
    block ends at entries 96 (a drain check), 47 and 95, 16 and 33 ..."""
    S = SHAPES[G]
    assert events(0, S, G)[0] >= 130
    eng, ors = make_engine(S, G)
    for k in range(5):
        run_call(eng, ors, 8100 + 10 * G + k, S, G)
    assert "polyphase: cls0 D8 T17 cols65" in eng.describe(), eng.describe()
    eng.close()


def test_shape_change_inside_a_lookahead_launch():
    """Equal calls until a launch of four calls is pending, then another shape (the pending tables are dropped), and back."""
    eng, ors = make_engine(max(SHAPES[3], SHAPES[2]), 3)
    seq = [(3, SHAPES[3])] * 5 + [(2, SHAPES[2])] * 2 + [(3, SHAPES[3])] * 2
    for k, (G, S) in enumerate(seq):
        run_call(eng, ors, 8200 + k, S, G)
    eng.close()


def test_lanes_with_different_block_ends():
    """33 clients, one block of 3 mod 8 samples, then 32 more: the two cohorts' grids are offset, and with blocks of 3 mod 8
    samples their block ends fall on different outputs (asserted), so the event is no longer the same in every lane."""
    S0, S, G = 8 * 1537 + 3, 8 * 768 + 3, 3
    eng, ors = make_engine(S0, G, nclients=33)
    run_call(eng, ors, 8300, S0, 1)
    add_clients(eng, ors, 33, 32, 2 * S0)
    old, new, differ = S0, 0, 0
    for k in range(4):
        a, b = events(old, S, G), events(new, S, G)
        assert a[0] >= 130 and b[0] >= 130
        differ += a[2] != b[2]
        run_call(eng, ors, 8301 + k, S, G)
        old, new = old + G * S, new + G * S
    assert differ >= 2
    eng.close()


def test_fma_step_mode_keeps_the_per_step_path():
    """The x86 FMA flavour: the contracted step, no renormalisation, per-step path throughout; three calls of three blocks."""
    S, G = SHAPES[3], 3
    eng, ors = make_engine(S, G, renorm=False, fma_step=True)
    for k in range(3):
        run_call(eng, ors, 8400 + k, S, G, variant="optimized_x86_fma")
    eng.close()
