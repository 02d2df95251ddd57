"""GPU tests (-m gpu) of the inverse launch's epilogue (xlp_inverse_body, xl_polyphase.hip): every store of a tile is guarded by one
window of shared points per column -- the column's shift, the outputs it owns, the segment's end, a vacant column -- and the phases come
from the tile row the expansion filled.  The forced polyphase plan of a small class puts every one of those cases into ONE tile:

* 40 clients join in three batches, at stream positions 0, N and 2 N samples with N mod 42 = 8 (16 for calls of two blocks): three
  offsets against the shared grid.  A member's shift is 0 exactly when its window offset j0 is below the reference member's, and
  (P - Q) mod 42 of the three batches changes its order as the stream position Q advances (test_three_offsets_rotate), so both shift
  values -- and, with N mod 42 != 0, both output counts K_c -- meet in one tile in some call;
* one client of the first batch leaves after the second call: a vacant column between live ones;
* 65536 bytes of cu8 per block are 780 or 781 outputs: seven segments of V = 116 shared points (M = 128), the last one partial;
* calls of one block and, in a second engine, of two blocks (group_blocks = 2).

After every call every client is compared with the oracle at the suite's 1e-5, and at M = 128 with the LDS transform (option
inverse_kernel = 3) a fixed sample of clients must equal tests/golden/inverse128_lds_parent.npz bit for bit: the outputs
tools/record_inverse128_golden.py recorded on an MI355X at commit 1c2f678 ("Batch engine: split xl_batch_run into stages, one copy of
each step"), the last one before the epilogue lost its branches -- the rewrite moves no float operation."""
import os

import numpy as np
import pytest

import siggen
import sdr_server_amd as xl
from conftest import GOLDEN
from pyoracle import Oracle

FS = 2016000
D = 42
BLOCK_BYTES = 65536
REL_TOL = 1e-5  # (the suite's bar for the optimized variant: tests/test_batch_gpu.py)
BATCHES = (14, 13, 13)  # clients joining before calls 0, 1, 2
LEAVER = 5  # index (join order) of the client that leaves after the second call
SAMPLE = (0, 4, 6, 13, 14, 26, 27, 39)  # join-order indices recorded in the golden file: both neighbours of the leaver, every batch's ends
GOLDEN_FILE = os.path.join(GOLDEN, "inverse128_lds_parent.npz")
CALLS = {1: 8, 2: 4}  # calls per engine, by blocks per call
SAMPLE_OF = {1: SAMPLE, 2: SAMPLE[1:8:2]}  # (the two-block engine records four clients: the file stays small)


def fc_of(i):
    return -900000 + 45000 * i


def run_scenario(group_blocks, each_call):
    """The call sequence above on one engine; each_call(call, x, outputs) gets every call's input bytes and {join index: complex64
    outputs} of the clients alive in it.  The plan is forced by the caller's environment (XL_EXP_POLY, XL_EXP_POLY_M, XL_EXP_INV)."""
    code, taps = xl.create_low_pass_filter(1.0, FS, 24000, 9600)
    assert code == 0 and len(taps) == 505
    eng = xl.BatchEngine(FS, "cu8", BLOCK_BYTES, group_blocks=group_blocks)
    ids, joined = {}, 0
    try:
        for call in range(CALLS[group_blocks]):
            if call < len(BATCHES):
                for i in range(joined, joined + BATCHES[call]):
                    ids[i] = eng.add_client(D, taps, fc_of(i))
                joined += BATCHES[call]
            if call == 2:
                eng.remove_client(ids.pop(LEAVER))
            x = siggen.xs_u8(siggen.XS_SEED + 300 + 10 * group_blocks + call, group_blocks * BLOCK_BYTES)
            if group_blocks == 1:
                eng.process_host(x, "optimized")
            else:
                eng.process_host_group(x, group_blocks, "optimized")
            eng.fetch()
            if call == 0:
                assert "polyphase: cls0 D42 T505" in eng.describe(), eng.describe()
            each_call(call, x, {i: eng.output(cid) for i, cid in ids.items()})
    finally:
        eng.close()


def force_plan(monkeypatch, m):
    monkeypatch.setenv("XL_EXP_POLY", "1")
    monkeypatch.setenv("XL_EXP_POLY_M", str(m))
    monkeypatch.setenv("XL_EXP_INV", "3")


def test_three_offsets_rotate():
    """The choice of the join positions, checked by arithmetic: a batch that joined at stream position P has window offset
    (P - Q) mod 42 in the call that starts at Q.  Whichever member the class takes as its reference, both shift values occur in a call
    in which the reference's offset is not the smallest; the smallest belongs to different batches in different calls after the
    third join, so there is such a call.  And a call's length is no multiple of 42: in some call members own K and K + 1 outputs."""
    for g, ncalls in CALLS.items():
        n = g * BLOCK_BYTES // 2
        assert n % D != 0
        joins = [b * n for b in range(len(BATCHES))]
        lowest, two_counts = set(), 0
        for call in range(len(BATCHES) - 1, ncalls):
            offs = [(p - call * n) % D for p in joins]
            assert len(set(offs)) == len(offs)
            lowest.add(offs.index(min(offs)))
            two_counts += len({(n - o + D - 1) // D for o in offs}) == 2  # outputs in [o, n) at spacing 42
        assert len(lowest) >= 2 and two_counts >= 1, (g, lowest, two_counts)
    assert all(0 <= i < sum(BATCHES) and i != LEAVER for i in SAMPLE) and LEAVER - 1 in SAMPLE and LEAVER + 1 in SAMPLE
    assert (BLOCK_BYTES // 2 + D - 1) // D in (780, 781) and 6 * 116 < 780 < 7 * 116


@pytest.mark.gpu
@pytest.mark.parametrize("m,group_blocks", [(128, 1), (128, 2), (64, 1), (256, 1)], ids=["M128", "M128-two-blocks", "M64", "M256"])
def test_epilogue_against_oracle_and_parent(m, group_blocks, monkeypatch):
    force_plan(monkeypatch, m)
    code, taps = xl.create_low_pass_filter(1.0, FS, 24000, 9600)
    golden = np.load(GOLDEN_FILE) if m == 128 else None
    oracles, worst, two_counts = {}, [0.0], [0]

    def each_call(call, x, outs):
        for i in outs:
            if i not in oracles:
                oracles[i] = Oracle(D, taps, fc_of(i), FS, BLOCK_BYTES)
        for i in [i for i in oracles if i not in outs]:
            oracles.pop(i).close()
        for i, got in outs.items():
            want = np.concatenate([oracles[i].process("cu8", xb) for xb in np.split(x, group_blocks)])
            assert len(got) == len(want), (call, i, len(got), len(want))
            err = float(np.abs(got.astype(np.complex128) - want.astype(np.complex128)).max() / np.abs(want).max())
            worst[0] = max(worst[0], err)
            assert err <= REL_TOL, (call, i, err)
        two_counts[0] += len({len(v) for v in outs.values()}) >= 2
        if golden is not None:
            for i in SAMPLE_OF[group_blocks]:
                key = "g%d_call%d_client%d" % (group_blocks, call, i)
                assert (key in golden.files) == (i in outs), key
                if i in outs:
                    assert np.array_equal(outs[i].view(np.uint32), golden[key]), (key, "differs from the parent's outputs")

    run_scenario(group_blocks, each_call)
    for o in oracles.values():
        o.close()
    print("worst relative error %.3g" % worst[0])
    assert two_counts[0] >= 1  # both output counts K_c met in one call
