"""GPU tests (-m gpu) of the inverse launches' phase expansion on the table's grid (xl_grid.h: xl_grid_duty; xl_dev_inline.h:
xl_phase_expand): lane g of a column takes table entry t0 + g and steps exactly 16 phases, the last lane a few more, and a wave none of
whose lanes meets a block end walks in a straight line.  No float operation moved, so every inverse kernel must give the outputs the
parent commit gave, bit for bit.

The scenario is tests/test_inverse_epilogue_gpu.py's -- 40 clients in three joins at stream positions 0, N and 2 N, one leaver, cu8
blocks of 65536 bytes (780 or 781 outputs in seven segments of V = 116 at M = 128), calls of one and of two blocks -- run under each of
the three 128-point inverse kernels (XL_EXP_INV = 3, 5, 6) and under the LDS kernel at M = 64 and M = 256.  Two more block lengths for
the two-block engine put a block end where only the new walk can go wrong (chosen with the model of tests/test_phase_expand_cpu.py,
shown to occur by arithmetic in test_added_lengths_hit_their_cases):

* 48460 bytes: in call 2 the first block of every member ends behind output 576, so that its output 577 is renormalised.  For a
  column of shift 1 segment 4 is the window [463, 579): t0 = 28, the eight lanes cover 448 .. 575 and the last one steps on through
  576, 577, 578 -- the block end lies inside the last lane's extra steps;
* 48360 bytes: the second block of every member starts at output 576, a multiple of 16: the renormalised phase is a table entry, step 0
  of lane 7 of segment 4 (shift 0) and of lane 0 of segment 5, and the lane before it must not use its own 16th step.

After every call every client is compared with the oracle at the suite's 1e-5, and two clients per case with
tests/golden/phase_expand_parent.npz: the outputs tools/record_phase_expand_golden.py recorded on an MI355X at commit 8d9cad7 ("Tune a
running client: a phase-continuous rotator bank behind the engine"), the parent of the change."""
import os

import numpy as np
import pytest

import siggen
import sdr_server_amd as xl
from conftest import GOLDEN
from pyoracle import Oracle

FS = 2016000
D = 42
V128 = 116  # valid outputs per segment at M = 128: 505 taps on 42 branches are 13 per branch
REL_TOL = 1e-5  # (the suite's bar for the optimized variant: tests/test_batch_gpu.py)
BATCHES = (14, 13, 13)  # clients joining before calls 0, 1, 2
LEAVER = 5  # index (join order) of the client that leaves after the second call
SAMPLE = (4, 27)  # join-order indices recorded in the golden file: a neighbour of the leaver (first batch), the third batch's first
GOLDEN_FILE = os.path.join(GOLDEN, "phase_expand_parent.npz")
TAIL_BYTES, ENTRY_BYTES = 48460, 48360
# id: (XL_EXP_INV, XL_EXP_POLY_M, blocks per call, bytes per block, calls, calls recorded in the golden file)
CASES = {
    "inv3-M128": (3, 128, 1, 65536, 8, (2, 3)),
    "inv3-M128-two-blocks": (3, 128, 2, 65536, 4, (2, 3)),
    "inv5-M128": (5, 128, 1, 65536, 8, (2, 3)),
    "inv5-M128-two-blocks": (5, 128, 2, 65536, 4, (2, 3)),
    "inv6-M128": (6, 128, 1, 65536, 8, (2, 3)),
    "inv6-M128-two-blocks": (6, 128, 2, 65536, 4, (2, 3)),
    "inv3-M64": (3, 64, 1, 65536, 8, (2, 3)),
    "inv3-M256": (3, 256, 1, 65536, 8, (2, 3)),
    "inv3-tail": (3, 128, 2, TAIL_BYTES, 3, (2,)),
    "inv5-tail": (5, 128, 2, TAIL_BYTES, 3, (2,)),
    "inv6-tail": (6, 128, 2, TAIL_BYTES, 3, (2,)),
    "inv3-entry": (3, 128, 2, ENTRY_BYTES, 3, (2,)),
    "inv5-entry": (5, 128, 2, ENTRY_BYTES, 3, (2,)),
    "inv6-entry": (6, 128, 2, ENTRY_BYTES, 3, (2,)),
}


def fc_of(i):
    return -900000 + 45000 * i


def force_plan(setenv, case):
    inv, m = CASES[case][:2]
    setenv("XL_EXP_POLY", "1")
    setenv("XL_EXP_POLY_M", str(m))
    setenv("XL_EXP_INV", str(inv))


def run_case(case, each_call):
    """The call sequence above on one engine; each_call(call, x, outputs) gets every call's input bytes and {join index: complex64
    outputs} of the clients alive in it.  The plan is forced by the caller's environment (force_plan)."""
    _, _, group_blocks, block_bytes, ncalls, _ = CASES[case]
    code, taps = xl.create_low_pass_filter(1.0, FS, 24000, 9600)
    assert code == 0 and len(taps) == 505
    eng = xl.BatchEngine(FS, "cu8", block_bytes, group_blocks=group_blocks)
    ids, joined = {}, 0
    try:
        for call in range(ncalls):
            if call < len(BATCHES):
                for i in range(joined, joined + BATCHES[call]):
                    ids[i] = eng.add_client(D, taps, fc_of(i))
                joined += BATCHES[call]
            if call == 2:
                eng.remove_client(ids.pop(LEAVER))
            x = siggen.xs_u8(siggen.XS_SEED + 700 + 10 * group_blocks + call, group_blocks * block_bytes)
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


def golden_key(case, call, i):
    return "%s_call%d_client%d" % (case, call, i)


def block_starts(block_bytes, call):
    """Per batch alive in `call` of the two-block engine: (window offset j0, output index of the second block's first output).  A batch
    that joined at stream position P has offset (P - Q) mod 42 in the call that starts at Q (tests/test_inverse_epilogue_gpu.py)."""
    s = block_bytes // 2
    n = 2 * s
    res = []
    for b in range(min(call + 1, len(BATCHES))):
        j0 = (b * n - call * n) % D
        res.append((j0, (s - j0 + D - 1) // D))
    return res


def test_added_lengths_hit_their_cases():
    """By arithmetic: in call 2 of the two added lengths a block end lies (a) inside the extra steps of the last lane of a column of
    shift 1, behind at least one of them and in front of a stored phase, (b) on a multiple of 16 that is a lane's first phase in two
    segments.  The member with the largest window offset has shift 1 whichever member is the class's reference (xl_grid.h)."""
    extra = V128 + 15 - 128
    assert extra == 3
    # (a)
    starts = block_starts(TAIL_BYTES, 2)
    assert len(starts) == 3 and TAIL_BYTES % D != 0
    j0, nb = max(starts)
    k = (TAIL_BYTES - j0 + D - 1) // D  # outputs of the member in the call
    hit = []
    for s in range((k + V128) // V128):
        m_lo, m_hi = max(s * V128, 1) - 1, min(s * V128 + V128, 1 + k) - 1
        tail0 = (m_lo & ~15) + 128  # the last lane's phases: tail0 - 16 .. tail0 + extra - 1
        if m_lo < m_hi and tail0 < nb < min(tail0 + extra, m_hi):
            hit.append(s)
    assert hit == [4] and nb == 577, (hit, nb)
    assert all(i // BATCHES[0] == 0 for i in SAMPLE[:1]) and max(starts) == starts[0]  # the recorded first-batch client is that member
    # (b)
    starts = block_starts(ENTRY_BYTES, 2)
    assert all(nb == 576 for _, nb in starts) and ENTRY_BYTES % D != 0
    firsts = set()
    for shift in (0, 1):
        for s in range(9):
            m_lo = max(s * V128, shift) - shift
            for g in range(8):
                if (m_lo & ~15) + 16 * g == 576 and 576 < m_lo + V128:
                    firsts.add((shift, s, g))
    assert {(0, 4, 7), (0, 5, 0), (1, 5, 0)} <= firsts, firsts


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
def test_against_oracle_and_parent(case, monkeypatch):
    force_plan(monkeypatch.setenv, case)
    _, _, group_blocks, block_bytes, _, recorded = CASES[case]
    code, taps = xl.create_low_pass_filter(1.0, FS, 24000, 9600)
    golden = np.load(GOLDEN_FILE)
    oracles, worst, compared = {}, [0.0], [0]

    def each_call(call, x, outs):
        for i in outs:
            if i not in oracles:
                oracles[i] = Oracle(D, taps, fc_of(i), FS, block_bytes)
        for i in [i for i in oracles if i not in outs]:
            oracles.pop(i).close()
        for i, got in outs.items():
            want = np.concatenate([oracles[i].process("cu8", xb) for xb in np.split(x, group_blocks)])
            assert len(got) == len(want), (call, i, len(got), len(want))
            err = float(np.abs(got.astype(np.complex128) - want.astype(np.complex128)).max() / np.abs(want).max())
            worst[0] = max(worst[0], err)
            assert err <= REL_TOL, (call, i, err)
        if call in recorded:
            for i in SAMPLE:
                key = golden_key(case, call, i)
                assert key in golden.files and i in outs, key
                assert np.array_equal(outs[i].view(np.uint32), golden[key]), (key, "differs from the parent's outputs")
                compared[0] += 1

    run_case(case, each_call)
    for o in oracles.values():
        o.close()
    print("worst relative error %.3g" % worst[0])
    assert compared[0] == len(recorded) * len(SAMPLE)
