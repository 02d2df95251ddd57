"""GPU tests (-m gpu) of the aligned 8-entry runs in the head and the tail of a region of xl_nco_chain_kernel's chain wave
(xl_chain_plan8, csrc/xl_chain_plan.h): single any-slot entries up to the next multiple of 8 ring slots, 8-entry runs up to the next
32-entry boundary, 32-entry blocks, 8-entry runs, single entries.

The engine, the call sequence and the checks are those of test_chain_regions_gpu.py (65 clients in two chain workgroups, D = 8, blocks
of 8 B samples = B outputs per block, calls of 3, 3, 3, 8, 3, ... blocks; after EVERY call every client's committed phase bit for bit and
every output against the oracle, test_chain_paths.run_call).  The covers are restated below (`cover8`) and the choice of B is asserted:
around 32-entry blocks every count of single entries in {0, 1, 7} and of 8-entry runs in {0, 1, 3} occurs on either side, and a second
shape has regions shorter than 32 entries that hold single entries, an 8-entry run and no block.

As those tests say of themselves: whether the chain wave WAITS for the drainers cannot be forced from Python; these cover the entry /
ring arithmetic of the new loops, not the waits."""
import pytest

import test_chain_paths as paths
import test_chain_regions_gpu as regions_gpu

STRIDE, RING, BLOCK, RUN = paths.STRIDE, paths.RING, 32, 8
SEQ = regions_gpu.SEQ


def cover8(e, e_stop):
    """(head1, head8, blocks, tail8, tail1) of the region [e, e_stop): xl_chain_plan8 restated"""
    if e_stop <= e:
        return (0, 0, 0, 0, 0)
    left, slot = e_stop - e, e % RING
    head1 = min((RUN - slot % RUN) % RUN, left)
    left, slot = left - head1, slot + head1
    to_block = (BLOCK - slot % BLOCK) % BLOCK
    if left < to_block:
        return (head1, left // RUN, 0, 0, left % RUN)
    left -= to_block
    return (head1, to_block // RUN, left // BLOCK, left % BLOCK // RUN, left % RUN)


def regions8(B, G):
    """covers of the regions of a call of G blocks of B outputs (test_chain_regions_gpu.regions, with cover8)"""
    _, ents, _ = paths.events(0, 8 * B, G)
    out, e = [], 0
    for en in ents + [(B * G - 1) // STRIDE]:
        if en >= e:
            out.append(cover8(e, en))
            e = en + 1
    return out


CASES = {"runs-around-blocks": 943, "runs-in-short-regions": 177}  # outputs per block


def test_chosen_lengths_give_the_runs():
    """(arithmetic only, no GPU: runs in the CPU suite)"""
    seen = {k: set() for k in ("head1", "head8", "tail8", "tail1")}
    for G in set(SEQ):
        for c, old in zip(regions8(CASES["runs-around-blocks"], G), regions_gpu.regions(CASES["runs-around-blocks"], G)[0]):
            assert c[0] + RUN * c[1] == old[0] and c[2] == old[1] and RUN * c[3] + c[4] == old[2], (c, old)  # the same head, blocks, tail
            if c[2] > 0:
                for k, v in zip(("head1", "head8", "tail8", "tail1"), (c[0], c[1], c[3], c[4])):
                    seen[k].add(v)
    assert {0, 1, 7} <= seen["head1"] and {0, 1, 7} <= seen["tail1"] and {0, 1, 3} <= seen["head8"] and {0, 1, 3} <= seen["tail8"], seen
    covs = regions8(CASES["runs-in-short-regions"], 3)
    assert all(c[2] == 0 and sum(c) > 0 and c[0] + RUN * c[1] + RUN * c[3] + c[4] < BLOCK for c in covs), covs
    assert any(c[0] > 0 and c[1] > 0 and c[4] > 0 for c in covs) and any(c[3] > 0 for c in covs), covs


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
def test_runs_of_eight(case):
    S = 8 * CASES[case]
    eng, ors = paths.make_engine(S, max(SEQ))
    for k, G in enumerate(SEQ):
        paths.run_call(eng, ors, 8700 + 20 * list(CASES).index(case) + k, S, G)
    assert "polyphase: cls0 D8 T17 cols65" in eng.describe(), eng.describe()
    eng.close()
