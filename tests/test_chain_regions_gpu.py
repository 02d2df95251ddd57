"""GPU tests (-m gpu) of how the chain wave of xl_nco_chain_kernel covers the regions between block ends (csrc/xl_chain_plan.h: a head
of any-slot single entries up to the next 32-entry boundary of the ring, 32-entry blocks, a tail of single entries) and of the entry
that holds a block end (counted steps, renormalisation, counted steps when the lanes agree).

The small engine of test_chain_paths.py: 65 clients (two chain workgroups, the second with a single client), D = 8 with 17 taps,
polyphase plan, chain on the side stream.  One table entry = 16 outputs.  Blocks of S = 8 B samples give every client B outputs per
block and leave the grid where it was, so every call of G blocks has its block ends after the outputs B, 2 B, ...: the entries that
hold them, the regions between them and the cover of each region are restated below (`regions`) and the choice of B is asserted.
After EVERY call: every client's committed phase bit for bit, every client's output within test_chain_paths.REL_TOL of the oracle.

Each case runs calls of 3, 3, 3, 8, 3, 3, 3, 3, 3 blocks: a fresh engine looks four calls ahead, a call of another shape drops the
look-ahead and the next launches tabulate one, two and four calls -- so the shape under test goes through chain launches of 1, 2
and 4 calls (and calls joined inside a launch), and through a call of 8 blocks.

What this does not reach (as test_chain_paths.py says of itself): whether the chain wave WAITS for the drainers cannot be forced from
Python -- with drainers that keep up the drain check in front of a head, a tail or a block run finds the ring free.  These tests
cover the entry / ring arithmetic of every path, not the waits."""
import pytest

import test_chain_paths as paths

STRIDE, RING, BLOCK = paths.STRIDE, paths.RING, 32
SEQ = (3, 3, 3, 8, 3, 3, 3, 3, 3)


def cover(e, e_stop):
    """(head, blocks, tail) of the region [e, e_stop): xl_chain_plan.h restated"""
    if e_stop <= e:
        return (0, 0, 0)
    left = e_stop - e
    head = min((BLOCK - e % BLOCK) % BLOCK, left)
    left -= head
    return (head, left // BLOCK, left % BLOCK)


def regions(B, G):
    """(covers of the regions of a call of G blocks of B outputs, entries that hold a block end, step of each block end inside its
    entry, K): the chain wave walks region, event entry, region, ... and the call's last entry is an event entry too (the call ends)"""
    E, ents, nbs = paths.events(0, 8 * B, G)
    K = B * G
    assert nbs == [g * B for g in range(1, G)] and E == (K + STRIDE - 1) // STRIDE
    out, e = [], 0
    for en in ents + [(K - 1) // STRIDE]:
        if en >= e:  # (en < e: a second block end in the same entry)
            out.append(cover(e, en))
            e = en + 1
    return out, ents, [(nb - 1) % STRIDE for nb in nbs], K


# outputs per block -> what the shape is there for
CASES = {
    "a-heads-0-15-16-31": 1155,
    "a-tails-15-31-heads-1-16": 1273,
    "b-short-regions": 200,
    "b-empty-regions": 17,
    "c-first-and-last-entry": 9,
    "d-event-at-step-0": 769,
    "d-event-at-step-15": 768,
}
WANT = {0, 1, 15, 16, 31}


def test_chosen_lengths_give_the_cases():
    """(arithmetic only, no GPU: runs in the CPU suite) the shapes put the heads, tails, short and empty regions and event steps where the cases ask for them"""
    heads, tails = set(), set()
    for B in (CASES["a-heads-0-15-16-31"], CASES["a-tails-15-31-heads-1-16"]):
        for G in (3, 8):
            covs = regions(B, G)[0]
            heads |= {h for h, b, t in covs if b > 0}
            tails |= {t for h, b, t in covs if b > 0}
    assert WANT <= heads and WANT <= tails, (heads, tails)  # (a): around at least one 32-entry block each
    covs = regions(CASES["b-short-regions"], 3)[0]
    assert all(b == 0 for h, b, t in covs) and any(h > 0 and t > 0 for h, b, t in covs), covs  # (b) shorter than 32, head and tail, no block
    for G in (3, 8):
        covs, ents, _, _ = regions(CASES["b-empty-regions"], G)
        assert ents == list(range(1, G)) and covs.count((0, 0, 0)) >= G - 1, (covs, ents)  # (b) block ends in consecutive entries
    _, ents, _, K = regions(CASES["c-first-and-last-entry"], 3)
    assert ents[0] == 0 and ents[-1] == (K - 1) // STRIDE and K % STRIDE != 0, (ents, K)  # (c)
    assert regions(CASES["d-event-at-step-0"], 3)[2][0] == 0  # (d)
    assert set(regions(CASES["d-event-at-step-15"], 3)[2]) == {15} and set(regions(CASES["d-event-at-step-15"], 8)[2]) == {15}
    # a second block end inside one entry (the entry falls back to the per-step loop after its first renormalisation)
    assert len(set(regions(CASES["c-first-and-last-entry"], 8)[1])) < 7


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
def test_regions_and_event_entries(case):
    S = 8 * CASES[case]
    eng, ors = paths.make_engine(S, max(SEQ))
    for k, G in enumerate(SEQ):
        paths.run_call(eng, ors, 8500 + 20 * list(CASES).index(case) + k, S, G)
    assert "polyphase: cls0 D8 T17 cols65" in eng.describe(), eng.describe()
    eng.close()
