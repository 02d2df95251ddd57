"""The cases that hold every k-block count of the polyphase mix kernels to the oracle (no GPU, no library).

A polyphase class's mix launch is compiled per number of k-blocks of 8 branches, nkb = ceil(D / 8) (XlpArgs::nkb), and D is the client's
decimation.  Four switches turn nkb into a template argument:

    xlp_mix_mfma_kernel<NKB, SEG, IMG>    xl_mixh.hip    NKB 1 .. 8: integer formats (converting staging), cf32 (per-segment scales,
                                                         SEG), the operand image (IMG)
    xlp_mix_mfma_wide_kernel<NKB, SEG>    xl_mixh2.hip   NKB 9 .. 14: integer formats, SEG
    xlp_mix_f32_kernel<NB8>               xl_mixf32.hip  NB8 1 .. 14 (option mix_kernel = 3)
    xlp_mix_f32_stream_kernel             xl_mixf32.hip  nkb >= 15, a run-time count

and NKB is more than a loop bound in them: the staging rounds ((NKB + 3) / 4: k-blocks of the last round beyond NKB are trimmed by a
guard or go to the wide kernel's dump slot), the rounds of the image copy, the waves-per-SIMD budget (SEG: 4 / 5, plain: 6 / 7), the
wide kernel's pinned schedule with A operands four k-blocks ahead, and the rows D .. 8 nkb - 1 that exist only as padding.

Per count two decimations: D = 8 nkb (no padding row) and D = 8 nkb - 7 (seven; nkb = 1: D = 3, five).  Filters of 4 D + 1 taps: 5 per
branch, inside the size rule's floor of 2 and the 8 that a 64-point class allows.  Every engine gets `polyphase` = 1 and its
transform length, so no case depends on a size rule: 128 points up to 8 k-blocks (the operand image exists at 128 and 256 only), 64
from 9 on (what the plan gives such classes), and 128 as well at 9, 12 and 14; 128 for the streamed kernel.

The call: blocks of 16384 samples, 8 per call -- wherever 8 blocks are at least 17 segments, i.e. two passes of 16 with the last one
partial.  They are not in the 128-point cases of more than 66 branches (V = 124 points per segment: D = 72 is 15 segments, D = 120
is 9), which would leave the wide kernels' and the streamed kernel's second pass without a 128-point case; those seven take 16
blocks per call (18 .. 30 segments).  tests/test_mix_kblocks_cpu.py asserts both sides from the grid arithmetic, and that this
table holds exactly the instantiations the four switches can reach; tests/test_mix_kblocks_gpu.py runs it."""
import collections

NSAMP = 16384                # samples per block
CLIENTS = 37                 # wave 0 full, wave 1 with five columns, waves 2 and 3 vacant
CLIENTS_TWO_GROUPS = 160     # a second, partial column group
NKB_TWO_GROUPS = (4, 10, 14)  # plain arm: also one case of 160 clients (the padded decimation)
NKB_ALSO_CS16 = (9, 12)
NKB_ALSO_128 = (9, 12, 14)
MIN_SEGMENTS = 17

Case = collections.namedtuple("Case", "arm nkb D T fmt M clients blocks options tag not_tag")
# options: the engine's options, in the order they are set; tag / not_tag: what describe() must / must not show for the class


def decimations(nkb):
    """(D_pad, D_full) of a k-block count"""
    return (3 if nkb == 1 else 8 * nkb - 7, 8 * nkb)


def taps_of(D):
    return 4 * D + 1


def segments_of(D, T, M, blocks):
    """xl_grid.h / xl_plan.cpp (restated in tests/poly_edges.py): segments of a call of `blocks` blocks, all members on one grid"""
    kq = (NSAMP * blocks + D - 1) // D + 1
    v = M - (T + D - 1) // D + 1
    return (kq + v - 1) // v


def blocks_of(D, M):
    """8 blocks per call, 16 where 8 are fewer than 17 segments"""
    return 8 if segments_of(D, taps_of(D), M, 8) >= MIN_SEGMENTS else 16


def _case(arm, nkb, D, fmt, M, clients=CLIENTS):
    opts = [("polyphase", 1), ("polyphase_m", M)]
    tag, not_tag = " mix=mfma", None
    if arm == "plain":
        opts += [("mix_kernel", 1), ("mix_operand_image", 0)]
        not_tag = "/img"
    elif arm == "seg":
        opts += [("mix_kernel", 1)]
        not_tag = "/img"
    elif arm == "img":
        opts += [("mix_kernel", 1), ("mix_operand_image", 1)]
        tag = " mix=mfma/img"
    elif arm == "f32":
        opts += [("mix_kernel", 3)]
        tag = " mix=mf32"
    else:
        assert arm == "stream"  # (the plan's own choice above 14 k-blocks: no mix option)
        tag = " mix=mf32"
    return Case(arm, nkb, D, taps_of(D), fmt, M, clients, blocks_of(D, M), tuple(opts), tag, not_tag)


def _table():
    out = []
    for nkb in range(1, 15):
        ms = (128,) if nkb <= 8 else ((64, 128) if nkb in NKB_ALSO_128 else (64,))
        for arm in ("plain", "seg", "img", "f32"):
            if arm == "img" and nkb > 8:
                continue
            fmts = {"plain": ("cu8", "cs16") if nkb in NKB_ALSO_CS16 else ("cu8",), "seg": ("cf32",), "img": ("cu8",),
                    "f32": ("cf32",) if nkb % 2 else ("cu8",)}[arm]
            for M in ms:
                for fmt in fmts:
                    for D in decimations(nkb):
                        out.append(_case(arm, nkb, D, fmt, M))
            if arm == "plain" and nkb in NKB_TWO_GROUPS:
                out.append(_case(arm, nkb, decimations(nkb)[0], "cu8", ms[0], CLIENTS_TWO_GROUPS))
    for D in (113, 120):
        out.append(_case("stream", 15, D, "cu8", 128))
    return out


CASES = _table()
ARMS = ("plain", "seg", "img", "f32", "stream")


def tests():
    """[(arm, nkb)]: one GPU test each, ordered so that the arms of a count -- which share oracle populations -- run together"""
    return sorted({(c.arm, c.nkb) for c in CASES}, key=lambda t: (t[1], ARMS.index(t[0])))


def cases_of(arm, nkb):
    return [c for c in CASES if (c.arm, c.nkb) == (arm, nkb)]
