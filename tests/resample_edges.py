"""The tile arithmetic of the two resampler banks, restated, and the streams chosen from it (no GPU, no library).

Both banks' kernels (xl_resample.hip, xl_resample_q15.hip) cut a feed's new outputs into tiles of XL_RS_TILE consecutive outputs of one
stream, one workgroup per tile (xl_resample_dev.h: xl_rs_tile).  A tile of nv outputs whose first output has phase pt reads a window of

    span = (nv - 1) * (M / L) + (pt + (nv - 1) * (M % L)) / L + Q          input samples

When span <= XL_RS_LDS_SPAN (the Q15 bank: XL_RSQ_LDS_SPAN) the window is staged in LDS, the part below the feed's first sample from
the stream's carry; a wider window is read in place, every thread choosing between carry and source by its own index.  The two are
separate code for one sum, and which of them a tile takes depends on where the feed begins: pt is a function of the stream position.

`cut` restates xl_resample_cut.h and `tile_paths` restates xl_rs_tile.  THIS IS A RESTATEMENT, READ AGAINST xl_resample_dev.h: the
device function cannot be compiled for the host, and nothing in the library or the kernels counts which branch ran.  What holds the
restatement to the code is (a) tests/test_resample_edges_cpu.py, which compares `cut` with xl_resample_cut.h compiled by gcc for every
(case, piece) below, and (b) the constants, which are parsed from the two headers here, never copied: a change of XL_RS_TILE or of a
span limit makes the condition tests of test_resample_edges_cpu.py fail instead of silently moving a case off its edge.  The GPU tests
(tests/test_resample_edges_gpu.py) feed exactly the piece lists whose paths the CPU tests assert.

The case table: (name, L, M, taps, N, pieces, banks); `pieces` maps a name to the list of feed lengths, "whole" and "edge" (the existing
tests' [Q - 1, 1, 300, 4097, rest]) always, and "flip" where another split changes the path of the same outputs."""
import collections
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sdr-server_amd", "csrc")


def constants():
    """XL_RS_TILE, XL_RS_LDS_SPAN (xl_resample.h), XL_RSQ_LDS_SPAN, XL_RSQ_LDS_TAPS (xl_resample_q15.h), as the headers define them"""
    out = {}
    for header, names in (("xl_resample.h", ("XL_RS_TILE", "XL_RS_LDS_SPAN")), ("xl_resample_q15.h", ("XL_RSQ_LDS_SPAN", "XL_RSQ_LDS_TAPS"))):
        text = open(os.path.join(CSRC, header)).read()
        for name in names:
            m = re.findall(r"^#define\s+%s\s+(\d+)u\b" % name, text, re.M)
            assert len(m) == 1, (header, name, m)
            out[name] = int(m[0])
    return out


CONST = constants()
TILE = CONST["XL_RS_TILE"]


# ---------------------------------------------------------------------------------------------------------------
# xl_resample_cut.h and xl_resample_dev.h, restated (Python integers)
def produced(L, M, P):
    return (P * L + M - 1) // M


def cut(L, M, Q, P0, n):
    """xl_resample_cut: what samples P0 .. P0 + n - 1 bring -> (m_first, count, n_first relative to the feed, p_first)"""
    t = produced(L, M, P0) * M
    return t // M, produced(L, M, P0 + n) - t // M, t // L - P0, t % L


def tile_paths(L, M, Q, P0, n, span_limit):
    """xl_rs_tile over every workgroup of a feed of n samples at stream position P0 -> [(nv, span, "lds" | "mem") per tile]"""
    m_first, count, n_first, p_first = cut(L, M, Q, P0, n)
    Mq, Mr = M // L, M % L
    out = []
    for k0 in range(0, count, TILE):
        nv = min(TILE, count - k0)
        pt = (p_first + k0 * M) % L
        span = (nv - 1) * Mq + (pt + (nv - 1) * Mr) // L + Q
        out.append((nv, span, "lds" if span <= span_limit else "mem"))
    return out


def feed_paths(L, M, Q, pieces, span_limit):
    """tile_paths of every feed of a piece list, from stream position 0 -> [[(nv, span, path) per tile] per feed]"""
    pos, out = 0, []
    for c in pieces:
        out.append(tile_paths(L, M, Q, pos, c, span_limit))
        pos += c
    return out


# ---------------------------------------------------------------------------------------------------------------
# the cases
def windowed_sinc(n, L, cutoff):
    """tests/test_resample_gpu.py's: a float32 low-pass of n taps at `cutoff` (cycles per sample of the upsampled grid), gain L"""
    k = np.arange(n) - (n - 1) / 2
    h = np.sinc(2 * cutoff * k) * np.hamming(n)
    return (h * (L / h.sum())).astype(np.float32)


def split(N, sizes):
    """N cut into the given sizes, the last piece taking what is left"""
    out, left = [], N
    for s in sizes:
        s = min(int(s), left)
        out.append(s)
        left -= s
    out.append(left)
    return out


Case = collections.namedtuple("Case", "name L M taps N pieces banks")
M_MAX = 2 ** 31 - 1  # the largest M a bank admits (and a prime)


def _case(name, L, M, taps, N, banks, flip=None):
    Q = -(-taps.size // L)
    pieces = collections.OrderedDict(whole=[N], edge=split(N, [Q - 1, 1, 300, 4097]))
    if flip is not None:
        pieces["flip"] = list(flip)
    assert all(sum(p) == N for p in pieces.values()), name
    taps.setflags(write=False)
    return Case(name, L, M, taps, N, pieces, banks)


def _cases():
    yield _case("1/16 Q16", 1, 16, windowed_sinc(16, 1, 0.45 / 16), 20000, "fq")          # span exactly at the limit: LDS
    yield _case("1/16 Q17", 1, 16, windowed_sinc(17, 1, 0.45 / 16), 20000, "fq")          # one past it; the short last tile in LDS
    yield _case("1/40 Q64", 1, 40, windowed_sinc(64, 1, 0.45 / 40), 30000, "f")           # (the Q15 bank's own tests have it)
    yield _case("3/50 Q40", 3, 50, windowed_sinc(120, 3, 0.45 / 50), 30000, "fq")         # M % L != 0 in place
    # M / L = 15, M % L = 1: from phase 0 a full tile spans 255 * 15 + 255 / 4 + 208 = 4096, from phase 1 on one more
    yield _case("4/61 Q208", 4, 61, windowed_sinc(832, 4, 0.45 / 61), 30000, "fq", flip=[1, 29999])
    yield _case("5/81 Q1000", 5, 81, windowed_sinc(5000, 5, 0.45 / 81), 30000, "q")       # the tap table in place as well
    # (its phases have sum |c| > 65535, so it sums in 64 bits; at half the gain the same table and window take the 32-bit sums)
    yield _case("5/81 Q1000 half", 5, 81, windowed_sinc(5000, 5, 0.45 / 81) * np.float32(0.5), 30000, "q")
    rng = np.random.default_rng(40)
    yield _case("1/40 wide", 1, 40, (rng.choice([-0.99, 0.99], 64)).astype(np.float32), 30000, "q")
    rng = np.random.default_rng(31)
    # (multiples of 2^-15 in [-1, 1): the Q15 bank takes the same taps)
    yield _case("4096/(2^31-1) Q3", 4096, M_MAX, (rng.integers(-32768, 32768, 12288) / 32768.0).astype(np.float32), 1300000, "fq")
    yield _case("1/(2^31-1) Q5", 1, M_MAX, windowed_sinc(5, 1, 0.2), 6000, "fq", flip=[1000, 5000])


CASES = list(_cases())
CASE = {c.name: c for c in CASES}
FLOAT_CASES = [c.name for c in CASES if "f" in c.banks]
Q15_CASES = [c.name for c in CASES if "q" in c.banks]


def taps_per_phase(case):
    return -(-case.taps.size // case.L)


def span_limit(bank):
    return CONST["XL_RS_LDS_SPAN" if bank == "f" else "XL_RSQ_LDS_SPAN"]


# ---------------------------------------------------------------------------------------------------------------
# the poisoned sample
def readers(L, M, Q, N, n_bad):
    """the outputs whose window holds input n_bad: {m : n_m - (Q - 1) <= n_bad <= n_m} -> (their indices m, their n_m), ascending"""
    nout = produced(L, M, N)
    lo = -(-(n_bad * L) // M)  # the first m with n_m = m M // L >= n_bad
    ms = [m for m in range(lo, nout) if m * M // L <= n_bad + Q - 1]
    return ms, [m * M // L for m in ms]


POISON = (("mem", 7), ("lds", 7))  # (the path of the readers' tiles, the seed of the position)


def poison_plan(case, where, seed):
    """a seeded input position with at least two readers, and a split [B, N - B] that cuts between them -- the first reader takes the
    sample from the source in the first feed, the others from the carry in the second -- such that the readers' tiles take the
    path `where` both when the stream is fed whole and in the second feed of the split -> (n_bad, [B, N - B])"""
    L, M, N, Q = case.L, case.M, case.N, taps_per_phase(case)
    tiles = tile_paths(L, M, Q, 0, N, span_limit("f"))
    rng = np.random.default_rng(seed)
    for _ in range(1000):
        n_bad = int(rng.integers(Q, N - Q))
        ms, ns = readers(L, M, Q, N, n_bad)
        if len(ms) < 2 or any(tiles[m // TILE][2] != where for m in ms):
            continue
        B = ns[1]
        if tile_paths(L, M, Q, B, N - B, span_limit("f"))[0][2] == where:
            return n_bad, [B, N - B]
    raise AssertionError((case.name, where))
