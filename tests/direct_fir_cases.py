"""The case table of the direct FIR kernel's tests (no GPU, no library): which populations make the planner launch
xl_fir_kernel<CT, MODE, WIDE> (csrc/xl_kernels.hip) at every tall tile height (8, 9, 10, 12, forced by XL_EXP_H), both read widths
(16-byte reads of the window need every decimation of the launch even), both tap steps (4; 6 at heights 9 and 10) and every lane
count (64, 32, 16, 8 outputs per wave), and the calls every engine makes.  tests/test_direct_fir_cases_cpu.py holds the table's claims
against the planner itself (tests/c/direct_plan_probe.cpp) and against the grid arithmetic; tests/test_direct_fir_gpu.py runs the
table against the oracle.

Cases, classes as (D, T, clients); H is the forced height:

  even        (42, 505, 5H+3), (21, 253, 6), (7, 81, 3), (2, 7, 2), (3, 16, 1)   16-byte reads at height H (five full tiles, a tile
              of three clients, two groups, the second with two spare waves); heights 8, 4, 2, 1 beside it.  At H = 8 the class of 6
              shares the tall launch, and its odd decimation makes that launch read single samples: there the 16-byte reads at
              height 8 are those of the lanes* cases
  all_even    (42, 505, 5H+3), (22, 253, 6), (8, 81, 3), (2, 7, 2), (4, 16, 1)   `even` with every decimation even: 16-byte reads in
              every launch of every H -- at H = 8 two groups of the tall class and the class of 6 in one wide launch at 64 lanes
  odd_mixed   (21, 253, 5H+3), (42, 505, 13)                                       8-byte reads at height H, an even group beside
  short_taps  (4, 1, H+1), (3, 5, H+1), (2, 6, H+1), (5, 7, H+1), (6, 13, H+1)     T below one tap step, Tpad of 4 against 6,
              steps / 2 == 0 in the priority split
  lanes32     (300 | 301, 2401, H+1), (42, 505, 9)                                 32 outputs per wave
  lanes16     (600 | 601, 2401, H+1), (42, 505, 9)                                 16
  lanes8      (1300 | 1301, 2401, H+1), (42, 505, 9)                               8
              (the large decimation is even at H = 8, 10 and odd at 9, 12; the lane count is the launch's: the D = 42 class runs
              at it too)

Input format: cu8, cs8, cs16, cf32 rotate over (case index + height index) mod 4.

Calls (group_blocks = 3; samples per block): 32768; 5001; 3; one call of 3 x 4099; 32768; 0; 20002 -- short_taps 4096 and 2002 in
place of 32768 and 20002.  No non-zero length may be a multiple of a decimation of its case: one that is moves to the nearest length
that is not (`nearest_free_length`: distance 1 upwards, 1 downwards, 2 upwards ...).
"""
import collections

import numpy as np

import siggen

FS = 2016000
HEIGHTS = (8, 9, 10, 12)
FMTS = ("cu8", "cs8", "cs16", "cf32")
CASES = ("even", "odd_mixed", "short_taps", "lanes32", "lanes16", "lanes8", "all_even")
SPARSE_CASES = ("even", "odd_mixed", "short_taps", "lanes16")
GROUP_BLOCKS = 3
LANES = {"even": 64, "all_even": 64, "odd_mixed": 64, "short_taps": 64, "lanes32": 32, "lanes16": 16, "lanes8": 8}
LANE_D = {"lanes32": 300, "lanes16": 600, "lanes8": 1300}

# csrc, restated (tests/test_direct_fir_cases_cpu.py pins them to the headers and to the planner's output)
XL_HCAP = 16384
XL_PH_STRIDE = 16
XL_NW = 4                 # tiles per group (XL_NW_DEFAULT)
LDS_BUDGET = 160 * 1024
LAUNCH_HEIGHTS = (12, 10, 9, 8, 4, 2, 1)  # kHeights: the order of the launches, and of describe()

Class = collections.namedtuple("Class", "D T count")
Call = collections.namedtuple("Call", "S G")


def tap_step(ct):
    """xl_tap_step"""
    return 6 if ct in (9, 10) else 4


def roundup(v, m):
    return -(-v // m) * m


def needs_wide(D, T, multiple=12):
    """xl_fir_needs_wide"""
    return (7 * D + roundup(T, multiple)) * 8 > LDS_BUDGET


def lds_bytes(D, Tpad, ota):
    """xl_fir_lds_bytes_ota"""
    return ((ota - 1) * D + Tpad) * 8


def classes(case, H):
    """-> [Class]: the tall classes (8 clients and more: the launch of height H) first"""
    if case == "even":
        return [Class(42, 505, 5 * H + 3), Class(21, 253, 6), Class(7, 81, 3), Class(2, 7, 2), Class(3, 16, 1)]
    if case == "all_even":
        return [Class(42, 505, 5 * H + 3), Class(22, 253, 6), Class(8, 81, 3), Class(2, 7, 2), Class(4, 16, 1)]
    if case == "odd_mixed":
        return [Class(21, 253, 5 * H + 3), Class(42, 505, 13)]
    if case == "short_taps":
        return [Class(D, T, H + 1) for D, T in ((4, 1), (3, 5), (2, 6), (5, 7), (6, 13))]
    D = LANE_D[case] + (1 if H in (9, 12) else 0)
    return [Class(D, 2401, H + 1), Class(42, 505, 9)]


def class_height(count, H):
    """xl_build_launches: classes of fewer than 8 clients take one small tile"""
    if count >= 8:
        return H
    return 8 if count > 4 else (4 if count > 2 else (2 if count > 1 else 1))


def fmt_of(case, H):
    return FMTS[(CASES.index(case) + HEIGHTS.index(H)) % 4]


def sparse_fmt_of(case, H):
    """The sparse block needs samples that are exactly zero, and cu8 has none ((x - 127.5) / 128): the three signed formats rotate"""
    return FMTS[1 + (CASES.index(case) + HEIGHTS.index(H)) % 3]


def free_lengths(n, Ds):
    """n and the lengths around it that are no multiple of any D, nearest first (upwards first at equal distance); 0 -> 0"""
    if n == 0:
        yield 0
        return
    for d in range(0, n):
        for v in ((n + d, n - d) if d else (n,)):
            if v > 0 and all(v % D for D in Ds):
                yield v


def nearest_free_length(n, Ds):
    return next(free_lengths(n, Ds))


def calls(case, H):
    """-> [Call]: the seven calls of an engine.  The two full calls (1 and 5) must leave every tall class a partial last x-tile; a
    length that gives one of them a multiple of the lane count (short_taps, call 5: 1024 outputs at D = 4) moves on to the next
    free length."""
    full, mid = (4096, 2002) if case == "short_taps" else (32768, 20002)
    cls = classes(case, H)
    Ds = sorted({c.D for c in cls})
    out, consumed = [], 0
    for i, (S, G) in enumerate(((full, 1), (5001, 1), (3, 1), (4099, GROUP_BLOCKS), (full, 1), (0, 1), (mid, 1))):
        for v in free_lengths(S, Ds):
            if i not in (0, 4) or all(grid_outputs(consumed, c.D, v) % LANES[case] for c in cls if c.count >= 8):
                break
        out.append(Call(v, G))
        consumed += v * G
    return out


def max_input(case, H):
    """samples per block the engine is created for"""
    return max(c.S for c in calls(case, H))


def taps_of(T, j, n, D):
    """Client j of a class of n: a Hamming-windowed sinc whose cutoff follows from j, so that no two clients of a class share taps
    (a single tap has no window: its value follows from j)"""
    if T == 1:
        return np.array([(j + 1.0) / (n + 1.0)], np.float32)
    return siggen.hamming_sinc(T, (0.2 + 0.6 * (j + 1) / (n + 1)) / (2.0 * D))


def clients(case, H, tall_fc0=False):
    """-> [(class index, D, taps, fc)]: class by class.  Distinct taps and centre frequencies within a class; tall_fc0: every client of
    a tall class sits at fc = 0 (the sparse block's test)"""
    out = []
    for k, cs in enumerate(classes(case, H)):
        for j in range(cs.count):
            fc = int(-0.42 * FS + 0.84 * FS * (j + 0.5) / cs.count) + 1013 * k + 7 * j
            if tall_fc0 and cs.count >= 8:
                fc = 0
            out.append((k, cs.D, taps_of(cs.T, j, cs.count, cs.D), fc))
    return out


# ---------------------------------------------------------------------------------------------------------------
# the reference
class GapOracle:
    """pyoracle.Oracle for a filter shorter than its decimation step (T - 1 < D: the class (4, 1) of short_taps) on blocks that are no
    multiple of D.  The reference keeps `working_len - current_index` samples as history (xlating.c:76), and with T - 1 < D the window
    start of the next output lies up to D - T samples BEYOND what it holds: the count underflows and the memmove behind it is
    undefined.  Those samples lie between two windows -- no output reads them.  This wrapper hands them to the oracle as zeros at the
    end of the call that would underflow and drops them from the next blocks when they arrive, so the oracle's counter ends at 0: the
    same oracle and arithmetic, the same outputs in the same calls (an output belongs to the call that holds its newest sample), one
    renormalisation per call with output."""

    def __init__(self, D, taps, fc, fs, max_input, sum_mode=0):
        from pyoracle import Oracle
        self.o, self.D, self.T, self.skip = Oracle(D, taps, fc, fs, max_input + 2 * D, sum_mode=sum_mode), D, len(taps), 0

    def process(self, fmt, x):
        x = np.asarray(x)
        drop = min(self.skip, x.size // 2)
        self.skip -= drop
        x = x[2 * drop:]
        if x.size == 0:
            return np.zeros(0, np.complex64)
        avail = self.o.history + x.size // 2
        if avail > self.T - 1:
            pos = roundup(avail - (self.T - 1), self.D)  # window start of the next call's first output
            if pos > avail:
                self.skip = pos - avail
                x = np.concatenate([x, np.zeros(2 * self.skip, x.dtype) + (128 if fmt == "cu8" else 0)]).astype(x.dtype)
        return self.o.process(fmt, x)

    @property
    def phase(self):
        return self.o.phase

    def close(self):
        self.o.close()


def make_oracle(D, taps, fc, max_input, sum_mode=0):
    """the reference of one client; max_input in scalar elements, as the oracle takes it"""
    from pyoracle import Oracle
    return (GapOracle if len(taps) - 1 < D else Oracle)(D, taps, fc, FS, max_input, sum_mode=sum_mode)


# ---------------------------------------------------------------------------------------------------------------
# the plan the table claims (xl_build_launches, restated)
def expected_launches(class_list, H):
    """class_list: [(D, T, count)] of classes that are one direct class each -> {ct: dict(groups, ota, wide, tpads, tiles)} with
    tiles = per group the clients of each tile, groups in class order"""
    out = {}
    for D, T, count in class_list:
        ct = class_height(count, H)
        L = out.setdefault(ct, dict(groups=0, ota=64, wide=True, tpads=[], tiles=[], Ds=[]))
        fill = [min(ct, count - i) for i in range(0, count, ct)]
        for g in range(0, len(fill), XL_NW):
            L["tiles"].append(fill[g:g + XL_NW])
            L["tpads"].append(roundup(T, tap_step(ct)))
            L["Ds"].append(D)
        L["wide"] = L["wide"] and D % 2 == 0
    for ct, L in out.items():
        L["groups"] = len(L["tiles"])
        for ota in (64, 32, 16, 8):
            if max(lds_bytes(D, tp, ota) for D, tp in zip(L["Ds"], L["tpads"])) <= LDS_BUDGET:
                L["ota"] = ota
                break
        else:
            raise AssertionError("no lane count fits")
    return out


def describe_direct(class_list, H):
    """the text of describe() behind "direct:" for these classes"""
    exp = expected_launches(class_list, H)
    text = ""
    for ct in LAUNCH_HEIGHTS:
        if ct in exp:
            L = exp[ct]
            text += " h%d x %d groups" % (ct, L["groups"])
            if L["ota"] < 64:
                text += " lanes%d" % L["ota"]
            if not L["wide"]:
                text += " reads8"
    return text


# ---------------------------------------------------------------------------------------------------------------
# xl_grid.h, restated
def grid_j0(consumed, D):
    return (-consumed) % D


def grid_outputs(consumed, D, n):
    """XlDyn::K of a call of n samples in all"""
    j0 = grid_j0(consumed, D)
    return (n - j0 + D - 1) // D if n > j0 else 0


def grid_mstart(j0, D, S, g):
    n = g * S
    return (n - j0 + D - 1) // D if n > j0 else 0


ALL_CALLS = (0, 1, 2, 3, 4, 5, 6)
FLAT_CALLS = (0, 1, 3)     # test_flat_priority_loop: calls 1, 2 and 4
ROLE_CALLS = (0, 1, 3, 4)  # test_role_inside_the_tall_launch: calls 1, 2, 4 and 5
FLAT_CASES = ("even", "short_taps")
ROLE_CASE = "even"


def walk(case, H, which=ALL_CALLS):
    """-> [(Call, consumed before the call)] of an engine that makes the calls `which` of the case"""
    out, consumed = [], 0
    for c in (calls(case, H)[i] for i in which):
        out.append((c, consumed))
        consumed += c.S * c.G
    return out


# ---------------------------------------------------------------------------------------------------------------
# inputs
def call_input(fmt, seed, n):
    """n samples of noise in the engine's format (cf32: sixteen-bit values / 32768, exact in every consumer)"""
    if n == 0:
        return np.zeros(0, {"cu8": np.uint8, "cs8": np.int8, "cs16": np.int16, "cf32": np.float32}[fmt])
    if fmt == "cu8":
        return siggen.xs_u8(seed, 2 * n)
    if fmt == "cs8":
        return siggen.xs_s8(seed, 2 * n)
    if fmt == "cs16":
        return siggen.xs_s16(seed, 2 * n)
    return (siggen.xs_s16(seed, 2 * n).astype(np.float32) / np.float32(32768)).astype(np.float32)


def sparse_spacing(case, H):
    """samples between two impulses: more than the largest T of the case, and odd, so that the impulses walk through the residues of
    the even decimations"""
    t = max(c.T for c in classes(case, H)) + 6
    return t + 1 - t % 2


def sparse_input(case, H):
    """-> (fmt, block): one block of max_input samples, zero but for impulses `sparse_spacing` apart whose real and imaginary parts
    are powers of two of either sign"""
    fmt, n, step = sparse_fmt_of(case, H), max_input(case, H), sparse_spacing(case, H)
    bits = {"cs8": 7, "cs16": 15, "cf32": 15}[fmt]
    x = np.zeros(2 * n, np.int32)
    for k, pos in enumerate(range(3, n, step)):
        x[2 * pos] = (1 << (k % bits)) * (1 if k % 3 else -1)
        x[2 * pos + 1] = (1 << ((3 * k + 2) % bits)) * (-1 if k % 2 else 1)
    if fmt == "cs8":
        return fmt, x.astype(np.int8)
    if fmt == "cs16":
        return fmt, x.astype(np.int16)
    return fmt, (x.astype(np.float32) / np.float32(32768)).astype(np.float32)
