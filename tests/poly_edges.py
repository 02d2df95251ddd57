"""The call-length arithmetic of the polyphase overlap-save path, restated, and the call lengths chosen from it (no GPU, no library).

xl_call_poly_class (xl_batch.cpp) cuts a call of G blocks of S samples into segments of V shared points and passes of XLP_SEG
segments; everything that decides where the call's last outputs come from is a function of its length:

    Kq     = ceil(S G / D) + 1            shared points (xl_grid.h: xl_merge_points)
    V      = M - A + 1,  A = ceil((T + dmax) / D)     (xl_plan.cpp: dmax = the largest grid offset of a member against the reference)
    nseg   = ceil(Kq / V),   passes = ceil(nseg / 16)
    use_poly = the largest K of the call >= 2 * XLP_M_MAX = 512         (xl_call_begin; below it the call runs on the direct kernel)
    nseg_cap = (cap_samples / D + 2 + V - 1) / V + 1,  cap_samples = max_input * group_blocks      (xl_poly_sync_device)

tests/test_poly_edges_cpu.py pins these restatements to xl_grid.h and asserts that the sequences below hold every edge they are
built for, call by call; tests/test_poly_edges_gpu.py runs them against the oracle.

Every engine follows one protocol (`walk` restates its bookkeeping):
  * cohort A (NA clients, and the clients of a second class if the shape has one) joins before call 0, a one-block call whose length
    is r mod D, 0 < r < D / 2 -- small enough that ceil((T + r) / D) = ceil(T / D): V does not depend on the offset;
  * cohort B (NB clients) joins behind call 0.  During call 1 it is inside its zero history and forms a class of its own; from call
    2 on both cohorts are ONE class with two grid offsets: the reference is cohort A's grid (the candidate with the smallest largest
    delay, xl_poly_form_classes), cohort B's delay is delta = r;
  * client LEAVER of cohort A leaves behind call LEAVE_AFTER: a vacant column between live ones.
"""
import collections

XL_PH_STRIDE = 16   # xl_grid.h: outputs per phase-table entry = points per phase group of the inverse launch
XLP_SEG = 16        # xl_polyphase.h: segments per pass
XLP_M_MAX = 256     # xl_polyphase.h
MIN_POLY_OUTPUTS = 2 * XLP_M_MAX
XLP_FWD_GROUP_MIN_WGS = 96  # xl_polyphase.h: a cf32 forward launch of at least this many grouped workgroups runs groups of branches

NA, NB = 18, 17     # clients per cohort of a main class: 35, 34 after the leave -- more than one inverse tile column group of 32
LEAVER = 5          # index in cohort A
LEAVE_AFTER = 3     # ... leaves behind this call
N2 = 3              # clients of a second class


# ---------------------------------------------------------------------------------------------------------------
# xl_grid.h / xl_batch.cpp / xl_plan.cpp, restated
def grid_j0(consumed, D):
    """call-local position of output 0's newest sample for a client that has seen `consumed` samples (xl_grid_dyn)"""
    return (-consumed) % D


def grid_outputs(consumed, D, S, G):
    """XlDyn::K"""
    j0, N = grid_j0(consumed, D), S * G
    return (N - j0 + D - 1) // D if N > j0 else 0


def grid_mstart(j0, D, S, g):
    """index of the first output of block g (xl_grid_mstart)"""
    n = g * S
    return (n - j0 + D - 1) // D if n > j0 else 0


def merge_j0(j0_ref, delta, D):
    j = j0_ref + delta
    return j - D if j >= D else j


def merge_shift(j0_ref, delta, D):
    """q - k of a member: its output k is the shared point k + shift"""
    return 0 if j0_ref + delta >= D else 1


def merge_points(D, S, G):
    return (S * G + D - 1) // D + 1


def merge_outputs(j0_ref, delta, D, S, G):
    N = S * G
    Ka = N // D
    return Ka + (1 if merge_j0(j0_ref, delta, D) < N - Ka * D else 0)


def taps_per_branch(T, D, dmax=0):
    return (T + dmax + D - 1) // D


def valid_points(M, T, D, dmax=0):
    """V = M - A + 1"""
    return M - taps_per_branch(T, D, dmax) + 1


def segments(Kq, V):
    return (Kq + V - 1) // V


def passes(nseg):
    return (nseg + XLP_SEG - 1) // XLP_SEG


def use_poly(max_k):
    return max_k >= 2 * XLP_M_MAX


def nseg_cap(cap_samples, D, V):
    return (cap_samples // D + 2 + V - 1) // V + 1


def forward_grouped(fmt, D, M, nseg):
    """xlp_launch_forward: cf32 streams run (pass, group of 4 adjacent branches -- 2 at M = 256) per workgroup from 96 such workgroups on"""
    nb = 2 if M == 256 else 4
    return fmt == "cf32" and passes(nseg) * ((D + nb - 1) // nb) >= XLP_FWD_GROUP_MIN_WGS


# ---------------------------------------------------------------------------------------------------------------
# shapes
Shape = collections.namedtuple("Shape", "name fmt fs D T cutoff r Ms second")
# second: (D2, T2, cutoff2) of a class of N2 clients beside the main one, or None

SHAPES = {
    "A": Shape("A", "cu8", 384000, 8, 17, 0.05, 3, (64, 128, 256), (400, 961, 0.001)),
    "B": Shape("B", "cf32", 384000, 8, 17, 0.05, 3, (64, 128), (400, 961, 0.001)),
    "C": Shape("C", "cf32", 10000000, 100, 257, 0.004, 37, (64, 128), None),
    "D": Shape("D", "cu8", 9600000, 200, 481, 0.002, 41, (128,), None),
}
# Shape C has no second class of nseg = 1, Kq <= 16 (case 4): its calls cross the threshold at 512 * 100 samples, where Kq <= 16 needs
# a decimation of 51200 / 14 > 3657 -- a wide client (xl_wide.h), which no polyphase class holds.  Shape D runs cases 1, 3 and 6.
# The forward launch takes its grouped form from 96 workgroups of four branches on: with D = 8 that would be 48 passes (shape B never gets
# there), with D = 100 it is four passes -- shape C's sequence "long", whose calls have 49 .. 65 segments.
SEQUENCES_OF = {"A": ("edges", "thresh", "g2", "g3"), "B": ("edges", "thresh", "g2", "g3"), "C": ("edges", "thresh", "g2", "g3", "long"),
                "D": ("edges",)}
SEQUENCE_NAMES = ("edges", "thresh", "g2", "g3", "long")

Call = collections.namedtuple("Call", "name S G variant quiet")
# quiet (cf32 shapes): "tail" = the call's last two segments, "head" = its first segment, lie 2^10 below the rest of the call


def _call(name, n_total, G=1, variant="optimized", quiet=None):
    assert n_total % G == 0, (name, n_total, G)
    return Call(name, n_total // G, G, variant, quiet)


def _len(D, Kq, rem):
    """samples of a call with Kq shared points whose length is rem mod D: Kq = N / D + 1 (rem = 0), floor(N / D) + 2 (else)"""
    assert 0 <= rem < D
    return D * (Kq - 1) if rem == 0 else D * (Kq - 2) + rem


def sequences(shape, M):
    """-> {sequence name: [Call, ...]}; the engine of a sequence has max_input = its largest S and group_blocks = its largest G."""
    D, r = shape.D, shape.r
    V = valid_points(M, shape.T, D, r)
    k0 = -(-(MIN_POLY_OUTPUTS + 8) // V)      # segments of a call just above the threshold
    full = XLP_SEG * V                        # the shared points of one full pass
    seqs = {}
    # ---- one block per call: Kq and nseg residues, the capacity call (cases 1, 2, 3, 6, 8)
    seqs["edges"] = [
        _call("warm", _len(D, k0 * V + 2, r)),                       # Kq = 2 mod V; the first offset: r mod D
        _call("full16", _len(D, full, 0)),                           # Kq = 16 V: one full pass (cohort B's first call)
        _call("one-mult", _len(D, full + 1, 0)),                     # Kq = 16 V + 1, S = 0 mod D: the last pass is one segment of one
                                                                     # point, owned by the members of shift 1 (= capacity less a sample)
        _call("one-rem", _len(D, full + 1, 2), quiet="tail"),        # Kq = 16 V + 1, S = 2 mod D: nobody's point; K and K + 1 outputs
        _call("native", _len(D, k0 * V + 9, 1), variant="native"),   # the bit-exact call
        _call("vm1", _len(D, full - 1, 3), quiet="tail"),            # Kq = V - 1 mod V, nseg = 16
        _call("n15", _len(D, 15 * V, 5), quiet="head"),              # Kq = 0 mod V, nseg = 15
        _call("cap", D * full + 1),                                  # S = max_input: Kq = 16 V + 2, nseg = 17 = nseg_cap - 1
    ]
    # ---- the threshold (cases 4, 5): the largest K of the call 512 and 511, a second class of a fraction of one segment
    seqs["thresh"] = [
        _call("warm", D * 600 + r),
        _call("k520", D * 520),
        _call("k512", D * 512),                                      # every member owns 512 outputs: polyphase
        _call("k511", D * 511),                                      # every member owns 511: the direct kernel
        _call("k512-some", D * 511 + 1),                             # cohort B owns 512, cohort A 511: polyphase
        _call("native", D * 515 + 2, variant="native"),
        _call("k512-again", D * 512, quiet="tail"),
        _call("k530", D * 530, quiet="head"),
    ]
    # ---- calls of 2 and of 3 blocks of n D samples each (case 7): the first output of an inner block g is output g n of every member,
    # the shared point g n + shift; cohort A has shift 1, cohort B shift 0 throughout (every length behind call 0 is 0 mod D)
    k = -(-(MIN_POLY_OUTPUTS // 2 + 4) // V)
    for G in (2, 3):
        seqs["g%d" % G] = [
            _call("warm", D * k * V + r),                            # (one block, below the threshold: the direct kernel)
            _call("first", G * D * (k * V + 5), G),
            _call("sV", G * D * (k * V), G),                         # shift 0: point 0 of a segment; shift 1: point 1
            _call("sV-1", G * D * (k * V - 1), G),                   # shift 0: point V - 1; shift 1: point 0
            _call("sV+1", G * D * (k * V + 1), G),                   # shift 0: point 1
            _call("native", G * D * (k * V + 7), G, variant="native"),
            _call("sV-2", G * D * (k * V - 2), G, quiet="tail"),     # shift 1: point V - 1
            _call("sV+16", G * D * (k * V + 16), G, quiet="head"),   # shift 0: the second phase group (capacity)
            _call("sV+15", G * D * (k * V + 15), G),                 # shift 1: the second phase group
            _call("cap-1", G * (D * (k * V + 16) - 1), G),           # capacity less a sample per block
        ]
    # ---- four and five passes per call (cf32, D = 100: the forward launch in groups of four branches): the one-point last pass, full passes
    seqs["long"] = [
        _call("warm", _len(D, k0 * V + 2, r)),
        _call("first", _len(D, 3 * full + 3 * V + 3, 0)),            # (cohort B's first call; four passes)
        _call("p4-one-mult", _len(D, 3 * full + 1, 0)),              # nseg = 49: the fourth pass is one segment of one point (cohort A's)
        _call("p4-one-rem", _len(D, 3 * full + 1, 2), quiet="tail"), # ... nobody's
        _call("p4-full", _len(D, 4 * full, 3), quiet="head"),        # nseg = 64: four full passes
        _call("native", _len(D, k0 * V + 9, 1), variant="native"),
        _call("cap-1", D * 4 * full),                                # nseg = 65: the fifth pass is one segment of one point
        _call("cap", D * 4 * full + 1),                              # S = max_input: Kq = 64 V + 2, five passes
    ]
    return seqs


def engine_limits(calls):
    """-> (max_input in samples, group_blocks) an engine of the sequence is created with: no larger than its calls need"""
    return max(c.S for c in calls), max(c.G for c in calls)


Rec = collections.namedtuple("Rec", "call merged consumed_a consumed_b j0_ref delta_b shift_a shift_b k_a k_b max_k poly Kq nseg passes "
                                    "last_points Kq2 nseg2")


def walk(shape, M, calls, second=False):
    """The bookkeeping of the main class over a sequence (second: beside a second class that joined with cohort A) -> [Rec per call].  consumed_b / k_b are None in call 0; `merged`: both cohorts
    are one class (from call 2 on), whose reference grid is cohort A's; before that each cohort has its own grid (shift 1, delta 0)."""
    D = shape.D
    V = valid_points(M, shape.T, D, shape.r)
    ca, cb, out = 0, None, []
    for i, c in enumerate(calls):
        if i == 1:
            cb = 0
        merged = i >= 2
        j0_ref = grid_j0(ca, D)
        delta_b = (grid_j0(cb, D) - j0_ref) % D if cb is not None else None
        k_a = grid_outputs(ca, D, c.S, c.G)
        k_b = grid_outputs(cb, D, c.S, c.G) if cb is not None else None
        max_k = max(k_a, k_b or 0)
        Kq = merge_points(D, c.S, c.G)
        nseg = segments(Kq, V)
        Kq2 = nseg2 = None
        if second:
            D2, T2 = shape.second[0], shape.second[1]
            Kq2 = merge_points(D2, c.S, c.G)
            nseg2 = segments(Kq2, valid_points(M, T2, D2))
            max_k = max(max_k, grid_outputs(ca, D2, c.S, c.G))
        out.append(Rec(c, merged, ca, cb, j0_ref, delta_b, 1, merge_shift(j0_ref, delta_b, D) if merged else 1, k_a, k_b, max_k,
                       c.variant == "optimized" and use_poly(max_k), Kq, nseg, passes(nseg), Kq - (nseg - 1) * V, Kq2, nseg2))
        ca += c.S * c.G
        if cb is not None:
            cb += c.S * c.G
    return out


def inner_block_points(shape, M, rec):
    """{(shift, shared point mod V)} of the first outputs of the inner blocks (g = 1 .. G - 1) of a merged call, both cohorts"""
    D, c = shape.D, rec.call
    V = valid_points(M, shape.T, D, shape.r)
    out = set()
    for consumed, shift in ((rec.consumed_a, rec.shift_a), (rec.consumed_b, rec.shift_b)):
        for g in range(1, c.G):
            out.add((shift, (grid_mstart(grid_j0(consumed, D), D, c.S, g) + shift) % V))
    return out


def quiet_span(shape, M, rec):
    """-> (first, last + 1) call-local samples of the quiet passage of a call, or None.  Segment s of a call evaluates the shared points
    s V .. s V + V - 1 from M D samples that begin T - 1 + D - j0_ref samples in front of sample s V D; "tail" is quiet from one more
    decimation step in front of segment nseg - 2 to the end of the call, so the last two segments hold nothing louder; "head" from the
    call's first sample (behind a "tail" call, whose end is the history) to a step behind the end of segment 0."""
    c, D = rec.call, shape.D
    V = valid_points(M, shape.T, D, shape.r)
    N = c.S * c.G
    if c.quiet == "tail":
        return max(0, (rec.nseg - 2) * V * D - shape.T - 2 * D), N
    if c.quiet == "head":
        return 0, min(N, (M + 1) * D)
    return None
