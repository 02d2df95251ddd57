"""Shapes and inputs shared by tests/test_q15_extremes_cpu.py (which pins them on the CPU) and tests/test_q15_extremes_gpu.py
(which runs them through the HIP kernels): full-scale blocks that drive the Q15 family's saturating lines, and windows long enough
for the shifted sum to leave the int32 range."""
import numpy as np

import siggen
from pyoracle import Oracle

FS = 2016000
MAXIN = 65536          # elements per block (32768 samples)
FMTS = ("cu8", "cs8", "cs16")
NPDT = {"cu8": np.uint8, "cs8": np.int8, "cs16": np.int16}
FMT_MIN = {"cu8": 0, "cs8": -128, "cs16": -32768}
FMT_MAX = {"cu8": 255, "cs8": 127, "cs16": 32767}
SQUARE_PERIOD = 800    # samples


def _lpf(gain, cutoff, tw, ntaps):
    code, t = Oracle.lpf(gain, FS, cutoff, tw)
    assert code == 0 and t.size == ntaps, (code, None if t is None else t.size)
    return t


_cache = {}


def taps(name):
    """"d42": 505 taps, gain 1 (the server's own filter);  "d21": 253 taps, gain 2;  "d7": 81 taps, gain 1;  "edge7": 7 explicit
    taps holding -1.0 and the largest float32 below 1.0 (Q15: -32768 and 32767);  "even16": 16 explicit taps (an even count: the
    reference's reversal leaves the central pair in place)"""
    if name not in _cache:
        if name == "d42":
            t = _lpf(1.0, 24000, 9600, 505)
        elif name == "d21":
            t = _lpf(2.0, 48000, 19200, 253)
        elif name == "d7":
            t = _lpf(1.0, 144000, 60000, 81)
        elif name == "edge7":
            t = np.array([-1.0, np.nextafter(np.float32(1.0), np.float32(0.0)), 0.25, -1.0, np.nextafter(np.float32(1.0), np.float32(0.0)),
                          -0.5, 0.125], np.float32)
        elif name == "even16":
            t = (np.random.default_rng(16).uniform(-0.9, 0.9, 16)).astype(np.float32)
        else:
            raise KeyError(name)
        _cache[name] = t
    return _cache[name]


SHAPE_D = {"d42": 42, "d21": 21, "d7": 7, "edge7": 2, "even16": 3}
STOP_BAND = (-250000, 600000)
FC_D42 = (0, 1234, -1234, 40000, -40000) + STOP_BAND

# the saturation engine: (shape, fc) per client; classes of 13, 6, 3, 2 and 1 clients
SAT_CLIENTS = [("d42", FC_D42[c % len(FC_D42)]) for c in range(13)] + \
              [("d21", fc) for fc in (0, 1234, -1234, 40000, -40000, -250000)] + \
              [("d7", fc) for fc in (1234, 0, -40000)] + \
              [("edge7", fc) for fc in (0, 1234)] + \
              [("even16", 345678)]
# the tile-height engine: one class of 25 (a partial last tile at every height) and classes of 6, 3, 2 and 1 (heights 8, 4, 2, 1)
HEIGHT_CLIENTS = [("d42", FC_D42[c % len(FC_D42)] + 3 * (c // len(FC_D42))) for c in range(25)] + SAT_CLIENTS[13:]
SINGLE_SHAPES = [("d42", 1234), ("d21", -40000), ("d7", 40000)]


def block(kind, fmt, n, seed=0):
    """n elements (I, Q interleaved) of: "square" -- both components at the format's maximum for half a period, at its minimum for
    the other half (the phase of the wave set by seed); "min" / "max" -- constant; "noise" -- siggen's xorshift stream"""
    dt = NPDT[fmt]
    if kind == "noise":
        return {"cu8": siggen.xs_u8, "cs8": siggen.xs_s8, "cs16": siggen.xs_s16}[fmt](0x915 + seed, n)
    if kind == "min":
        return np.full(n, FMT_MIN[fmt], dt)
    if kind == "max":
        return np.full(n, FMT_MAX[fmt], dt)
    assert kind == "square"
    s = (np.arange((n + 1) // 2) + 37 * seed) % SQUARE_PERIOD < SQUARE_PERIOD // 2
    return np.repeat(np.where(s, FMT_MAX[fmt], FMT_MIN[fmt]), 2)[:n].astype(dt)


KINDS = ("noise", "square", "min", "max")

# the saturation engine's calls: (blocks per call, elements per block, kind of each block)
SAT_CALLS = [(1, MAXIN, ("square",)), (1, MAXIN, ("noise",)), (1, MAXIN, ("min",)), (1, MAXIN, ("max",)),
             (3, 30002, ("square", "max", "noise")), (1, 2, ("square",))]
SINGLE_CALLS = [(MAXIN, "square"), (MAXIN, "min"), (20002, "max"), (MAXIN, "noise"), (2, "square"), (40000, "square"), (MAXIN, "noise")]


def call_input(fmt, k, G, n, kinds):
    """the G blocks of call k, back to back"""
    return np.concatenate([block(kind, fmt, n, seed=10 * k + g) for g, kind in enumerate(kinds)])


# ---- windows long enough for the shifted sum to leave the int32 range (engine option max_window; the wide kernel)
WRAP_FMTS = ("cs16", "cs8")
WRAP_D = 1000
WRAP_TAP = 0.9999
WRAP_CASES = [("below", 65000, 0), ("t65700", 65700, 0), ("t70000", 70000, 0), ("t70000_fc500", 70000, 500)]
WRAP_SAMPLES = 70000 + 5000
WRAP_MAX_WINDOW = 131072
# I and Q of each block: constants at the format's extremes, then -- for the client at fc = 500, whose rotated taps cancel over
# any constant -- a full-scale square tone at +500 Hz (the sign of cos and of sin) and its negative
WRAP_BLOCKS = (("max", "zero"), ("min", "zero"), ("max", "max"), ("tone+", "tone+"), ("tone-", "tone-"))
WRAP_TONE = 500


def wrap_taps(T):
    return np.full(T, WRAP_TAP, np.float32)


def wrap_block(fmt, b, samples=WRAP_SAMPLES):
    x = np.empty((samples, 2), NPDT[fmt])
    ang = 2.0 * np.pi * WRAP_TONE / FS * np.arange(samples)
    for c, kind in enumerate(WRAP_BLOCKS[b]):
        if kind.startswith("tone"):
            up = ((np.cos(ang) if c == 0 else np.sin(ang)) >= 0.0) == (kind == "tone+")
            x[:, c] = np.where(up, FMT_MAX[fmt], FMT_MIN[fmt])
        else:
            x[:, c] = {"max": FMT_MAX[fmt], "min": FMT_MIN[fmt], "zero": 0}[kind]
    return x.reshape(-1)


def wrap_reachable(fmt, T):
    """(high, low) for the clients at fc = 0: whether a full-scale constant input can push sum >> 15 past 2^31 - 1 / below -2^31 with T taps of WRAP_TAP --
    plain arithmetic on the quantised tap and the format's extremes (cs8's maximum is 127 << 8 = 32512, not 32767)"""
    q = int(np.float32(WRAP_TAP) * np.float32(32768.0))
    top = FMT_MAX[fmt] << (8 if fmt == "cs8" else 0)
    bot = FMT_MIN[fmt] << (8 if fmt == "cs8" else 0)
    return (T * q * top) >> 15 > 0x7FFFFFFF, (T * q * bot) >> 15 < -0x80000000


# ---- the recorded reference run (tests/golden/q15_wrap_t65700.npz, made by tests/golden/make_golden.py)
GOLDEN_WRAP = dict(D=WRAP_D, T=65700, fc=0, fmt="cs16", samples=65700 + 5000, block=0)

# ---- mixing families on one engine: blocks whose length every decimation divides (the history before a call is then the T - 1
# samples before it, whatever the client)
MIX_N = 2 * 42 * 780   # elements: 32760 samples
MIX_CLIENTS = SAT_CLIENTS
# the same population with a class of 70 (optimized calls of 2 blocks take the polyphase path and the side-stream look-ahead)
MIX_CLIENTS_BIG = [("d42", -700000 + 20000 * c) for c in range(70)] + SAT_CLIENTS[13:]
# the tile-height engine's Q15 calls (a native call follows them: every decimation divides the blocks)
HEIGHT_CALLS = [(1, MIX_N, ("square",)), (1, MIX_N, ("noise",))]


def mix_blocks(fmt):
    """A (full-scale square: the Q15 call saturates) and C (noise)"""
    return block("square", fmt, MIX_N, seed=3), block("noise", fmt, MIX_N, seed=4)


# ---- churn: joins, leaves and slot reuse between calls of ragged lengths, every block one of KINDS
CHURN_SHAPES = ("d42", "d21", "d7", "edge7", "even16")
CHURN_FCS = (0, 1234, -1234, 40000, -40000, -250000, 345678)


def churn_schedule(seed, steps=12):
    """-> [(joins [(uid, shape, fc)], leaves [uid], G, n, kinds)]: what happens before and in each call.  A call of several blocks
    needs blocks of at least the largest decimation; single blocks go down to 2 elements."""
    rng = np.random.default_rng(seed)
    alive, uid, out = [], 0, []
    for step in range(steps):
        leaves = [] if step == 0 else [alive[i] for i in sorted(rng.choice(len(alive), size=min(len(alive) - 1, int(rng.integers(0, 4))), replace=False))]
        alive = [u for u in alive if u not in leaves]
        joins = []
        for _ in range(9 if step == 0 else int(rng.integers(0, 4))):
            shape = CHURN_SHAPES[int(rng.integers(0, len(CHURN_SHAPES)))]
            fcs = CHURN_FCS[:3] if shape == "edge7" else CHURN_FCS  # (small angles only: no rotation may turn edge7's -1.0 into +1.0, which Q15 cannot hold)
            joins.append((uid, shape, fcs[int(rng.integers(0, len(fcs)))]))
            alive.append(uid)
            uid += 1
        G = int(rng.integers(1, 4))
        n = int(rng.choice([2, 4, 1000, 20002, 40000, MAXIN]) if G == 1 else rng.choice([200, 20002, 30000, MAXIN]))
        kinds = tuple(KINDS[int(rng.integers(0, len(KINDS)))] for _ in range(G))
        out.append((joins, leaves, G, n, kinds))
    return out


CHURN_RUNS = ((1, "cu8"), (2, "cs16"))
