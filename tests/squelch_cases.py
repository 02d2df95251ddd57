"""The squelch scenario of the serve object's tests (tests/test_serve_squelch_cpu.py holds it to the oracle, tests/test_serve_squelch_gpu.py
runs it): the shape of tests/test_serve_tune_gpu.py -- cu8 at 2.016 Msps, calls of 2 blocks of 65536 bytes -- with 8 calls.  Four
clients: twins at 48000 Hz (the rate divides: D = 42) and twins at 44100 Hz (a fractional client); the second of each pair is
squelched.  Over a noise floor of 0.002 each pair's tone, 6 kHz above the pair's centre, is switched per call by an envelope: off, half
level or full.  Every on-interval begins 2048 input samples behind its call's start and ends 2048 before its end, so no filter tail
reaches a neighbouring call.

The envelopes hold, for hang_calls 0 and 1: a half-level call while the gate is closed (0) and while it is open (2), two quiet calls in
a row, a reopening, and a quiet last call; in call 0 both pairs are below their open mark (a call with every squelched client closed).
The marks and the half level are chosen so that the ORACLE's powers lie at least 10x above the open mark (full), 10x below the close
mark (off) and 3x from both (half): a GPU run can then never sit on a threshold."""
import functools

import numpy as np

BAND_FREQ = 437000000
BAND_RATE, BUFFER, GROUP, CALLS = 2016000, 65536, 2, 8
PER_CALL = GROUP * (BUFFER // 2)  # band samples per call
GUARD = 2048
CLIENTS = [(BAND_FREQ + 100000, 48000), (BAND_FREQ + 100000, 48000), (BAND_FREQ - 200000, 44100), (BAND_FREQ - 200000, 44100)]
SQUELCHED = (1, 3)
TONES = [100000 + 6000, -200000 + 6000]  # Hz from the band's centre, per pair
NOISE = 0.002
FULL, HALF = 0.4, 0.04
LEVEL = {"off": 0.0, "half": HALF, "full": FULL}
ENVELOPES = [["half", "full", "half", "off", "off", "full", "half", "off"],   # pair A (clients 0, 1)
             ["off", "half", "full", "off", "full", "half", "off", "off"]]    # pair B (clients 2, 3)
OPEN_POWER, CLOSE_POWER = 1.2e-2, 1.0e-4  # mean power, 1.0 = |y| of 1 (in the cs16 family: full scale)


@functools.lru_cache(maxsize=None)
def capture():
    n = CALLS * PER_CALL
    rng = np.random.default_rng(12)
    t = np.arange(n, dtype=np.float64) / BAND_RATE
    z = NOISE * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    for tone, env in zip(TONES, ENVELOPES):
        a = np.zeros(n)
        for k, what in enumerate(env):
            a[k * PER_CALL + GUARD:(k + 1) * PER_CALL - GUARD] = LEVEL[what]
        z += a * np.exp(2j * np.pi * tone * t)
    v = np.stack([z.real, z.imag], axis=1).reshape(-1)
    raw = np.clip(np.round(127.5 + 127 * v), 0, 255).astype(np.uint8)
    raw.setflags(write=False)
    return raw


def envelope(i):
    """client index -> its pair's envelope"""
    return ENVELOPES[i // 2]


def expected_gates(powers, lens, hang):
    """the Python policy on per-call powers of one squelched client -> (gates, log, withheld)"""
    import meter_ref as MR

    return MR.run_policy(powers, lens, OPEN_POWER, CLOSE_POWER, hang)
