"""The restatement of the tuner bank's rule (include/xlating_tune.h, csrc/xl_tune_rule.h) the GPU tests hold the kernel to bit for bit,
and the runner of the rule's sweep (tests/c/tune_rule_sweep.c).  The sweep is a sanitized program for the CPU tests alone
(tests/test_tune_cpu.py); a GPU test that needs its E reads the value DESIGN 3.11 carries (design_E), which a CPU test pins to the
sweep's own output.

Phases are Python integers, reduced mod 2^64 where the rule says so; cos and sin come through xl.tune_cs, the library's own export of
the rule (the sweep holds THAT text to libm over all 2^32 phases); the product is float32 numpy operations in the stated order:
re = fl(fl(xr c) - fl(xi s)), im = fl(fl(xr s) + fl(xi c))."""
import functools
import math
import os
import re
import subprocess
import tempfile
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import sdr_server_amd as xl
from conftest import ROOT

M64 = (1 << 64) - 1
CSRC = os.path.join(ROOT, "sdr-server_amd", "csrc")
SWEEP_SRC = os.path.join(ROOT, "tests", "c", "tune_rule_sweep.c")
SANITIZE = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def signed64(v):
    v &= M64
    return v - (1 << 64) if v >> 63 else v


def phase(P, F, R, j):
    """phi_j of a feed that starts in the state (P, F, R)"""
    return (P + j * F + (j * (j - 1) // 2) * R) & M64


def advance(P, F, R, n):
    """-> the state (P, F, R) after n samples"""
    return phase(P, F, R, n), signed64(F + n * R), R


def from_hz(shift_hz, ramp_hz_per_s, rate):
    """the stated double operations; round() of a float is to nearest, ties to even, as llrint in the default mode"""
    return round(math.ldexp(shift_hz / rate, 64)), round(math.ldexp(ramp_hz_per_s / rate / rate, 64))


def cs(phis):
    """phis: 64-bit phases -> (c, s) float32 arrays by the rule, of phi >> 32"""
    c, s = np.zeros(len(phis), np.float32), np.zeros(len(phis), np.float32)
    for i, phi in enumerate(phis):
        c[i], s[i] = xl.tune_cs(phi >> 32)
    return c, s


def rotate(x, P, F, R):
    """x: complex64 [n], the samples of one feed of a stream in the state (P, F, R) -> (its rotation complex64 [n], the state after)"""
    x = np.ascontiguousarray(x, dtype=np.complex64)
    phis = [phase(P, F, R, j) for j in range(x.size)]
    c, s = cs(phis)
    xr, xi = x.real.astype(np.float32), x.imag.astype(np.float32)
    y = np.empty(x.size, np.complex64)
    y.real = xr * c - xi * s
    y.imag = xr * s + xi * c
    return y, advance(P, F, R, x.size)


def exact(x, P, F, R):
    """x exp(2 pi i phi_j / 2^64) in float64 (the phase reduced to 53 bits of a turn first: 2^-53 of a turn is far below the bound)"""
    t = np.array([phase(P, F, R, j) / 2.0 ** 64 for j in range(len(x))])
    return np.asarray(x, np.complex128) * np.exp(2j * np.pi * t)


def design_E():
    """E as DESIGN 3.11 carries it: the sweep's printed hex value (test_design_states_the_measured_error holds the two equal), parsed,
    not retyped"""
    m = re.search(r"\*\*E = (0x[0-9a-f.]+p-\d+)\*\*", open(os.path.join(ROOT, "DESIGN.md")).read())
    assert m, "DESIGN 3.11 states E"
    return float.fromhex(m.group(1))


@functools.lru_cache(maxsize=None)
def sweep():
    """builds the sweep under ASan and UBSan and runs it: xl_tune_cs over all 2^32 phases in child processes, the phase arithmetic and
    from_hz (CPU tests only: never from a test marked gpu) -> {"E", "circle", "phases", "phase_checks", "hz_checks"}; E and circle as the program printed them.  Once per process."""
    tmp = tempfile.mkdtemp(prefix="tune_sweep_")
    exe = os.path.join(tmp, "tune_rule_sweep")
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-pedantic", "-ffp-contract=off"] + SANITIZE +
                       ["-I", CSRC, SWEEP_SRC, "-o", exe, "-lm"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]

    def run(args):
        r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=900)
        assert r.returncode == 0 and r.stdout.startswith("ok ") and r.stderr == "", (args, r.stdout[-500:], r.stderr[-2000:])
        return r.stdout.split()

    jobs = [("cs", a, a + 3) for a in range(0, 256, 4)]
    with ThreadPoolExecutor(max_workers=max(1, min(16, os.cpu_count() or 1))) as pool:
        outs = list(pool.map(run, jobs))
    ph, hz = run(("phase",)), run(("hz",))
    os.remove(exe)
    os.rmdir(tmp)
    return {"phases": sum(int(o[1]) for o in outs), "E": max(float.fromhex(o[2]) for o in outs),
            "circle": max(float.fromhex(o[3]) for o in outs), "phase_checks": int(ph[1]), "hz_checks": int(hz[1])}
