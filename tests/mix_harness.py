"""The harness shared by the GPU tests that run small forced polyphase engines over a few multi-block calls and hold every client to the
oracle population (tests/test_mix_operand_image_gpu.py, tests/test_mix_kblocks_gpu.py): input streams per format, client frequencies,
one engine run, the error figure.  `population` is oracle/pyoracle.py's every-client oracle."""
import numpy as np

import siggen
import sdr_server_amd as xl
from pyoracle import population  # noqa: F401  (re-exported)

FS = 2016000
NSAMP = 16384          # samples per block
ELEMS = 2 * NSAMP      # scalar elements per block = bytes of a cu8 block
REL_TOL = 1e-5         # the project's bar for the optimized variant
NCALLS = 3


def _stream(fmt, nblocks, seed):
    n = ELEMS * nblocks
    if fmt == "cu8":
        return siggen.xs_u8(seed, n)
    if fmt == "cs8":
        return siggen.xs_s8(seed, n)
    if fmt == "cs16":
        return siggen.xs_s16(seed, n)
    return (siggen.xs_s16(seed, n).astype(np.float32) / np.float32(32768)).astype(np.float32)


def _fcs(nclients):
    return [int(-0.45 * FS + (0.9 * FS / nclients) * c) + 17 * (c % 5) for c in range(nclients)]


def _run(fmt, D, taps, fcs, m, image, x, nblocks, ncalls=NCALLS, options=()):
    """One engine over ncalls calls of nblocks blocks: per client the concatenated outputs, and the plan's description.  image: option
    "mix_operand_image" (None: left alone); m: option "polyphase_m" (0: left alone); options: further (name, value) pairs, set in order."""
    eng = xl.BatchEngine(FS, fmt, ELEMS, group_blocks=max(nblocks, 1))
    if image is not None:
        eng.set_option("mix_operand_image", image)
    if m:
        eng.set_option("polyphase_m", m)
    for name, value in options:
        eng.set_option(name, value)
    ids = [eng.add_client(D, taps, fc) for fc in fcs]
    outs = [[] for _ in ids]
    per_call = ELEMS * nblocks
    for k in range(ncalls):
        eng.process_host_group(x[k * per_call:(k + 1) * per_call], nblocks, "optimized")
        eng.fetch()
        for c, i in enumerate(ids):
            outs[c].append(eng.output(i).copy())
    d = eng.describe()
    eng.close()
    return [np.concatenate(o) for o in outs], d


def _rel_err(a, b):
    return float(np.abs(a.astype(np.complex128) - b.astype(np.complex128)).max() / max(np.abs(b).max(), 1e-30))
