"""GPU tests of the operand-form image of the shared spectra (option "mix_operand_image"; csrc/xl_xop_layout.h): the forward launch
writes every spectrum value once in the two-half mix's A-operand form and the mix launch copies it, instead of every column group
converting the float32 spectra again.  The same halves reach the same matrix instructions in the same order, so an engine with the
option at 1 (the image wherever the form exists; the default, -1, takes it by a size rule) must give, bit for bit, the outputs of an
engine with the option at 0 -- and both stay inside the path's 1e-5 of max|y| against the oracle population.

Blocks are 32768 bytes of cu8 (16384 samples, the same count in every format).  With 128-point transforms 8 blocks of D = 42 are 27
segments: two passes, the second one partial; (21, 253) gives 3 k-blocks and four passes, (64, 769) 8 k-blocks (the three-waves
instantiation, no padding branches), (42, 505) 6 k-blocks with padding branches.  160 clients are two column groups, the second one
partial.  The 256-point kernels (what the size rule gives classes this small) run the same shapes with 16 blocks where two passes are
wanted."""
import numpy as np
import pytest

import siggen
import sdr_server_amd as xl
from mix_harness import ELEMS, FS, NCALLS, REL_TOL, _fcs, _rel_err, _run, _stream, population  # (shared with test_mix_kblocks_gpu.py)
from pyoracle import Oracle

pytestmark = pytest.mark.gpu


def _taps(ntaps):
    if ntaps == 505:
        code, t = xl.create_low_pass_filter(1.0, FS, 24000, 9600)  # the server's own filter
        assert code == 0 and t.size == 505
        return t
    return siggen.hamming_sinc(ntaps, 0.45 / {253: 21, 769: 64}[ntaps])


# (D, taps, format, clients, blocks per call, transform length: 0 = the size rule's 256 points)
CASES = [
    (42, 505, "cu8", 32, 8, 128),
    (42, 505, "cu8", 160, 1, 128),
    (42, 505, "cs8", 160, 8, 128),
    (42, 505, "cs16", 32, 1, 128),
    (42, 505, "cs16", 160, 8, 128),
    (42, 505, "cu8", 160, 16, 0),
    (21, 253, "cs16", 160, 8, 128),
    (21, 253, "cu8", 32, 1, 0),
    (64, 769, "cu8", 160, 8, 128),
    (64, 769, "cs8", 32, 16, 0),
]


@pytest.mark.parametrize("D,ntaps,fmt,nclients,nblocks,m", CASES, ids=lambda v: str(v))
def test_operand_image_bit_identical_to_converting_staging(D, ntaps, fmt, nclients, nblocks, m):
    taps, fcs = _taps(ntaps), _fcs(nclients)
    x = _stream(fmt, nblocks * NCALLS, 4242 + D + nblocks)
    old, d_old = _run(fmt, D, taps, fcs, m, 0, x, nblocks)
    new, d_new = _run(fmt, D, taps, fcs, m, 1, x, nblocks)
    plan = "polyphase: cls0 D%d T%d cols%d " % (D, ntaps, nclients)
    assert plan in d_old and " mix=mfma" in d_old and "mix=mfma/img" not in d_old, d_old
    assert plan in d_new and "mix=mfma/img" in d_new and " M%d " % (m or 256) in d_new, d_new
    for c in range(nclients):
        assert new[c].shape == old[c].shape and np.array_equal(new[c], old[c]), (c, _rel_err(new[c], old[c]))
    want = population(D, taps, fcs, FS, ELEMS, fmt, x, nblocks * NCALLS)
    worst = 0.0
    for c in range(nclients):
        assert len(new[c]) == len(want[c]), c
        worst = max(worst, _rel_err(new[c], want[c]))
    print("worst rel err vs oracle: %.3g" % worst)
    assert worst <= REL_TOL, worst


def test_operand_image_with_a_client_joining_between_calls():
    """A join computes the new column's branch spectra only; the image of the shared spectra is the same one.  Both engines, every
    client, every call bit for bit; the option-1 engine against the oracle (the joiner's own filter starts at its join)."""
    D, taps, fmt, nblocks = 42, _taps(505), "cu8", 8
    fcs = _fcs(159)
    joiner_fc = 123456
    ncalls, join_at = 6, 2
    x = _stream(fmt, nblocks * ncalls, 777)
    per_call = ELEMS * nblocks
    res = {}
    for image in (0, 1):
        eng = xl.BatchEngine(FS, fmt, ELEMS, group_blocks=nblocks)
        eng.set_option("mix_operand_image", image)
        eng.set_option("polyphase_m", 128)
        ids = [eng.add_client(D, taps, fc) for fc in fcs]
        outs = [[] for _ in range(len(ids) + 1)]
        for k in range(ncalls):
            if k == join_at:
                ids.append(eng.add_client(D, taps, joiner_fc))
            eng.process_host_group(x[k * per_call:(k + 1) * per_call], nblocks, "optimized")
            eng.fetch()
            for c, i in enumerate(ids):
                outs[c].append(eng.output(i).copy())
        d = eng.describe()
        eng.close()
        assert ("mix=mfma/img" in d) == bool(image) and "cols160 " in d, d  # (the joiner has merged into the class by the last call)
        res[image] = [np.concatenate(o) for o in outs]
    for c in range(160):
        assert np.array_equal(res[1][c], res[0][c]), c
    want = population(D, taps, fcs, FS, ELEMS, fmt, x, nblocks * ncalls)
    for c in range(159):
        assert len(res[1][c]) == len(want[c]) and _rel_err(res[1][c], want[c]) <= REL_TOL, (c, _rel_err(res[1][c], want[c]))
    o = Oracle(D, taps, joiner_fc, FS, ELEMS)
    wj = np.concatenate([o.process(fmt, x[b * ELEMS:(b + 1) * ELEMS]) for b in range(join_at * nblocks, ncalls * nblocks)])
    o.close()
    assert len(res[1][159]) == len(wj) and _rel_err(res[1][159], wj) <= REL_TOL, _rel_err(res[1][159], wj)


def test_cf32_stream_does_not_take_the_operand_image():
    """A cf32 stream's scale is known only behind the forward launch (per segment): its classes keep the float32 spectra whatever the
    option says, and the option changes nothing in their outputs."""
    D, taps, fmt, nblocks, nclients = 42, _taps(505), "cf32", 8, 40
    fcs = _fcs(nclients)
    x = _stream(fmt, nblocks * NCALLS, 99)
    old, d_old = _run(fmt, D, taps, fcs, 128, 0, x, nblocks)
    new, d_new = _run(fmt, D, taps, fcs, 128, 1, x, nblocks)
    for d in (d_old, d_new):
        assert "polyphase: cls0 D42 T505 cols40 " in d and " mix=mfma" in d and "mix=mfma/img" not in d, d
    for c in range(nclients):
        assert np.array_equal(new[c], old[c]), c
    want = population(D, taps, fcs, FS, ELEMS, fmt, x, nblocks * NCALLS)
    for c in range(nclients):
        assert len(new[c]) == len(want[c]) and _rel_err(new[c], want[c]) <= REL_TOL, (c, _rel_err(new[c], want[c]))


def test_option_values():
    eng = xl.BatchEngine(FS, "cu8", ELEMS)
    for bad in (-2, 2):
        with pytest.raises(xl.XlatingError):
            eng.set_option("mix_operand_image", bad)
    for ok in (0, 1, -1):
        eng.set_option("mix_operand_image", ok)
    eng.close()


@pytest.mark.parametrize("nclients,nblocks,image", [(160, 8, False), (1024, 8, True), (1024, 1, False), (1280, 8, False)])
def test_size_rule(nclients, nblocks, image):
    """By default (-1) the image is taken where it measured ahead (xlp_ximg_pays: 768 .. 1088 clients, calls of four blocks or more);
    every other class keeps the converting staging.  (Forcing the image changes no output bit: the cases above.)"""
    eng = xl.BatchEngine(FS, "cu8", ELEMS, group_blocks=nblocks)
    taps = _taps(505)
    for fc in _fcs(nclients):
        eng.add_client(42, taps, fc)
    d = eng.describe()
    eng.close()
    assert "polyphase: cls0 D42 T505 cols%d " % nclients in d and " mix=mfma" in d and ("mix=mfma/img" in d) == image, d
