#!/usr/bin/env python3
"""Fixed sequences of engine calls that cross every branch of a phase look-ahead, for comparing the HIP calls of two builds: run one under
`rocprofv3 --hip-trace -- python tools/ahead_trace.py [--q15]` in each tree and compare the engine thread's ordered hipStreamWaitEvent /
hipEventRecord / kernel-launch calls between the two hipDeviceSynchronize calls that bracket the sequence.

70 clients of the default shape (D = 42, 505 taps), calls of up to 4 blocks.
Default, the float look-ahead (csrc/xl_ahead.h): 40 calls that mix side-stream calls (optimized: polyphase) and fused ones (native on a
caller's stream), a shape change, a join, a Q15 call, two caller streams and the engine's.
--q15, the Q15 look-ahead (csrc/xl_q15_ahead.h, option "q15_nco" = 1): 33 Q15 calls and a float call between them -- runs of equal calls
(hits), two shape changes, a join, the float call, two caller streams and the engine's in turn, the option set to 0 and back to 1.
Either ends with a bit-exact check of the committed phases (float, and Q15 under --q15) of every seventh client and of the joined one against
the oracle; prints "ahead_trace ok <calls>"."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import numpy as np
import torch

import sdr_server_amd as xl
import siggen
from pyoracle import Oracle

FS, N, G = 2016000, 100002, 4


def float_sequence(A, B, E):
    seq = [("optimized", G, N, E)] * 6 + [("native", G, N, A)] * 3 + [("optimized", G, N, B)] * 4 + [("optimized", 2, 65536, E)] * 3 + \
          ["join"] + [("optimized", G, N, E)] * 5 + [("q15", 1, 84000, E)] + [("optimized", G, N, A)] * 6 + [("native", G, N, E)] * 4 + \
          [("optimized", G, N, B), ("optimized", G, N, E)] * 4
    return seq, 40


def q15_sequence(A, B, E):
    seq = [("q15", G, N, E)] * 4 + [("q15", G, N, A)] * 3 + [("q15", G, N, B), ("q15", G, N, A)] * 2 + [("q15", 2, 65536, E)] * 3 + \
          ["join"] + [("q15", G, N, E)] * 4 + [("optimized", G, N, E)] + [("q15", G, N, A)] * 3 + [("option", 0)] + [("q15", G, N, B)] * 2 + \
          [("option", 1)] + [("q15", G, N, B)] * 3 + [("q15", 1, 84000, E)] * 3 + [("q15", G, N, A), ("q15", G, N, E)] * 2
    return seq, 34


def main():
    q15 = "--q15" in sys.argv[1:]
    code, taps = xl.create_low_pass_filter(1.0, FS, 24000, 9600)
    assert code == 0
    eng = xl.BatchEngine(FS, "cu8", N, group_blocks=G)
    if q15:
        eng.set_option("q15_nco", 1)
    fcs = [-700000 + 20000 * c for c in range(70)]
    ids = [eng.add_client(42, taps, fc) for fc in fcs]
    oracles = {ids[c]: Oracle(42, taps, fcs[c], FS, N) for c in range(0, 70, 7)}
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    seq, ncalls = (q15_sequence if q15 else float_sequence)(sa.cuda_stream, sb.cuda_stream, "engine")
    calls = [c for c in seq if len(c) == 4 and c != "join"]
    assert len(calls) == ncalls
    xs = [siggen.xs_u8(9100 + k, g * n) for k, (_, g, n, _) in enumerate(calls)]
    dev = [torch.from_numpy(x).cuda() for x in xs]
    torch.cuda.synchronize()  # ---- the sequence begins
    k = 0
    for c in seq:
        if c == "join":
            oracles[eng.add_client(42, taps, 333333)] = Oracle(42, taps, 333333, FS, N)
        elif c[0] == "option":
            eng.set_option("q15_nco", c[1])
        else:
            variant, g, n, stream = c
            eng.process_device_group(dev[k].data_ptr(), n, g, variant, stream)
            k += 1
    eng.sync()
    torch.cuda.synchronize()  # ---- and ends
    joined, k = max(oracles), 0
    for i, c in enumerate(seq):
        if len(c) != 4 or c == "join":
            continue
        variant, g, n, _ = c
        for cid, o in oracles.items():
            if cid == joined and i < seq.index("join"):
                continue  # (the joined client's stream begins with the join)
            for bl in np.split(xs[k], g):
                o.process("cu8", bl, "cs16") if variant == "q15" else o.process("cu8", bl)
        k += 1
    for cid, o in oracles.items():
        got = tuple(np.float32(v).tobytes() for v in eng.phase(cid))
        assert got == tuple(np.float32(v).tobytes() for v in o.phase), (cid, eng.phase(cid), o.phase)
        if q15:
            assert tuple(eng.phase_q15(cid)) == tuple(o.phase_q15), (cid, eng.phase_q15(cid), o.phase_q15)
    if q15:
        assert "| q15 nco: ahead, " in eng.describe(), eng.describe()
        print(eng.describe().split("| q15 nco: ")[1].split(" |")[0])
    eng.close()
    print(f"ahead_trace ok {len(calls)}")


if __name__ == "__main__":
    main()
