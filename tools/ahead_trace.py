#!/usr/bin/env python3
"""A fixed sequence of engine calls that crosses every branch of the float phase look-ahead (csrc/xl_ahead.h), for comparing the HIP calls
of two builds: run it under `rocprofv3 --hip-trace -- python tools/ahead_trace.py` in each tree and compare the engine thread's ordered
hipStreamWaitEvent / hipEventRecord / kernel-launch calls between the two hipDeviceSynchronize calls that bracket the sequence.

70 clients of the default shape (D = 42, 505 taps), calls of up to 4 blocks: 40 calls that mix side-stream calls (optimized: polyphase) and
fused ones (native on a caller's stream), a shape change, a join, a Q15 call, two caller streams and the engine's.  Ends with a bit-exact
check of the committed phases of every seventh client (and of the joined one) against the oracle; prints "ahead_trace ok <calls>"."""
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


def main():
    code, taps = xl.create_low_pass_filter(1.0, FS, 24000, 9600)
    assert code == 0
    eng = xl.BatchEngine(FS, "cu8", N, group_blocks=G)
    fcs = [-700000 + 20000 * c for c in range(70)]
    ids = [eng.add_client(42, taps, fc) for fc in fcs]
    oracles = {ids[c]: Oracle(42, taps, fcs[c], FS, N) for c in range(0, 70, 7)}
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    A, B, E = sa.cuda_stream, sb.cuda_stream, "engine"
    seq = [("optimized", G, N, E)] * 6 + [("native", G, N, A)] * 3 + [("optimized", G, N, B)] * 4 + [("optimized", 2, 65536, E)] * 3 + \
          ["join"] + [("optimized", G, N, E)] * 5 + [("q15", 1, 84000, E)] + [("optimized", G, N, A)] * 6 + [("native", G, N, E)] * 4 + \
          [("optimized", G, N, B), ("optimized", G, N, E)] * 4
    calls = [c for c in seq if c != "join"]
    assert len(calls) == 40
    xs = [siggen.xs_u8(9100 + k, g * n) for k, (_, g, n, _) in enumerate(calls)]
    dev = [torch.from_numpy(x).cuda() for x in xs]
    torch.cuda.synchronize()  # ---- the sequence begins
    k = 0
    for c in seq:
        if c == "join":
            oracles[eng.add_client(42, taps, 333333)] = Oracle(42, taps, 333333, FS, N)
            continue
        variant, g, n, stream = c
        eng.process_device_group(dev[k].data_ptr(), n, g, variant, stream)
        k += 1
    eng.sync()
    torch.cuda.synchronize()  # ---- and ends
    joined, k = max(oracles), 0
    for c in seq:
        if c == "join":
            continue
        variant, g, n, _ = c
        for cid, o in oracles.items():
            if cid == joined and k < seq.index("join"):
                continue  # (the joined client's stream begins with the join)
            for bl in np.split(xs[k], g):
                o.process("cu8", bl, "cs16") if variant == "q15" else o.process("cu8", bl)
        k += 1
    for cid, o in oracles.items():
        got = tuple(np.float32(v).tobytes() for v in eng.phase(cid))
        assert got == tuple(np.float32(v).tobytes() for v in o.phase), (cid, eng.phase(cid), o.phase)
    eng.close()
    print(f"ahead_trace ok {len(calls)}")


if __name__ == "__main__":
    main()
