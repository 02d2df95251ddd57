#!/usr/bin/env python3
"""tools/record_phase_expand_golden.py -- GPU: record tests/golden/phase_expand_parent.npz, the outputs of two clients in the recorded
calls of every case of tests/test_phase_expand_gpu.py (each inverse kernel, each transform length, the added block lengths), as uint32
bit patterns.  Run it at the commit whose outputs later ones must reproduce bit for bit (the test's docstring names the one that wrote
the committed file); the test compares with array_equal.    python tools/record_phase_expand_golden.py [out.npz]"""
import os
import sys

os.environ["XL_TESTING"] = "1"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402

import test_phase_expand_gpu as t  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else t.GOLDEN_FILE
    rec = {}
    for case in t.CASES:
        t.force_plan(os.environ.__setitem__, case)

        def each_call(call, x, outs, case=case):
            if call in t.CASES[case][5]:
                for i in t.SAMPLE:
                    rec[t.golden_key(case, call, i)] = outs[i].view(np.uint32).copy()
        t.run_case(case, each_call)
        print("recorded", case, flush=True)
    np.savez_compressed(out, **rec)
    print("wrote %s: %d arrays, %d bytes" % (out, len(rec), os.path.getsize(out)))


if __name__ == "__main__":
    main()
