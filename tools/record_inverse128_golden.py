#!/usr/bin/env python3
"""tools/record_inverse128_golden.py -- GPU: record tests/golden/inverse128_lds_parent.npz, the outputs of a fixed sample of clients in
every call of tests/test_inverse_epilogue_gpu.py's scenario at M = 128 with the LDS transform (option inverse_kernel = 3), as uint32
bit patterns.  Run it at the commit whose outputs later ones must reproduce bit for bit (the test's docstring names the one that wrote
the committed file); the test compares with array_equal.    python tools/record_inverse128_golden.py [out.npz]"""
import os
import sys

os.environ["XL_TESTING"] = "1"
os.environ["XL_EXP_POLY"] = "1"
os.environ["XL_EXP_POLY_M"] = "128"
os.environ["XL_EXP_INV"] = "3"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402

import test_inverse_epilogue_gpu as t  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else t.GOLDEN_FILE
    rec = {}
    for g in sorted(t.CALLS):
        def each_call(call, x, outs, g=g):
            for i in t.SAMPLE_OF[g]:
                if i in outs:
                    rec["g%d_call%d_client%d" % (g, call, i)] = outs[i].view(np.uint32).copy()
        t.run_scenario(g, each_call)
    np.savez(out, **rec)
    print("wrote %s: %d arrays, %d bytes" % (out, len(rec), os.path.getsize(out)))


if __name__ == "__main__":
    main()
