"""Measurements of the wide direct FIR (csrc/xl_wide.hip); prints one JSON object.

  dropin   create_frequency_xlating_filter shapes whose window image fits no LDS tile: microseconds per process_* call (the call
           is synchronous: host wall clock around it, median after warm-up), native and optimized, 262144-byte blocks
  engine   the headline engine (1024 clients at D = 42, cu8 at 2.016 Msps, 8 blocks of 262144 bytes per call, optimized) with and
           without 16 added D = 1120 clients, alternating in one process; microseconds per call from device events around
           `calls` consecutive calls on one stream, after warm-up

usage: python tools/wide_bench.py [--calls N] [--warmup W] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import siggen  # noqa: E402
import sdr_server_amd as xl  # noqa: E402


def lpf(fs, rate):
    code, t = xl.create_low_pass_filter(1.0, fs, rate // 2, rate // 5)
    assert code == 0
    return t


def dropin(fs, fmt, rate, calls, warmup):
    D = fs // rate
    taps = lpf(fs, rate)
    n = 262144
    x = siggen.xs_u8(11, n) if fmt == "cu8" else siggen.xs_s8(11, n)
    res = {"fs": fs, "fmt": fmt, "D": D, "T": len(taps)}
    for variant in ("native", "optimized"):
        f = xl.XlatingFilter(D, taps, 100000, fs, n)
        for _ in range(warmup):
            f.process(variant, fmt, "cf32", x)
        ts = []
        for _ in range(calls):
            t0 = time.perf_counter()
            f.process(variant, fmt, "cf32", x)
            ts.append(time.perf_counter() - t0)
        f.close()
        res[variant + "_us"] = round(float(np.median(ts)) * 1e6, 1)
    res["block_real_time_us"] = round(n / 2 / fs * 1e6, 1)
    return res


def engine(calls, warmup, rounds):
    import torch

    fs, n, G = 2016000, 262144, 8
    t42, t1120 = lpf(fs, 48000), lpf(fs, 1800)
    x = torch.from_numpy(siggen.xs_u8(12, G * n)).cuda()
    stream = torch.cuda.current_stream()

    def make(wide):
        e = xl.BatchEngine(fs, "cu8", n, group_blocks=G)
        for c in range(1024):
            e.add_client(42, t42, -900000 + 1750 * c)
        for c in range(wide):
            e.add_client(1120, t1120, -800000 + 100000 * c)
        return e

    engs = {"base": make(0), "with_16_wide": make(16)}
    for e in engs.values():
        for _ in range(warmup):
            e.process_device_group(x.data_ptr(), n, G, "optimized", stream=stream.cuda_stream)
    torch.cuda.synchronize()
    res = {k: [] for k in engs}
    for _ in range(rounds):  # alternating
        for k, e in engs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            for _ in range(calls):
                e.process_device_group(x.data_ptr(), n, G, "optimized", stream=stream.cuda_stream)
            b.record(stream)
            b.synchronize()
            res[k].append(a.elapsed_time(b) * 1e3 / calls)
    out = {k + "_us_per_call": round(float(np.median(v)), 1) for k, v in res.items()}
    out["growth"] = round(out["with_16_wide_us_per_call"] / out["base_us_per_call"] - 1.0, 3)
    out["plan_with_wide"] = engs["with_16_wide"].describe()
    for e in engs.values():
        e.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out")
    a = ap.parse_args()
    r = {"device": xl.device_info(),
         "dropin": [dropin(20000000, "cs8", 10000, a.calls, a.warmup), dropin(2400000, "cu8", 2000, a.calls, a.warmup)],
         "engine": engine(a.calls, a.warmup, a.rounds)}
    s = json.dumps(r)
    print(s)
    if a.out:
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
