"""Measurements of the GPU spectrogram (csrc/xl_spectrum.hip, include/xlating_spectrum.h, include/spectrogram.h); prints one JSON object.

  device     device-resident throughput: xlating_spectrum_feed_device on a filled device buffer (10 Msps rows), samples per second of
             device time (events around each feed; the rows are taken after each), median over `calls` feeds after warm-up;
             W = 1024 and 4096 (power-of-two transform) and W = 1000 (Bluestein), cu8 and cf32
  file       end to end, file -> PNG through spectrogram_main, for a ~1 GB cu8 plain file and the same file gzipped, each against the
             read floor: the same reader loop into the same pinned buffers with no GPU work (XL_EXP_SPEC_READ_FLOOR=1).  The files
             are written just before and read from the page cache; best of `reps` runs each.

  --wide     instead of both: the widths above 8192 (csrc/xl_spectrum_wide.hip, Spectrum(..., wide=True)) in ONE process -- 16384, 65536
             and 1048576 (two-level radix-4: two launches per scratch chunk) and 20000 and 200000 (two-level Bluestein: three) -- beside
             8192 and 8191 (the one-workgroup kernels), cf32 and cu8, 2^24-sample feeds of rows without a skip; and each width's time
             beside its byte model at the rate of a plain device copy measured in the same run (torch, 256 MiB, read + write counted):
             the input once plus two (plain) or three (Bluestein) round trips of 16 N bytes per transform through the scratch.

usage: python tools/spectrogram_bench.py [--calls N] [--gb G] [--skip-file] [--wide] [--out FILE]
"""
import argparse
import gzip
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ.setdefault("XL_TESTING", "1")

import sdr_server_amd as xl  # noqa: E402


def device_bench(W, fmt, calls, nsamp, sr=10000000, wide=False):
    import torch

    g = torch.Generator(device="cuda").manual_seed(1)
    if fmt == "cf32":
        d = torch.randn(2 * nsamp, device="cuda", generator=g, dtype=torch.float32) * 0.3
    else:
        d = torch.randint(0, 256, (2 * nsamp,), device="cuda", generator=g, dtype=torch.int32).to(torch.uint8)
    st = torch.cuda.current_stream()
    s = xl.Spectrum(sr, W, fmt, wide=wide)
    times = []
    for k in range(calls + 2):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(st)
        s.feed(d.data_ptr(), nsamp, st.cuda_stream)
        b.record(st)
        s.take_rows()
        b.synchronize()
        if k >= 2:
            times.append(a.elapsed_time(b) * 1e-3)
    s.close()
    t = float(np.median(times))
    return {"W": W, "fmt": fmt, "samples_per_feed": nsamp, "median_s": t, "gsps": nsamp / t / 1e9,
            "transform": "bluestein" if W & (W - 1) else "radix-4"}


def copy_rate(nbytes=256 << 20, reps=10):
    """bytes per second (read + write) of a plain device-to-device copy"""
    import torch

    a = torch.empty(nbytes, device="cuda", dtype=torch.uint8).fill_(1)
    b = torch.empty_like(a)
    times = []
    for k in range(reps + 2):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        b.copy_(a)
        e1.record()
        e1.synchronize()
        if k >= 2:
            times.append(e0.elapsed_time(e1) * 1e-3)
    return 2 * nbytes / float(np.median(times))


def wide_bench(calls, nsamp):
    rate = copy_rate()
    res = {"copy_bytes_per_s": rate, "widths": []}
    for W in (8192, 8191, 16384, 65536, 1048576, 20000, 200000):
        for fmt in ("cf32", "cu8"):
            sr = W * max(1, 10000000 // W)  # rows of about 10 Msps, no skipped samples
            r = device_bench(W, fmt, calls, nsamp, sr, wide=True)
            if W > 8192:
                blue = bool(W & (W - 1))
                N = W
                if blue:
                    N = 1
                    while N < 2 * W - 1:
                        N <<= 1
                T = (nsamp // sr) * (sr // W) + min(sr // W, (nsamp % sr) // W)
                trips = 3 if blue else 2
                r["N"], r["transforms"], r["scratch_round_trips"] = N, T, trips
                r["model_bytes"] = nsamp * (8 if fmt == "cf32" else 2) + trips * 16 * N * T
                r["model_s"] = r["model_bytes"] / rate
                r["fraction_of_byte_model"] = r["model_s"] / r["median_s"]
                r["transform"] = "two-level bluestein" if blue else "two-level radix-4"
            res["widths"].append(r)
            print(json.dumps(r), file=sys.stderr, flush=True)
    return res


def timed_main(inp, out, W, sr, floor):
    if floor:
        os.environ["XL_EXP_SPEC_READ_FLOOR"] = "1"
    else:
        os.environ.pop("XL_EXP_SPEC_READ_FLOOR", None)
    t0 = time.perf_counter()
    code = xl.spectrogram_main(inp, out, W, sr, "cu8")
    t = time.perf_counter() - t0
    os.environ.pop("XL_EXP_SPEC_READ_FLOOR", None)
    assert code == 0, code
    return t


def file_bench(gb, reps, W=1024, sr=10000000):
    # xl_exp_getenv reads the environment at each call: one process can switch the floor on and off
    tmp = tempfile.mkdtemp(prefix="specbench_")
    try:
        nbytes = int(gb * (1 << 30)) // 2 * 2
        rng = np.random.default_rng(5)
        block = (127.5 + 40 * rng.standard_normal(1 << 24)).clip(0, 255).astype(np.uint8)  # 16 MiB of noise, repeated
        plain, gz = os.path.join(tmp, "rec.cu8"), os.path.join(tmp, "rec.cu8.gz")
        with open(plain, "wb") as f, gzip.open(gz, "wb", compresslevel=1) as g:
            left = nbytes
            while left > 0:
                b = block[:min(left, block.size)]
                f.write(b.tobytes())
                g.write(b.tobytes())
                left -= b.size
        res = {}
        for name, path in (("plain", plain), ("gz", gz)):
            out = os.path.join(tmp, "out.png")
            timed_main(path, out, W, sr, False)  # (warm: page cache, device init)
            floor = min(timed_main(path, out, W, sr, True) for _ in range(reps))
            full = min(timed_main(path, out, W, sr, False) for _ in range(reps))
            rows = nbytes // 2 // sr
            res[name] = {"bytes": nbytes, "file_bytes": os.path.getsize(path), "rows": rows, "W": W, "sr": sr, "read_floor_s": floor,
                         "end_to_end_s": full, "ratio": full / floor}
        return res
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--nsamp", type=int, default=1 << 26)
    ap.add_argument("--gb", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--skip-file", action="store_true")
    ap.add_argument("--wide", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    res = {"device": xl.device_info(), "device_resident": []}
    if a.wide:
        res["wide"] = wide_bench(a.calls, min(a.nsamp, 1 << 24))
    for W in () if a.wide else (1024, 4096, 1000):
        for fmt in ("cu8", "cf32"):
            res["device_resident"].append(device_bench(W, fmt, a.calls, a.nsamp))
            print(json.dumps(res["device_resident"][-1]), file=sys.stderr, flush=True)
    if not a.skip_file and not a.wide:
        res["file"] = file_bench(a.gb, a.reps)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
