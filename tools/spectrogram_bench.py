"""Measurements of the GPU spectrogram (csrc/xl_spectrum.hip, include/xlating_spectrum.h, include/spectrogram.h); prints one JSON object.

  device     device-resident throughput: xlating_spectrum_feed_device on a filled device buffer (10 Msps rows), samples per second of
             device time (events around each feed; the rows are taken after each), median over `calls` feeds after warm-up;
             W = 1024 and 4096 (power-of-two transform) and W = 1000 (Bluestein), cu8 and cf32
  file       end to end, file -> PNG through spectrogram_main, for a ~1 GB cu8 plain file and the same file gzipped, each against the
             read floor: the same reader loop into the same pinned buffers with no GPU work (XL_EXP_SPEC_READ_FLOOR=1).  The files
             are written just before and read from the page cache; best of `reps` runs each.

usage: python tools/spectrogram_bench.py [--calls N] [--gb G] [--skip-file] [--out FILE]
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


def device_bench(W, fmt, calls, nsamp, sr=10000000):
    import torch

    g = torch.Generator(device="cuda").manual_seed(1)
    if fmt == "cf32":
        d = torch.randn(2 * nsamp, device="cuda", generator=g, dtype=torch.float32) * 0.3
    else:
        d = torch.randint(0, 256, (2 * nsamp,), device="cuda", generator=g, dtype=torch.int32).to(torch.uint8)
    st = torch.cuda.current_stream()
    s = xl.Spectrum(sr, W, fmt)
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
    ap.add_argument("--out")
    a = ap.parse_args()
    res = {"device": xl.device_info(), "device_resident": []}
    for W in (1024, 4096, 1000):
        for fmt in ("cu8", "cf32"):
            res["device_resident"].append(device_bench(W, fmt, a.calls, a.nsamp))
            print(json.dumps(res["device_resident"][-1]), file=sys.stderr, flush=True)
    if not a.skip_file:
        res["file"] = file_bench(a.gb, a.reps)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
