#!/usr/bin/env python3
"""tools/tune_bank_bench.py -- what a feed of the tuner bank (include/xlating_tune.h) costs at the headline call's rows: 1024 streams of
8 x 3120 complex float32 samples (1024 clients x 48 kHz in a band of 2016000 Hz, 8 blocks of 262144 bytes per call), every stream with
a shift and a ramp of its own.

The yardstick is the plain delivery pack launch (xlating_delivery_pack_device) over the same rows in the same process: both read 8
bytes a sample and write 8 bytes a sample.  Three things alternate, in rounds:
  feed    one tuner feed of all streams: one table copy and one ragged launch
  pack    one delivery pack of the same rows: one table copy and one pack launch (its device-to-host copy lies outside the events and
          is waited for outside the clocks)
  loop    1024 feeds of one stream each, the rows of `feed` one by one: what rotating per client costs
Per item: the device time between HIP events recorded on the launch stream around the call(s), and the host time of the call(s)
themselves (the feed waits for nothing, so this is what the serve object's thread spends).  Medians of --iters per round; the spread
of each over its rounds is reported, and a ratio is called a difference only where it exceeds the yardstick's own spread.
Prints a report; profiles/tune_bank_vs_pack.txt is one run of it on an MI355X."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("XL_TESTING", "1")
import numpy as np  # noqa: E402

import sdr_server_amd as xl  # noqa: E402

BUFFER = 262144


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=1024)
    ap.add_argument("--group", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--loop-iters", type=int, default=3)
    ap.add_argument("--report", default=None)
    a = ap.parse_args(argv)
    import torch

    n, rows = a.streams, a.group * (BUFFER // 2 // 42)
    pitch = rows * 8 + 64
    src = (0.3 * torch.randn((n * pitch // 4,), dtype=torch.float32, device="cuda")).view(torch.uint8)
    ptrs = [src.data_ptr() + i * pitch for i in range(n)]
    st = torch.cuda.Stream()
    bank, d = xl.TuneBank(), xl.Delivery(2)
    rng = np.random.default_rng(1)
    sids = [bank.add(int(rng.integers(0, 1 << 63)), *xl.tune_from_hz(float(rng.uniform(-10000, 10000)), float(rng.uniform(-300, 300)), 48000.0))
            for _ in range(n)]
    keys, counts, nbytes = list(range(n)), [rows] * n, [rows * 8] * n

    def timed(what):
        ev0, ev1 = (torch.cuda.Event(enable_timing=True) for _ in range(2))
        t = None
        with torch.cuda.stream(st):
            ev0.record()
            h0 = time.perf_counter()
            if what == "feed":
                bank.feed(sids, ptrs, counts, st.cuda_stream)
            elif what == "pack":
                t = d.pack(keys, ptrs, nbytes, st.cuda_stream)
            else:
                for i in range(n):
                    bank.feed(sids[i:i + 1], ptrs[i:i + 1], counts[i:i + 1], st.cuda_stream)
            h1 = time.perf_counter()
            ev1.record()
        if t is not None:
            d.wait(t)
            d.release(t)
        st.synchronize()
        return ev0.elapsed_time(ev1), 1e3 * (h1 - h0)

    names = ("feed", "pack", "loop")
    iters = {"feed": a.iters, "pack": a.iters, "loop": a.loop_iters}
    for what in names:  # (the arena, the slots' buffers, the tables, the clocks)
        for _ in range(2):
            timed(what)
    dev, host = {k: [] for k in names}, {k: [] for k in names}
    for rnd in range(a.rounds):
        for what in names:
            got = [timed(what) for _ in range(iters[what])]
            dev[what].append(float(np.median([g[0] for g in got])))
            host[what].append(float(np.median([g[1] for g in got])))
    total = n * rows * 8
    label = {"feed": "one tuner feed (table copy + ragged launch)", "pack": "one delivery pack (table copy + pack launch)",
             "loop": f"{n} one-stream tuner feeds"}
    out = [f"tune_bank_bench: {xl.device_info()}",
           f"{n} streams of {rows} cf32 samples = {total / 1e6:.1f} MB read and {total / 1e6:.1f} MB written by either launch; HIP events on the "
           f"launch stream and a host clock around the call(s); {a.rounds} alternating rounds, median of {a.iters} each ({a.loop_iters} for the loop)"]
    for k in names:
        m, lo, hi = float(np.median(dev[k])), min(dev[k]), max(dev[k])
        hm = float(np.median(host[k]))
        out.append(f"  {label[k]:46s} device ms, rounds: " + " ".join(f"{v:7.3f}" for v in dev[k]) +
                   f"  median {m:.3f} ms = {2 * total / m / 1e6:.0f} GB/s read + written, spread {100 * (hi - lo) / lo:.1f} %;  host ms, median {hm:.3f} "
                   f"(rounds " + " ".join(f"{v:.3f}" for v in host[k]) + ")")
    f, p, lp = (float(np.median(dev[k])) for k in names)
    spread = (max(dev["pack"]) - min(dev["pack"])) / min(dev["pack"])
    out.append(f"  device: feed / pack = {f / p:.3f}; the pack's own spread over its rounds is {100 * spread:.1f} %: the difference "
               f"{'exceeds' if abs(f / p - 1.0) > spread else 'lies within'} it")
    out.append(f"  device: loop of one-stream feeds / one feed = {lp / f:.1f}")
    hf, hp, hl = (float(np.median(host[k])) for k in names)
    out.append(f"  host: feed / pack = {hf / hp:.3f}; loop of one-stream feeds / one feed = {hl / hf:.1f}")
    assert bank.last_feed_ops() == (1, 1)
    bank.close()
    d.close()
    text = "\n".join(out)
    print(text)
    if a.report:
        with open(a.report, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
