"""Measurement of the resampler bank (csrc/xl_resample.hip, include/xlating_resample.h); prints one JSON object.

  One bank feed of all streams against a loop of one-stream feeds of the same bank (a second set of streams of the same definition),
  in the same process, on the same device rows, alternating.  Two measures per repetition: host time of the feed call(s) (the enqueue:
  neither waits for the device) and device time between HIP events recorded before the first and behind the last queued operation.
  Median, minimum and maximum over `reps` repetitions after warm-up.

  The case: 1024 clients x 48 kHz on a 10 Msps cf32 band, as xlating_wire_admit_any_rate admits them: D = 125 in the engine, 3 / 5 and
  61 taps (Q = 21) in the bank.  Every stream is fed a row of the length the engine's headline-shaped call (8 blocks of 262144 bytes)
  leaves it: 8 * 32768 / 125 = 2097 samples at 80 kHz, from which a feed makes 1258 or 1259 outputs at 48 kHz.

  --q15: the Q15 bank (include/xlating_resample_q15.h) beside the float bank instead, in the same setup and process, alternating: one
  feed of all streams each, the float bank's on cf32 rows, the Q15 bank's on int16-pair rows of the same length.  The float feed is
  the yardstick.  Two more Q15 banks run in the same alternation with one of the kernel's two choices switched off each (XL_EXP_RSQ,
  read when a bank is created): the sums in 64 bits, and the tap table read in place and not from LDS -- what each choice buys.

usage: python tools/resample_bank_bench.py [--q15] [--reps N] [--streams N] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("XL_TESTING", "1")

import sdr_server_amd as xl  # noqa: E402


def stats(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v)), "n": len(v)}


def bench(nstreams, reps, warm=3):
    import torch

    band, fo = 10000000, 48000
    req = xl.WireRequest(460101000, fo, 460100000, 0)
    code, adm, rs, why = xl.wire_admit_any_rate(req, band, 0, 5)
    assert code == 0 and (adm.decimation, rs.L, rs.M) == (125, 3, 5)
    code, taps = xl.wire_resample_taps(req, rs, 5)
    assert code == 0
    per = 8 * (262144 // 8) // adm.decimation
    d = torch.randn(2 * per * nstreams, device="cuda", dtype=torch.float32) * 0.3
    ptrs = [d.data_ptr() + 8 * per * i for i in range(nstreams)]
    counts = [per] * nstreams
    st = torch.cuda.current_stream()
    bank = xl.ResamplerBank()
    ids = [bank.add(rs.L, rs.M, taps) for _ in range(nstreams)]
    loop_ids = [bank.add(rs.L, rs.M, taps) for _ in range(nstreams)]
    res = {"bank": {"host_s": [], "device_s": []}, "loop": {"host_s": [], "device_s": []}}
    ops = None
    for k in range(reps + warm):
        for which in ("bank", "loop"):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(st)
            t0 = time.perf_counter()
            if which == "bank":
                bank.feed(ids, ptrs, counts, st.cuda_stream)
            else:
                for i, p in zip(loop_ids, ptrs):
                    bank.feed([i], [p], [per], st.cuda_stream)
            t1 = time.perf_counter()
            b.record(st)
            b.synchronize()
            if which == "bank":
                ops = bank.last_feed_ops()
            if k >= warm:
                res[which]["host_s"].append(t1 - t0)
                res[which]["device_s"].append(a.elapsed_time(b) * 1e-3)
    produced = bank.produced(ids[0])
    stats_ = bank.stats()
    bank.close()
    out = {"case": f"{nstreams} x 48 kHz on 10 Msps cf32: D 125, then 3/5 with {taps.size} taps", "streams": nstreams,
           "samples_per_stream_per_feed": per, "outputs_per_stream_per_feed": produced / (reps + warm),
           "bank_last_feed_ops": ops, "tables": stats_[1], "table_bytes": stats_[2]}
    for which in res:
        out[which] = {m: stats(v) for m, v in res[which].items()}
    out["host_speedup"] = out["loop"]["host_s"]["median"] / out["bank"]["host_s"]["median"]
    out["device_speedup"] = out["loop"]["device_s"]["median"] / out["bank"]["device_s"]["median"]
    return out


def bench_q15(nstreams, reps, warm=3):
    import torch

    band, fo = 10000000, 48000
    req = xl.WireRequest(460101000, fo, 460100000, 0)
    code, adm, rs, why = xl.wire_admit_any_rate(req, band, 0, 5)
    assert code == 0 and (adm.decimation, rs.L, rs.M) == (125, 3, 5)
    code, taps = xl.wire_resample_taps(req, rs, 5)
    assert code == 0
    per = 8 * (262144 // 8) // adm.decimation
    st = torch.cuda.current_stream()
    df = torch.randn(2 * per * nstreams, device="cuda", dtype=torch.float32) * 0.3
    dq = torch.randint(-32768, 32768, (2 * per * nstreams,), device="cuda", dtype=torch.int32).to(torch.int16)
    arms = {"float": (xl.ResamplerBank, None, df.data_ptr(), 8), "q15": (xl.ResamplerBankQ15, None, dq.data_ptr(), 4),
            "q15_sums_in_64_bits": (xl.ResamplerBankQ15, "1", dq.data_ptr(), 4),
            "q15_taps_in_place": (xl.ResamplerBankQ15, "2", dq.data_ptr(), 4)}
    banks, res, ops = {}, {}, {}
    for name, (cls, knob, base, esz) in arms.items():
        if knob is None:
            os.environ.pop("XL_EXP_RSQ", None)
        else:
            os.environ["XL_EXP_RSQ"] = knob
        bank = cls()
        ids = [bank.add(rs.L, rs.M, taps) for _ in range(nstreams)]
        banks[name] = (bank, ids, [base + esz * per * i for i in range(nstreams)])
        res[name] = {"host_s": [], "device_s": []}
    os.environ.pop("XL_EXP_RSQ", None)
    counts = [per] * nstreams
    for k in range(reps + warm):
        for name, (bank, ids, ptrs) in banks.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(st)
            t0 = time.perf_counter()
            bank.feed(ids, ptrs, counts, st.cuda_stream)
            t1 = time.perf_counter()
            b.record(st)
            b.synchronize()
            ops[name] = bank.last_feed_ops()
            if k >= warm:
                res[name]["host_s"].append(t1 - t0)
                res[name]["device_s"].append(a.elapsed_time(b) * 1e-3)
    out = {"case": f"{nstreams} x 48 kHz on 10 Msps: D 125, then 3/5 with {taps.size} taps; one feed of all streams per bank, alternating",
           "streams": nstreams, "samples_per_stream_per_feed": per,
           "outputs_per_stream_per_feed": banks["q15"][0].produced(banks["q15"][1][0]) / (reps + warm)}
    for name, (bank, ids, ptrs) in banks.items():
        out[name] = {m: stats(v) for m, v in res[name].items()}
        out[name]["last_feed_ops"] = ops[name]
        out[name]["tables"], out[name]["table_bytes"] = bank.stats()[1:]
        bank.close()
    for name in banks:
        if name != "float":
            out[name]["device_vs_float"] = out[name]["device_s"]["median"] / out["float"]["device_s"]["median"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--streams", type=int, default=1024)
    ap.add_argument("--out")
    ap.add_argument("--q15", action="store_true", help="the Q15 bank beside the float bank (the yardstick), not the bank beside a loop")
    a = ap.parse_args()
    if "no usable device" in xl.device_info():
        raise SystemExit("resample_bank_bench needs a HIP device: " + xl.device_info())
    res = {"device": xl.device_info(), "feeds": (bench_q15 if a.q15 else bench)(a.streams, a.reps)}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
