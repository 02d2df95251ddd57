"""Measurements of the spectrum bank (csrc/xl_spectrum_bank.hip, include/xlating_spectrum.h); prints one JSON object.

  feeds      one bank feed of all streams against what the single-stream object offers for the same job: a loop of
             xlating_spectrum_feed_device over one xl.Spectrum per stream, in the same process, on the same device buffers, alternating.
             Two measures per repetition: host time of the feed call(s) (the enqueue: neither waits for the device) and device time
             between events recorded before the first and behind the last queued operation.  Median, minimum and maximum over `reps`
             repetitions after warm-up; rows are taken outside the timed windows.  Cases: 1024 streams x 48 kHz rows at W = 256 with the
             headline call's 24 966 samples per stream, 64 streams of two rates (48 / 96 kHz), and 1024 streams at W = 1000 (Bluestein).
             (The loop's objects are created with XL_EXP_SPEC_CHUNK=65536: their host staging, which a device feed never touches, would
             otherwise pin 32 MiB per object.)
  engine     the headline shape (1024 clients x 48 kHz, D = 42, 505 taps, 8 blocks per call, optimized, the engine's own stream): time per
             call with and without SpectrumBank.feed_engine of all clients behind every call (record_event ordering; the feed is waited
             for before the next call, which reuses the device rows), alternating in one process; the feed's device time and the
             host time of the Python gather of the 1024 output pointers are reported beside them.

  --wide     (alone) the wide bank: 1024 streams x 48 000 Hz at W = 48 000 (1 Hz per bin; Bluestein at N = 131072, F = 1), fed the
             headline call's 24 966 samples per stream, against a loop over 1024 xlating_spectrum_create_wide objects in the same
             process.  Every other feed completes no transform (the samples go to the carries); the others run 1024 transforms and
             complete 1024 rows: the two kinds are reported apart, each with the bank's launches and copies per feed.  (The loop's
             objects are created with a scratch of one transform, XL_EXP_SPEC_SCRATCH = 1 MiB -- a feed of theirs never runs more --
             instead of 64 MiB each; the bank keeps its default scratch and staging.)

usage: python tools/spectrum_bank_bench.py [--reps N] [--skip-engine] [--skip-loop] [--wide] [--out FILE]
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
os.environ.setdefault("XL_TESTING", "1")

import sdr_server_amd as xl  # noqa: E402


def stats(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v)), "n": len(v)}


def feeds_bench(name, W, rates, counts, reps, warm=3, with_loop=True):
    """rates[i], counts[i]: stream i's row length and samples per feed"""
    import torch

    n = len(rates)
    d = torch.randn(2 * int(sum(counts)), device="cuda", dtype=torch.float32) * 0.3
    offs = np.concatenate([[0], np.cumsum(counts)[:-1]])
    ptrs = [d.data_ptr() + 8 * int(o) for o in offs]
    st = torch.cuda.current_stream()
    bank = xl.SpectrumBank(W, "cf32")
    ids = [bank.add(r) for r in rates]
    objs = []
    if with_loop:
        os.environ["XL_EXP_SPEC_CHUNK"] = "65536"
        objs = [xl.Spectrum(r, W, "cf32") for r in rates]
        os.environ.pop("XL_EXP_SPEC_CHUNK")
    S = xl.spectrum_lib()
    res = {"bank": {"host_s": [], "device_s": []}, "loop": {"host_s": [], "device_s": []}}
    ops = None
    for k in range(reps + warm):
        for which in ("bank", "loop") if with_loop else ("bank",):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(st)
            t0 = time.perf_counter()
            if which == "bank":
                bank.feed(ids, ptrs, counts, st.cuda_stream)
            else:
                for o, p, c in zip(objs, ptrs, counts):
                    S.xlating_spectrum_feed_device(o.h, p, c, st.cuda_stream)
            t1 = time.perf_counter()
            b.record(st)
            b.synchronize()
            if which == "bank":
                ops = bank.last_feed_ops()
                for i in ids:
                    if bank.rows_pending(i):
                        bank.take_rows(i)
            else:
                for o in objs:
                    o.take_rows()
            if k >= warm:
                res[which]["host_s"].append(t1 - t0)
                res[which]["device_s"].append(a.elapsed_time(b) * 1e-3)
    bank.close()
    for o in objs:
        o.close()
    out = {"case": name, "streams": n, "W": W, "samples_per_feed": int(sum(counts)), "bank_last_feed_ops": ops,
           "transform": "bluestein" if W & (W - 1) else "radix-4"}
    for which in res:
        if res[which]["host_s"]:
            out[which] = {m: stats(v) for m, v in res[which].items()}
    if with_loop:
        out["host_speedup"] = out["loop"]["host_s"]["median"] / out["bank"]["host_s"]["median"]
        out["device_speedup"] = out["loop"]["device_s"]["median"] / out["bank"]["device_s"]["median"]
        # the one threshold: not slower than the loop beyond the spread of the repetitions
        out["bank_not_slower"] = bool(all(out["bank"][m]["median"] <= out["loop"][m]["median"] +
                                          (out["loop"][m]["max"] - out["loop"][m]["min"]) for m in ("host_s", "device_s")))
    return out


def wide_bench(reps, warm=2, n=1024, W=48000, rate=48000, count=24966, with_loop=True):
    """-> the --wide case: per kind of feed ("quiet": no transform completes, "rows": every stream completes a row) host and device
    time of the bank's feed and of the loop over single wide objects, and the bank's (launches, copies)"""
    import torch

    d = torch.randn(2 * n * count, device="cuda", dtype=torch.float32) * 0.3
    ptrs = [d.data_ptr() + 8 * i * count for i in range(n)]
    counts = [count] * n
    st = torch.cuda.current_stream()
    bank = xl.SpectrumBank(W, "cf32", wide=True)
    ids = [bank.add(rate) for _ in range(n)]
    objs = []
    if with_loop:
        N = 1
        while N < 2 * W - 1:
            N *= 2
        os.environ["XL_EXP_SPEC_CHUNK"] = "65536"
        os.environ["XL_EXP_SPEC_SCRATCH"] = str(8 * N)
        objs = [xl.Spectrum(rate, W, "cf32", wide=True) for _ in range(n)]
        os.environ.pop("XL_EXP_SPEC_CHUNK")
        os.environ.pop("XL_EXP_SPEC_SCRATCH")
    S = xl.spectrum_lib()
    res = {k: {w: {"host_s": [], "device_s": []} for w in ("bank", "loop")} for k in ("quiet", "rows")}
    ops = {}
    for k in range(2 * (reps + warm)):
        kind, first = None, {}  # this repetition's kind of feed (decided by the bank's feed, which runs first) and first stream's rows
        for which in ("bank", "loop") if with_loop else ("bank",):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(st)
            t0 = time.perf_counter()
            if which == "bank":
                bank.feed(ids, ptrs, counts, st.cuda_stream)
            else:
                assert kind is not None
                for o, p in zip(objs, ptrs):
                    S.xlating_spectrum_feed_device(o.h, p, count, st.cuda_stream)
            t1 = time.perf_counter()
            b.record(st)
            b.synchronize()
            if which == "bank":
                rows = sum(bank.rows_pending(i) for i in ids)
                assert rows in (0, n)
                kind = "rows" if rows else "quiet"
                ops[kind] = bank.last_feed_ops()
                first[which] = bank.take_rows(ids[0])
                for i in ids[1:] if rows else []:
                    bank.take_rows(i)
            else:  # (the loop's feed of the same samples: the same kind, and the same first row)
                first[which] = objs[0].take_rows()
                assert first[which][0].shape[0] == (1 if kind == "rows" else 0)
                for o in objs[1:] if kind == "rows" else []:
                    o.take_rows(1)
                assert all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(first["bank"], first["loop"]))
            if k >= 2 * warm:
                res[kind][which]["host_s"].append(t1 - t0)
                res[kind][which]["device_s"].append(a.elapsed_time(b) * 1e-3)
    bank.close()
    for o in objs:
        o.close()
    out = {"case": f"wide: {n} x {rate} Hz, W {W}", "streams": n, "W": W, "samples_per_feed": n * count, "transform": "two-level bluestein"}
    for kind in res:
        out[kind] = {"bank_last_feed_ops": ops.get(kind)}
        for which in res[kind]:
            if res[kind][which]["host_s"]:
                out[kind][which] = {m: stats(v) for m, v in res[kind][which].items()}
        if with_loop:
            out[kind]["host_speedup"] = out[kind]["loop"]["host_s"]["median"] / out[kind]["bank"]["host_s"]["median"]
            out[kind]["device_speedup"] = out[kind]["loop"]["device_s"]["median"] / out[kind]["bank"]["device_s"]["median"]
    return out


def engine_bench(reps, W=256, warm=4):
    import torch

    import siggen

    band, nbytes, G = 2016000, 262144, 8
    code, taps = xl.create_low_pass_filter(1.0, band, 24000, 9600)
    assert code == 0
    eng = xl.BatchEngine(band, "cu8", nbytes, group_blocks=G)
    ids = [eng.add_client(42, taps, -900000 + 1758 * c) for c in range(1024)]
    bank = xl.SpectrumBank(W, "cf32")
    sid = {cid: bank.add(48000) for cid in ids}
    d = torch.from_numpy(siggen.xs_u8(99, G * nbytes)).cuda()
    st = torch.cuda.current_stream()
    ev = torch.cuda.Event()
    ev.record(st)
    torch.cuda.synchronize()
    t = {"without": [], "with": [], "feed_device_s": [], "gather_host_s": []}
    for k in range(2 * (reps + warm)):
        which = "with" if k % 2 else "without"
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        eng.process_device_group(d.data_ptr(), nbytes, G, "optimized", "engine")
        if which == "with":
            eng.record_event(ev.cuda_event)
            st.wait_event(ev)
            g0 = time.perf_counter()
            args = bank.gather_engine(eng, sid)  # (1024 host-side lookups through ctypes)
            g1 = time.perf_counter()
            a.record(st)
            bank.feed(*args, st.cuda_stream)
            b.record(st)
            t["gather_host_s"].append(g1 - g0)
            st.synchronize()
        eng.sync()
        t1 = time.perf_counter()
        if which == "with":
            for s in sid.values():
                if bank.rows_pending(s):
                    bank.take_rows(s)
        if k >= 2 * warm:
            t[which].append(t1 - t0)
            if which == "with":
                t["feed_device_s"].append(a.elapsed_time(b) * 1e-3)
    desc = eng.describe()
    bank.close()
    eng.close()
    return {"shape": "1024 clients x 48 kHz, D 42, 505 taps, 8 blocks of 262144 bytes per call, optimized, XL_STREAM_ENGINE", "W": W,
            "plan": desc, "call_s_without_feed": stats(t["without"]), "call_s_with_feed": stats(t["with"]),
            "feed_device_s": stats(t["feed_device_s"]), "python_gather_host_s": stats(t["gather_host_s"][warm:])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--skip-engine", action="store_true")
    ap.add_argument("--skip-loop", action="store_true")
    ap.add_argument("--wide", action="store_true", help="the wide bank's case alone: 1024 streams of 48 000 Hz at W = 48 000")
    ap.add_argument("--out")
    a = ap.parse_args()
    if "no usable device" in xl.device_info():
        raise SystemExit("spectrum_bank_bench needs a HIP device: " + xl.device_info())
    if a.wide:
        line = json.dumps({"device": xl.device_info(), "wide": wide_bench(a.reps, with_loop=not a.skip_loop)})
        print(line)
        if a.out:
            with open(a.out, "w") as f:
                f.write(line + "\n")
        return
    res = {"device": xl.device_info(), "feeds": []}
    cases = [("1024 x 48 kHz, W 256", 256, [48000] * 1024, [24966] * 1024),
             ("64 of two rates, W 256", 256, [48000, 96000] * 32, [24966, 49932] * 32),
             ("1024 x 48 kHz, W 1000", 1000, [48000] * 1024, [24966] * 1024)]
    for name, W, rates, counts in cases:
        res["feeds"].append(feeds_bench(name, W, rates, counts, a.reps, with_loop=not a.skip_loop))
        print(json.dumps(res["feeds"][-1]), file=sys.stderr, flush=True)
    if not a.skip_engine:
        res["engine"] = engine_bench(a.reps)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
