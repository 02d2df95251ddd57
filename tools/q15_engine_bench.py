"""Measurement of the Q15 engine call with and without the matrix-core FIR (engine option "q15_kernel"; csrc/q15mm/xl_q15_mm.hip).

  One process, two engines per shape -- option 0 (the float64 launches: the yardstick, untouched by the option) and option 1 -- fed the
  same device blocks, alternating call by call.  HIP events around each call; median, minimum and maximum of `reps` calls after warm-up.
  After the timed calls every client's rows of the two engines are compared bit for bit.  The GPU's clocks (rocm-smi --showclocks, a
  read) are recorded before and after.

  Shapes: the headline shape -- 1024 clients, D = 42, 505 taps, blocks of 131072 samples -- in cu8 and cs16, at 8 blocks and at 1 block
  per call, and tests/q15_extremes_cases.MIX_CLIENTS_BIG as a small mixed population (82 clients of five shapes, cu8, one block).

  --profile-only SHAPE: a few calls of one shape and nothing else, for a run under `rocprofv3 --kernel-trace --stats`.

  --q15-nco: the axis of engine option "q15_nco" (the phase table tabulated a call ahead on the side stream) instead: per shape, in the
  same process and alternating call by call, engines (q15_kernel, q15_nco) = (1, 0) -- the yardstick --, (1, 1) and (0, 1) fed equal calls
  (every look-ahead used), and a pair (1, 0), (1, 1) whose every timed call is followed by an untimed one-block call of another length,
  so that every timed call of the (1, 1) engine finds a look-ahead of the wrong shape: the price of a miss.  Rows compared bit for bit
  after the run, the steady engines against (1, 0), the pair against each other.  With --profile-only the same engines, fewer calls.

usage: python tools/q15_engine_bench.py [--q15-nco] [--reps N] [--out FILE.json] [--txt FILE.txt] [--profile-only headline_cu8_g8]
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]
os.environ.setdefault("XL_TESTING", "1")

import sdr_server_amd as xl  # noqa: E402

FS = 2016000
S = 131072  # samples per block of the headline shape


def clocks():
    try:
        r = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=60)
        return [ln.strip() for ln in r.stdout.splitlines() if "sclk" in ln or "mclk" in ln][:4]
    except Exception as e:  # (no rocm-smi on this host: the run still counts, without the clocks)
        return [f"unavailable: {e}"]


def shapes():
    import q15_extremes_cases as QC

    d42 = QC.taps("d42")
    head = [(42, d42, -1000000 + 1953 * c) for c in range(1024)]
    mixed = [(QC.SHAPE_D[s], QC.taps(s), fc) for s, fc in QC.MIX_CLIENTS_BIG]
    return {"headline_cu8_g8": ("cu8", head, S, 8), "headline_cu8_g1": ("cu8", head, S, 1), "headline_cs16_g8": ("cs16", head, S, 8),
            "headline_cs16_g1": ("cs16", head, S, 1), "mixed82_cu8_g1": ("cu8", mixed, QC.MIX_N // 2, 1)}


def stats(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v)), "n": len(v)}


def run_shape(name, fmt, clients, samples, G, reps, warm=3, options=(0, 1)):
    import torch

    st = torch.cuda.current_stream()
    npdt = {"cu8": np.uint8, "cs16": np.int16}[fmt]
    rng = np.random.default_rng(7)
    info = np.iinfo(npdt)
    blocks = [torch.from_numpy(rng.integers(info.min, info.max + 1, 2 * samples * G, dtype=npdt)).cuda() for _ in range(2)]
    engs = {}
    for opt in options:
        eng = xl.BatchEngine(FS, fmt, 2 * samples, group_blocks=G)
        eng.set_option("q15_kernel", opt)
        engs[opt] = (eng, [eng.add_client(D, t, fc) for D, t, fc in clients])
    ms = {opt: [] for opt in options}
    for k in range(reps + warm):
        x = blocks[k & 1]
        for opt in options:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(st)
            engs[opt][0].process_device_group(x.data_ptr(), 2 * samples, G, "q15", st.cuda_stream)
            b.record(st)
            b.synchronize()
            if k >= warm:
                ms[opt].append(a.elapsed_time(b))
    out = {"shape": name, "format": fmt, "clients": len(clients), "samples_per_block": samples, "blocks_per_call": G,
           "describe": {str(opt): engs[opt][0].describe() for opt in options}}
    for opt in options:
        out[f"q15_kernel_{opt}"] = {"call_us": stats([1e3 * v for v in ms[opt]]),
                                    "us_per_block": float(np.median(ms[opt])) * 1e3 / G}
    if len(options) == 2:
        rows = []
        for opt in options:
            eng, ids = engs[opt]
            eng.fetch()
            rows.append([eng.output_cs16(cid) for cid in ids])
        out["clients_compared"] = len(rows[0])
        out["bit_identical"] = all(a.shape == b.shape and np.array_equal(a, b) for a, b in zip(*rows))
        out["speedup"] = out["q15_kernel_0"]["call_us"]["median"] / out["q15_kernel_1"]["call_us"]["median"]
    for eng, _ in engs.values():
        eng.close()
    return out


NCO_ENGINES = (("k1n0", 1, 0, False), ("k1n1", 1, 1, False), ("k0n1", 0, 1, False), ("k1n0_alt", 1, 0, True), ("k1n1_miss", 1, 1, True))
ALT_SAMPLES = 4200  # the untimed call between the timed calls of the alternating pair: one block of this many samples


def run_nco_shape(name, fmt, clients, samples, G, reps, warm=3):
    import torch

    st = torch.cuda.current_stream()
    npdt = {"cu8": np.uint8, "cs16": np.int16}[fmt]
    rng = np.random.default_rng(7)
    info = np.iinfo(npdt)
    blocks = [torch.from_numpy(rng.integers(info.min, info.max + 1, 2 * samples * G, dtype=npdt)).cuda() for _ in range(2)]
    engs = {}
    for tag, qk, qn, _ in NCO_ENGINES:
        eng = xl.BatchEngine(FS, fmt, 2 * samples, group_blocks=G)
        eng.set_option("q15_kernel", qk)
        eng.set_option("q15_nco", qn)
        engs[tag] = (eng, [eng.add_client(D, t, fc) for D, t, fc in clients])
    ms = {tag: [] for tag, _, _, _ in NCO_ENGINES}
    for k in range(reps + warm):
        x = blocks[k & 1]
        for tag, _, _, alt in NCO_ENGINES:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(st)
            engs[tag][0].process_device_group(x.data_ptr(), 2 * samples, G, "q15", st.cuda_stream)
            b.record(st)
            b.synchronize()
            if k >= warm:
                ms[tag].append(a.elapsed_time(b))
            if alt and k + 1 < reps + warm:
                engs[tag][0].process_device_group(x.data_ptr(), 2 * ALT_SAMPLES, 1, "q15", st.cuda_stream)
                engs[tag][0].sync()
    out = {"shape": name, "format": fmt, "clients": len(clients), "samples_per_block": samples, "blocks_per_call": G,
           "describe": {tag: engs[tag][0].describe() for tag in engs}}
    rows = {}
    for tag, (eng, ids) in engs.items():
        out[tag] = {"call_us": stats([1e3 * v for v in ms[tag]])}
        eng.fetch()
        rows[tag] = [eng.output_cs16(cid) for cid in ids]

    def same(p, q):
        return all(a.shape == b.shape and a.shape[0] > 0 and np.array_equal(a, b) for a, b in zip(rows[p], rows[q]))

    out["clients_compared"] = len(clients)
    out["bit_identical"] = same("k1n0", "k1n1") and same("k1n0", "k0n1") and same("k1n0_alt", "k1n1_miss")
    for eng, _ in engs.values():
        eng.close()
    return out


def nco_main(a, sh):
    if a.profile_only:
        fmt, clients, samples, G = sh[a.profile_only]
        print(json.dumps(run_nco_shape(a.profile_only, fmt, clients, samples, G, 6, warm=2)))
        return
    res = {"device": xl.device_info(), "clocks_before": clocks(), "shapes": []}
    for name, (fmt, clients, samples, G) in sh.items():
        res["shapes"].append(run_nco_shape(name, fmt, clients, samples, G, a.reps))
    res["clocks_after"] = clocks()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    if a.txt:
        with open(a.txt, "w") as f:
            f.write("Q15 engine call, option q15_nco; engines (q15_kernel, q15_nco); one process, alternating calls, HIP events around the call,\n"
                    "median (min - max) of %d calls in us; rows compared bit for bit after the run.  alt / miss: every timed call follows an\n"
                    "untimed one-block call of %d samples, so the (1, 1) engine's look-ahead is always of the wrong shape\n\n" % (a.reps, ALT_SAMPLES))
            f.write("%-18s %7s %6s  %-25s %-25s %-25s %-25s %-25s %s\n" % ("shape", "clients", "blocks", "(1, 0)", "(1, 1) all used", "(0, 1) all used",
                                                                       "(1, 0) alt", "(1, 1) all missed", "identical"))
            for s in res["shapes"]:
                cells = ["%.1f (%.1f - %.1f)" % (s[t]["call_us"]["median"], s[t]["call_us"]["min"], s[t]["call_us"]["max"]) for t, _, _, _ in NCO_ENGINES]
                f.write("%-18s %7d %6d  %-25s %-25s %-25s %-25s %-25s %s\n" % ((s["shape"], s["clients"], s["blocks_per_call"]) + tuple(cells) + (s["bit_identical"],)))
            f.write("\n")
            for s in res["shapes"]:
                f.write("%s (1, 1): %s\n%s miss:   %s\n" % (s["shape"], s["describe"]["k1n1"], s["shape"], s["describe"]["k1n1_miss"]))
            f.write("\nclocks before: %s\nclocks after:  %s\n%s\n" % (res["clocks_before"], res["clocks_after"], res["device"]))
    if not all(s["bit_identical"] for s in res["shapes"]):
        raise SystemExit("the engines differ")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--q15-nco", action="store_true")
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--out")
    ap.add_argument("--txt")
    ap.add_argument("--profile-only", metavar="SHAPE")
    a = ap.parse_args()
    if "no usable device" in xl.device_info():
        raise SystemExit("q15_engine_bench needs a HIP device: " + xl.device_info())
    sh = shapes()
    if a.q15_nco:
        return nco_main(a, sh)
    if a.profile_only:
        fmt, clients, samples, G = sh[a.profile_only]
        print(json.dumps(run_shape(a.profile_only, fmt, clients, samples, G, 6, warm=2)))
        return
    res = {"device": xl.device_info(), "clocks_before": clocks(), "shapes": []}
    for name, (fmt, clients, samples, G) in sh.items():
        res["shapes"].append(run_shape(name, fmt, clients, samples, G, a.reps))
    res["clocks_after"] = clocks()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    if a.txt:
        with open(a.txt, "w") as f:
            f.write("Q15 engine call, option q15_kernel 0 (float64 launches) against 1 (matrix-core launch); one process, alternating calls,\n"
                    "HIP events around the call, median (min - max) of %d calls in us; rows compared bit for bit after the run\n\n" % a.reps)
            f.write("%-18s %8s %7s  %-28s %-28s %8s %s\n" % ("shape", "clients", "blocks", "option 0", "option 1", "speedup", "identical"))
            for s in res["shapes"]:
                c0, c1 = s["q15_kernel_0"]["call_us"], s["q15_kernel_1"]["call_us"]
                f.write("%-18s %8d %7d  %-28s %-28s %7.2fx %s\n" % (
                    s["shape"], s["clients"], s["blocks_per_call"], "%.1f (%.1f - %.1f)" % (c0["median"], c0["min"], c0["max"]),
                    "%.1f (%.1f - %.1f)" % (c1["median"], c1["min"], c1["max"]), s["speedup"], s["bit_identical"]))
            f.write("\nclocks before: %s\nclocks after:  %s\n%s\n" % (res["clocks_before"], res["clocks_after"], res["device"]))
    if not all(s["bit_identical"] for s in res["shapes"]):
        raise SystemExit("the two engines differ")


if __name__ == "__main__":
    main()
