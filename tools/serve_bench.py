#!/usr/bin/env python3
"""tools/serve_bench.py -- what the serve object (include/xlating_serve.h) costs and saves at the headline population: 1024 clients x
48 kHz in a band of 2016000 Hz, the server's own 505-tap filter, cu8, 8 blocks of 262144 bytes per call; both output families.  Every
client's sink is a pipe, and one reader thread drains them all.

  (a) the pack kernels: HIP events around the pack launch of one call's rows, around the NARROWING pack launch of the same rows
      (xlating_delivery_pack_device_cs16: the same bytes read, half of them written) and around a hipMemcpyAsync device-to-device
      copy of the same bytes, alternating in one process, in rounds (--pack; run it under `rocprofv3 --kernel-trace --stats` for the
      kernels' own times)
  (b) the call period: a host clock around bursts of BURST calls, each burst ending in a flush and a synchronise INSIDE the clock, for
      three loops alternating in one process, three rounds: the parent's (process_host_group + fetch + sinks.submit), Serve with
      overlap 0, Serve with overlap 1.  Every loop is timed for the same work: BURST calls, BURST deliveries (with overlap 1 the flush
      hands the last call's rows over) and the drain of the queues into the pipes.  A burst is what the clients' queues hold, because
      the sinks cannot take 204 MB per call at the rate the device produces them (nobody is dropped; the tool checks); bursts repeat
      until at least a second has been timed
  (c) cs16: the bytes Serve moves to the host per call (counted) against what xlating_batch_fetch copies after a Q15 call (the whole
      arena in float2-sized rows), and the two call periods
  (d) cf32-cs16 (--families cf32,cs16,cf32-cs16): the cf32 family's engine call, its rows narrowed to cs16 by the delivery; its parent
      loop is the cf32 family's (the parent has no such delivery)

  (e) --gain: only the pack launch with a gain and a level a row (xlating_delivery_pack_device_cs16_gain, every gain 0: the same
      bytes) against the narrowing pack launch it grew from (xlating_delivery_pack_device_cs16, xl_dlv_narrow_kernel) on the same
      batch, the rows of the headline call; HIP events, the two alternating in one process, the spread of each over its rounds
      reported (profiles/serve_gain_vs_parent.txt)

  (f) --tune: only the call period of Serve (cf32, overlap 0 and 1) with EVERY client tuned (xlating_serve_set_tune, a shift and a
      ramp of its own each: one tuner-bank feed more per call) against the same object untuned, the loops alternating in one
      process as in (b); the untuned loop's spread over its rounds is reported (profiles/tune_bank_vs_pack.txt)

  (g) --squelch FRACTIONS (e.g. 1.0,0.25,0.05): the call period and the bytes to the host per call of Serve (--families, overlap 0
      and 1) with EVERY client squelched (xlating_serve_set_squelch) and that fraction of the gates open, against the same object
      with no squelch set, the loops alternating in one process as in (b).  The capture is noise, and the fraction is made by
      per-client marks: (0, 0) never closes, marks far above the noise never open -- the figures measure bytes, not detection.  Then
      the meter alone: HIP events around one measurement of the headline call's rows (table upload, launch, copy back) against the
      plain pack launch of the same rows, alternating in one process (profiles/serve_squelch_vs_parent.txt)

Prints a report; profiles/serve_vs_parent.txt is one run of it on an MI355X."""
import argparse
import os
import select
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("XL_TESTING", "1")
import numpy as np  # noqa: E402

import sdr_server_amd as xl  # noqa: E402

BAND_RATE, BAND_FREQ, BUFFER, RATE = 2016000, 460100000, 262144, 48000


class Drain(threading.Thread):
    """one thread reading every pipe empty, until closed"""

    def __init__(self):
        super().__init__(daemon=True)
        self.poll, self.fds, self.bytes, self.stop = select.epoll(), {}, 0, False
        self.lock = threading.Lock()
        self.null = os.open(os.devnull, os.O_WRONLY)
        self.start()

    def pipes(self, n):
        """n write ends, made once and shared by the loops that run in turn"""
        while len(self.fds) < n:
            self.pipe()
        with self.lock:
            return list(self.fds.values())[:n]

    def pipe(self):
        r, w = os.pipe()
        os.set_blocking(r, False)
        try:
            import fcntl
            fcntl.fcntl(w, 1031, 1 << 20)  # F_SETPIPE_SZ (best effort: the per-user limit may refuse it)
        except OSError:
            pass
        with self.lock:
            self.fds[r] = w
        self.poll.register(r, select.EPOLLIN)
        return w

    def run(self):
        while not self.stop:
            for fd, _ in self.poll.poll(0.05):
                try:
                    while True:  # (to /dev/null without a copy through this process)
                        got = os.splice(fd, self.null, 1 << 20)
                        if got == 0:
                            break
                        self.bytes += got
                except (BlockingIOError, OSError):
                    pass

    def close(self):
        self.stop = True
        self.join()
        for r, w in self.fds.items():
            os.close(r), os.close(w)


def centers(n):
    return [BAND_FREQ - 900000 + (1800000 // n) * c for c in range(n)]


def make_serve(n, family, overlap, group, drain, out_dir):
    s = xl.Serve(BAND_RATE, "cu8", BUFFER, out_dir, family=family, native=False, any_rate=True, overlap=overlap, group_blocks=group,
                 writer_threads=8, queue_bytes=(BURST + 2) * group * (BUFFER // 2 // 42 + 8) * 8, delivery_slots=2)
    s.engine().set_option("expected_clients", min(n, 8192))
    s.ids = []  # the ids the requests returned
    for c, w in zip(centers(n), drain.pipes(n)):
        code, _, cid = s.request(xl.wire_build_request(c, RATE, BAND_FREQ, 1), socket_fd=w)
        assert code == 0
        s.ids.append(cid)
    return s


def make_parent(n, variant, group, drain):
    eng = xl.BatchEngine(BAND_RATE, "cu8", BUFFER, group_blocks=group)
    eng.set_option("expected_clients", min(n, 8192))
    sinks = xl.Sinks(writer_threads=8, queue_bytes=(BURST + 2) * group * (BUFFER // 2 // 42 + 8) * 8)
    for c, w in zip(centers(n), drain.pipes(n)):
        req = xl.WireRequest(c, RATE, BAND_FREQ, 1)
        code, adm, why = xl.wire_admit(req, BAND_RATE, 0, 5)
        assert code == 0
        cid = xl.wire_add_client(eng, adm, BAND_RATE)
        assert sinks.attach_fd(cid, w) == 0
    return eng, sinks


BURST = 8  # calls per timed burst; the queues hold BURST + 2 calls


def period(step, sync, flush, x, seconds):
    """seconds per call of `step` over bursts of BURST calls, each ending in `flush` (the hand-over of what is still owed and the
    sinks' drain) and `sync`, all inside the clock, until `seconds` have been timed"""
    step(x), step(x), flush(), sync()
    n, timed = 0, 0.0
    while timed < seconds:
        t0 = time.perf_counter()
        for _ in range(BURST):
            step(x)
        flush()
        sync()
        timed += time.perf_counter() - t0
        n += BURST
    return timed / n, n


def run_periods(args, family, drain, out):
    import torch

    variant = "q15" if family == "cs16" else "optimized"  # ("cf32-cs16" runs the cf32 family's engine call)
    x = np.random.default_rng(1).integers(0, 256, BUFFER * args.group, dtype=np.uint8)
    eng, sinks = make_parent(args.clients, variant, args.group, drain)
    serves = {ov: make_serve(args.clients, family, ov, args.group, drain, args.out) for ov in (0, 1)}

    def parent_step(x):
        eng.process_host_group(x, args.group, variant)
        eng.fetch()
        if family != "cs16":
            sinks.submit(eng)  # (after a Q15 call submit queues nothing: the parent has no cs16 delivery; its loop is engine + fetch)

    loops = {"parent": (parent_step, torch.cuda.synchronize, sinks.flush)}
    for ov, s in serves.items():
        loops[f"serve overlap={ov}"] = (lambda x, s=s: s.blocks_host(x, args.group), torch.cuda.synchronize, s.flush)
    res = {k: [] for k in loops}
    for rnd in range(args.rounds):
        for name, (step, sync, flush) in loops.items():
            res[name].append(period(step, sync, flush, x, args.seconds))
    out.append(f"[{family}] call period, {args.clients} clients x {RATE} Hz, {args.group} blocks per call, sinks: pipes drained by one thread, bursts of {BURST} calls")
    for name, rs in res.items():
        ms = [1e3 * p for p, _ in rs]
        out.append(f"  {name:18s} ms per call, rounds: " + "  ".join(f"{m:8.3f}" for m in ms) + f"   (calls per round: {[n for _, n in rs]})")
    pm = [p for p, _ in res["parent"]]
    spread = (max(pm) - min(pm)) / min(pm)
    out.append(f"  parent's spread over its rounds: {100 * spread:.1f} %")
    for name in list(loops)[1:]:
        r = np.median([p for p, _ in res[name]]) / np.median(pm)
        out.append(f"  {name}: median period / parent's median = {r:.3f}")
    dropped = {ov: len(s.dropped()) for ov, s in serves.items()}
    failed = len(sinks.failed())
    out.append(f"  clients dropped by back-pressure: parent {failed}, serve {dropped} (a dropped client shortens the calls after it)")
    d2h = serves[0].last_ops()[2]
    lens = [eng.output_len(c) for c in range(args.clients)]
    arena = 8 * sum(lens)  # what the fetch copies: float2-sized rows whatever they hold (a lower bound: rows are padded)
    out.append(f"  bytes to the host per call: serve {d2h} (counted), parent's fetch >= {arena} (8 x out_total)")
    for s in serves.values():
        s.close()
    sinks.close()
    eng.close()


def run_pack(args, out):
    """the pack launch of one call's rows, the narrowing pack launch of the same rows and a device-to-device copy of the same bytes,
    in turn, args.rounds rounds of args.pack_iters each"""
    import torch

    esz, rows = 8, args.group * (BUFFER // 2 // 42)
    n = args.clients
    src = (0.3 * torch.randn((n * (rows * esz + 64) // 4,), dtype=torch.float32, device="cuda")).view(torch.uint8)
    dst = torch.empty_like(src)
    ptrs = [src.data_ptr() + i * (rows * esz + 64) for i in range(n)]
    d = xl.Delivery(2)
    st = torch.cuda.Stream()
    total = n * rows * esz
    keys = list(range(n))

    def timed(what):
        a, b = (torch.cuda.Event(enable_timing=True) for _ in range(2))
        with torch.cuda.stream(st):
            a.record()
            if what == "d2d":
                dst[:total].copy_(src[:total], non_blocking=True)
            elif what == "pack":
                t = d.pack(keys, ptrs, [rows * esz] * n, st.cuda_stream)
            else:
                t = d.pack_cs16(keys, ptrs, [rows] * n, st.cuda_stream)
            b.record()
        if what != "d2d":
            d.wait(t)
            d.release(t)
        st.synchronize()
        return a.elapsed_time(b)

    names = ("pack", "narrow", "d2d")
    for what in names:  # (the slots' buffers, the table, the clocks)
        for _ in range(3):
            timed(what)
    med = {k: [] for k in names}
    for rnd in range(args.rounds):
        for what in names:
            med[what].append(float(np.median([timed(what) for _ in range(args.pack_iters)])))
    moved = {"pack": 2 * total, "narrow": total + total // 2, "d2d": 2 * total}
    label = {"pack": "table upload + pack launch", "narrow": "table upload + narrowing pack launch", "d2d": "device-to-device copy of the same bytes"}
    out.append(f"[pack] {n} rows of {rows * esz} bytes = {total / 1e6:.1f} MB of cf32; HIP events on the launch stream, "
               f"{args.rounds} alternating rounds, median of {args.pack_iters} each")
    for k in names:
        m = float(np.median(med[k]))
        out.append(f"  {label[k]:40s} ms, rounds: " + "  ".join(f"{v:7.3f}" for v in med[k]) +
                   f"   median {m:.3f} ms = {moved[k] / m / 1e6:.0f} GB/s read + written ({moved[k] / 1e6:.1f} MB)")
    p, q, c = (float(np.median(med[k])) for k in names)
    spread = max((max(v) - min(v)) / min(v) for v in med.values())
    out.append(f"  pack / copy = {p / c:.2f}; narrowing / plain pack = {q / p:.2f}; largest spread of one launch over its rounds: {100 * spread:.1f} %")
    d.close()


def run_gain(args, out):
    """the narrowing pack launch and the pack launch with gains and levels on the same rows, in turn, args.rounds rounds of
    args.pack_iters each; the events enclose the table's upload, the zeroing of the level table (gain only) and the launch"""
    import torch

    rows, n = args.group * (BUFFER // 2 // 42), args.clients
    src = (0.3 * torch.randn((n * (rows * 8 + 64) // 4,), dtype=torch.float32, device="cuda")).view(torch.uint8)
    ptrs = [src.data_ptr() + i * (rows * 8 + 64) for i in range(n)]
    d = xl.Delivery(2)
    st = torch.cuda.Stream()
    keys, lens, gains = list(range(n)), [rows] * n, [0] * n

    def timed(what):
        a, b = (torch.cuda.Event(enable_timing=True) for _ in range(2))
        with torch.cuda.stream(st):
            a.record()
            t = d.pack_cs16(keys, ptrs, lens, st.cuda_stream) if what == "narrow" else d.pack_device_cs16_gain(keys, ptrs, lens, gains, st.cuda_stream)
            b.record()
        d.wait(t)
        if what == "gain":
            assert d.row_level(t, 0)[0] > 0
        d.release(t)
        st.synchronize()
        return a.elapsed_time(b)

    names = ("narrow", "gain")
    for what in names:
        for _ in range(3):
            timed(what)
    med = {k: [] for k in names}
    for rnd in range(args.rounds):
        for what in names:
            med[what].append(float(np.median([timed(what) for _ in range(args.pack_iters)])))
    label = {"narrow": "table upload + narrowing pack launch (parent)", "gain": "table upload + zeroing + pack launch with gains, levels"}
    out.append(f"[gain] {n} rows of {rows} cf32 samples = {n * rows * 8 / 1e6:.1f} MB read, {n * rows * 4 / 1e6:.1f} MB written; HIP events on the "
               f"launch stream, {args.rounds} alternating rounds, median of {args.pack_iters} each")
    for k in names:
        m, lo, hi = float(np.median(med[k])), min(med[k]), max(med[k])
        out.append(f"  {label[k]:56s} ms, rounds: " + "  ".join(f"{v:7.3f}" for v in med[k]) +
                   f"   median {m:.3f} ms, spread over its rounds {100 * (hi - lo) / lo:.1f} %")
    p, g = (float(np.median(med[k])) for k in names)
    spread = (max(med["narrow"]) - min(med["narrow"])) / min(med["narrow"])
    out.append(f"  with gains and levels / parent = {g / p:.3f}; the parent's own spread is {100 * spread:.1f} %: the difference "
               f"{'exceeds' if abs(g / p - 1.0) > spread else 'lies within'} it")
    d.close()


def run_tune(args, drain, out):
    """the call period with every client tuned against the same run untuned, per overlap, alternating rounds"""
    import torch

    x = np.random.default_rng(1).integers(0, 256, BUFFER * args.group, dtype=np.uint8)
    loops = {}
    serves = []
    for ov in (0, 1):
        for tuned in (False, True):
            s = make_serve(args.clients, "cf32", ov, args.group, drain, args.out)
            if tuned:
                assert len(s.ids) == args.clients
                for i, cid in enumerate(s.ids):
                    s.set_tune(cid, -10000.0 + 20000.0 * i / args.clients, 300.0 - 600.0 * i / args.clients)
            serves.append(s)
            loops[f"overlap={ov} {'tuned  ' if tuned else 'untuned'}"] = (lambda x, s=s: s.blocks_host(x, args.group), torch.cuda.synchronize, s.flush, s)
    res = {k: [] for k in loops}
    for rnd in range(args.rounds):
        for name, (step, sync, flush, _) in loops.items():
            res[name].append(period(step, sync, flush, x, args.seconds))
    out.append(f"[tune] call period, {args.clients} clients x {RATE} Hz, {args.group} blocks per call, cf32, sinks: pipes drained by one thread, "
               f"bursts of {BURST} calls; every client tuned against the same run untuned")
    for name, rs in res.items():
        out.append(f"  {name:18s} ms per call, rounds: " + "  ".join(f"{1e3 * p:8.3f}" for p, _ in rs) +
                   f"   launches, copies behind the engine call: {loops[name][3].last_ops()[:2]}")
    for ov in (0, 1):
        u = [p for p, _ in res[f"overlap={ov} untuned"]]
        t = [p for p, _ in res[f"overlap={ov} tuned  "]]
        spread = (max(u) - min(u)) / min(u)
        r = float(np.median(t) / np.median(u))
        out.append(f"  overlap={ov}: tuned / untuned (medians) = {r:.3f}, + {1e3 * (np.median(t) - np.median(u)):.3f} ms per call; the untuned loop's spread "
                   f"over its rounds is {100 * spread:.1f} %: the difference {'exceeds' if abs(r - 1.0) > spread else 'lies within'} it")
    out.append(f"  clients dropped by back-pressure: {[len(s.dropped()) for s in serves]}")
    for s in serves:
        s.close()


def run_squelch(args, family, fractions, drain, out):
    """the call period with every client squelched and a fraction of the gates open against the same run with no squelch set, per
    overlap, alternating rounds"""
    import torch

    x = np.random.default_rng(1).integers(0, 256, BUFFER * args.group, dtype=np.uint8)
    loops, serves = {}, []
    for ov in (0, 1):
        for fr in [None] + fractions:
            s = make_serve(args.clients, family, ov, args.group, drain, args.out)
            if fr is not None:
                nopen = int(round(fr * args.clients))
                for i, cid in enumerate(s.ids):  # (open gates spread evenly over the band)
                    is_open = (i * nopen) // args.clients != ((i + 1) * nopen) // args.clients
                    s.set_squelch(cid, *((0.0, 0.0) if is_open else (1e30, 1e30)), 0)
            serves.append(s)
            name = f"overlap={ov} " + ("no squelch " if fr is None else f"open {fr:5.3f} ")
            loops[name] = (lambda x, s=s: s.blocks_host(x, args.group), torch.cuda.synchronize, s.flush, s)
    res = {k: [] for k in loops}
    for rnd in range(args.rounds):
        for name, (step, sync, flush, _) in loops.items():
            res[name].append(period(step, sync, flush, x, args.seconds))
    out.append(f"[squelch {family}] call period, {args.clients} clients x {RATE} Hz, {args.group} blocks per call, sinks: pipes drained by one "
               f"thread, bursts of {BURST} calls; every client squelched, a fraction of the gates open, against no squelch set")
    for name, rs in res.items():
        s = loops[name][3]
        st = s.squelch_state(s.ids)
        out.append(f"  {name:22s} ms per call, rounds: " + "  ".join(f"{1e3 * p:8.3f}" for p, _ in rs) +
                   f"   median {1e3 * float(np.median([p for p, _ in rs])):8.3f}   ops behind the engine call {s.last_ops()[:2]}, bytes to the host "
                   f"{s.last_ops()[2]}, gates open {int(st['open'].sum())}")
    for ov in (0, 1):
        u = [p for p, _ in res[f"overlap={ov} no squelch "]]
        spread = (max(u) - min(u)) / min(u)
        out.append(f"  overlap={ov}: the unsquelched loop's spread over its rounds is {100 * spread:.1f} %")
        for fr in fractions:
            t = [p for p, _ in res[f"overlap={ov} open {fr:5.3f} "]]
            out.append(f"    open {fr:5.3f}: squelched / unsquelched (medians) = {float(np.median(t) / np.median(u)):.3f}")
    out.append(f"  clients dropped by back-pressure: {[len(s.dropped()) for s in serves]}")
    for s in serves:
        s.close()


def run_meter(args, out):
    """one measurement of the headline call's rows (table upload, launch, copy back) against the plain pack launch of the same rows,
    in turn, args.rounds rounds of args.pack_iters each"""
    import torch

    esz, rows = 8, args.group * (BUFFER // 2 // 42)
    n = args.clients
    src = (0.3 * torch.randn((n * (rows * esz + 64) // 4,), dtype=torch.float32, device="cuda")).view(torch.uint8)
    ptrs = [src.data_ptr() + i * (rows * esz + 64) for i in range(n)]
    d, m = xl.Delivery(2), xl.Meter()
    st = torch.cuda.Stream()
    keys = list(range(n))

    def timed(what):
        a, b = (torch.cuda.Event(enable_timing=True) for _ in range(2))
        with torch.cuda.stream(st):
            a.record()
            if what == "pack":
                t = d.pack(keys, ptrs, [rows * esz] * n, st.cuda_stream)
            else:
                m.measure("cf32" if what == "meter cf32" else "cs16", ptrs, [rows if what == "meter cf32" else 2 * rows] * n, st.cuda_stream)
            b.record()
        if what == "pack":
            d.wait(t)
            d.release(t)
        else:
            m.wait()
        st.synchronize()
        return a.elapsed_time(b)

    names = ("pack", "meter cf32", "meter cs16")
    for what in names:
        for _ in range(3):
            timed(what)
    med = {k: [] for k in names}
    for rnd in range(args.rounds):
        for what in names:
            med[what].append(float(np.median([timed(what) for _ in range(args.pack_iters)])))
    total = n * rows * esz
    label = {"pack": "table upload + plain pack launch (read + write)", "meter cf32": "table upload + meter launch + copy back, cf32 rows",
             "meter cs16": "the same bytes measured as cs16 rows"}
    out.append(f"[meter] {n} rows of {rows * esz} bytes = {total / 1e6:.1f} MB; HIP events on the launch stream, {args.rounds} alternating rounds, "
               f"median of {args.pack_iters} each; {m.last_ops()} launches, copies per measurement")
    for k in names:
        v = med[k]
        out.append(f"  {label[k]:52s} ms, rounds: " + "  ".join(f"{t:7.3f}" for t in v) +
                   f"   median {float(np.median(v)):.3f} ms, spread {100 * (max(v) - min(v)) / min(v):.1f} %, {total / float(np.median(v)) / 1e6:.0f} GB/s read")
    p = float(np.median(med["pack"]))
    out.append(f"  meter / plain pack: cf32 {float(np.median(med['meter cf32'])) / p:.2f}, cs16 {float(np.median(med['meter cs16'])) / p:.2f}")
    d.close()
    m.close()


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--clients", type=int, default=1024)
    ap.add_argument("--group", type=int, default=8)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--pack-iters", type=int, default=20)
    ap.add_argument("--families", default="cf32,cs16", help="of cf32, cs16, cf32-cs16")
    ap.add_argument("--pack", action="store_true", help="only (a): the two pack launches against a device-to-device copy")
    ap.add_argument("--gain", action="store_true", help="only (e): the pack launch with gains and levels against the narrowing pack launch")
    ap.add_argument("--tune", action="store_true", help="only (f): the call with every client tuned against the same run untuned")
    ap.add_argument("--squelch", default=None, metavar="FRACTIONS",
                    help="only (g): every client squelched with these fractions of the gates open (e.g. 1.0,0.25,0.05) against no squelch, then the meter against the pack launch")
    ap.add_argument("--out", default="/tmp/serve_bench_out")
    ap.add_argument("--report", default=None)
    a = ap.parse_args(argv)
    import resource

    soft, hard = resource.getrlimit(resource.RLIMIT_NOFILE)  # (two descriptors per client's pipe)
    resource.setrlimit(resource.RLIMIT_NOFILE, (hard if hard != resource.RLIM_INFINITY else 1 << 16, hard))
    os.makedirs(a.out, exist_ok=True)
    out = [f"serve_bench: {xl.device_info()}"]
    if a.squelch:
        drain = Drain()
        for family in a.families.split(","):
            run_squelch(a, family, [float(v) for v in a.squelch.split(",")], drain, out)
        drain.close()
        run_meter(a, out)
    elif a.tune:
        drain = Drain()
        run_tune(a, drain, out)
        drain.close()
    elif a.gain:
        run_gain(a, out)
    else:
        run_pack(a, out)
    if not a.pack and not a.gain and not a.tune and not a.squelch:
        drain = Drain()
        for family in a.families.split(","):
            run_periods(a, family, drain, out)
        drain.close()
    text = "\n".join(out)
    print(text)
    if a.report:
        with open(a.report, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
