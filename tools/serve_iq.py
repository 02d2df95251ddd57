#!/usr/bin/env python3
"""tools/serve_iq.py -- tools/replay_iq.py's run through the serve object (include/xlating_serve.h): the same command line, the same
files, but the loop -- admission, engine, second stage, delivery, sinks -- is the C object's, one call per block:

  python tools/serve_iq.py capture.cu8 --format cu8 --band-rate 2016000 --band-freq 460100000 --out /tmp/out \\
         --client 460112000:48000 --client 460050000:44100 --any-rate [--gzip] [--overlap] [--variant optimized | native | q15] [--cs16-out]

Every --client CENTER_HZ:RATE_HZ is sent to the object as the 15-byte wire message and ends up as <out>/<id>.cf32[.gz], or with
--variant q15 as <out>/<id>.cs16[.gz]: the sinks library writes both families, so --gzip works with q15 here.  --cs16-out with
--variant native | optimized also writes <out>/<id>.cs16[.gz], but from the cf32 family's streams, narrowed on their way to the host
(family "cf32-cs16": round to nearest of y * 32768, saturated); the waterfalls are then still fed with the cf32 rows on the device.  With --waterfall-width W
every admitted client fast enough also gets <out>/<id>.png from a spectrum bank fed with the object's final rows
(xlating_serve_outputs_device) after every block.  With --cs16-out, --gain G delivers every client's stream as y * 2^(15 + G) (G a
power of two's exponent, -48 .. 48) and --auto-gain lets the object choose each client's G from its level (include/xlating_serve.h);
both also write <out>/<id>.gain: lines "first_sample gain_log2" from the client's gain log -- from that sample of the file on, the
int16 values are y * 2^(15 + gain_log2); before the first line the gain is 0 -- and a last line "clipped_total N".  --tune FILE (not with --variant q15) tunes running clients
(xlating_serve_set_tune: a phase-continuous rotation of the client's final row, behind its filters): each line of FILE is
"client_index seconds shift_hz ramp_hz_per_s" (client_index counts the --client options from 0; '#' starts a comment) and is applied
before the first call whose first band sample is at or after `seconds`; every client so tuned also gets <out>/<id>.tune: lines
"first_sample F R" from its tune log -- from that sample of the file on the steps are F and R (turns * 2^64 per sample and per
sample^2), the phase 0 at the first line's sample and continuous from there.  --squelch OPEN_DB[:CLOSE_DB[:HANG]] (every variant) gives
every client a squelch (xlating_serve_set_squelch): the marks in dBFS of the mean power of its final row (0 dBFS: |y| of 1; with
--variant q15 full scale), converted here to powers as 10^(dB / 10); CLOSE_DB defaults to OPEN_DB, HANG (calls) to 0; write it with '=' (--squelch=-20:-40:2), as the
marks begin with a minus sign.  A client's file
then holds only the calls its gate was open in, and <out>/<id>.squelch its gate changes: lines "stream_sample delivered_sample open"
-- from that sample of the stream the client produced the gate is `open`, and the file held delivered_sample samples at that point --
and a last line "withheld_samples N".  No fetch of the engine's or the bank's arena happens anywhere: per block one pack
launch and one copy of exactly the delivered bytes."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402

import replay_iq  # noqa: E402
import sdr_server_amd as xl  # noqa: E402

DTYPES = replay_iq.DTYPES


def replay(path, fmt, band_rate, band_freq, clients, out_dir, buffer_size=262144, lpf_cutoff_rate=5, variant="optimized",
           gzip=False, writer_threads=2, waterfall_width=None, any_rate=False, q15_kernel=0, q15_nco=0, overlap=False, cs16_out=False, gain=None,
           auto_gain=False, tune=None, squelch=None):
    """replay_iq.replay's arguments and its triple: {client_id: (center_hz, rate_hz)} of the admitted requests, [(center, rate,
    failure_details)] of the refused ones, and the counters -- blocks, and the sinks' own bytes_written and blocks_dropped
    (xlating_serve_sink_stats: what replay_iq reads from its Sinks objects)."""
    q15 = variant == "q15"
    os.makedirs(out_dir, exist_ok=True)
    family = "cs16" if q15 else ("cf32-cs16" if cs16_out else "cf32")  # (with q15 the files are cs16 anyway)
    serve = xl.Serve(band_rate, fmt, buffer_size, out_dir, family=family, native=variant == "native", any_rate=any_rate,
                     gzip=gzip, overlap=overlap, lpf_cutoff_rate=lpf_cutoff_rate, writer_threads=writer_threads,
                     queue_bytes=64 * (buffer_size // 2 // 8 + 64) * 8)
    eng = serve.engine()
    if q15:
        eng.set_option("q15_kernel", q15_kernel)
        if q15_nco:
            eng.set_option("q15_nco", q15_nco)
    metered = family == "cf32-cs16" and (gain is not None or auto_gain)
    if (gain is not None or auto_gain) and not metered:
        raise ValueError("--gain and --auto-gain need --cs16-out with --variant native | optimized")
    tune = sorted(tune or [], key=lambda t: t[1])  # [(client index, seconds, shift_hz, ramp_hz_per_s)], stable in time
    if tune and q15:
        raise ValueError("--tune needs --variant native | optimized")
    by_index, tuned = {}, set()
    bank = xl.SpectrumBank(waterfall_width, "cs16" if q15 else "cf32", wide=waterfall_width > 8192) if waterfall_width else None
    streams, rows, samples = {}, {}, {}
    admitted, rejected = {}, []
    for index, (center, rate) in enumerate(clients):
        code, resp, cid = serve.request(xl.wire_build_request(center, rate, band_freq, 0))
        if code != 0:
            rejected.append((center, rate, xl.wire_parse_response(resp)[2]))
            continue
        admitted[cid] = (center, rate)
        by_index[index] = cid
        if metered:
            if gain is not None:
                serve.set_gain(cid, gain)
            if auto_gain:
                serve.set_auto_gain(cid, True)
        if squelch is not None:
            serve.set_squelch(cid, *squelch)
        if bank is not None and rate >= waterfall_width:
            streams[cid], rows[cid], samples[cid] = bank.add(rate), [], 0
    elem = np.dtype(DTYPES[fmt]).itemsize
    per_block = buffer_size // elem
    data = np.fromfile(path, dtype=DTYPES[fmt])
    nblocks = 0
    for off in range(0, data.size, per_block):
        blk = data[off:off + per_block]
        if blk.size % 2:
            blk = blk[:-1]
        if blk.size == 0:
            break
        while tune and tune[0][1] * band_rate <= off // 2:  # (the call's first band sample is at or after the line's time)
            index, _, shift, ramp = tune.pop(0)
            if by_index.get(index) in admitted:
                serve.set_tune(by_index[index], shift, ramp)
                tuned.add(by_index[index])
        serve.blocks_host(blk)
        for cid in serve.dropped():
            admitted.pop(cid, None)
            if cid in streams:
                bank.remove(streams.pop(cid))
        if streams:
            ids = list(streams)
            ptrs, counts = serve.outputs_device(ids)
            if overlap:  # (nothing has waited for the latest rows yet, and the bank reads them on another stream than the object's)
                import torch

                torch.cuda.synchronize()
            bank.feed([streams[c] for c in ids], ptrs, counts)
            for cid, n in zip(ids, counts.tolist()):
                samples[cid] += n
                if bank.rows_pending(streams[cid]):
                    rows[cid].append(bank.take_rows(streams[cid])[1])
        nblocks += 1
    serve.flush()
    written, dropped = serve.sink_stats()
    if metered:  # (tool-level: the sinks write the samples only)
        ids = sorted(admitted)
        totals = serve.levels(ids)["clipped_total"].tolist() if ids else []
        for cid, total in zip(ids, totals):
            with open(os.path.join(out_dir, f"{cid}.gain"), "w") as f:
                for first, g in serve.gain_log(cid):
                    f.write(f"{first} {g}\n")
                f.write(f"clipped_total {total}\n")
    for cid in sorted(tuned & set(admitted)):
        with open(os.path.join(out_dir, f"{cid}.tune"), "w") as f:
            for first, F, R in serve.tune_log(cid):
                f.write(f"{first} {F} {R}\n")
    if squelch is not None:
        ids = sorted(admitted)
        withheld = serve.squelch_state(ids)["withheld_samples"].tolist() if ids else []
        for cid, total in zip(ids, withheld):
            with open(os.path.join(out_dir, f"{cid}.squelch"), "w") as f:
                for stream_sample, delivered_sample, is_open in serve.squelch_log(cid):
                    f.write(f"{stream_sample} {delivered_sample} {is_open}\n")
                f.write(f"withheld_samples {total}\n")
    for cid, sid in streams.items():
        rows[cid].append(bank.take_rows(sid)[1])
        px = np.concatenate(rows[cid])[:samples[cid] // admitted[cid][1]]
        if px.shape[0] > 0:
            replay_iq.write_gray_png(os.path.join(out_dir, f"{cid}.png"), px)
    if bank is not None:
        bank.close()
    serve.close()
    return admitted, rejected, {"blocks": nblocks, "bytes_written": written, "blocks_dropped": dropped}


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("iq_file")
    ap.add_argument("--format", default="cu8", choices=list(DTYPES))
    ap.add_argument("--band-rate", type=int, default=2016000)
    ap.add_argument("--band-freq", type=int, required=True)
    ap.add_argument("--client", action="append", default=[], help="CENTER_HZ:RATE_HZ (repeatable)")
    ap.add_argument("--out", required=True)
    ap.add_argument("--buffer-size", type=int, default=262144)
    ap.add_argument("--lpf-cutoff-rate", type=int, default=5)
    ap.add_argument("--variant", default="optimized", choices=["native", "optimized", "q15"],
                    help="q15: the cs16 output family; every client's samples are written as <id>.cs16[.gz] (int16 pairs)")
    ap.add_argument("--q15-kernel", type=int, default=0, choices=[0, 1])
    ap.add_argument("--q15-nco", type=int, default=0, choices=[0, 1])
    ap.add_argument("--gzip", action="store_true", help="gzip the files (either family)")
    ap.add_argument("--waterfall-width", type=int, default=None, help="also write <id>.png: each client's waterfall, this many bins wide")
    ap.add_argument("--any-rate", action="store_true",
                    help="admit rates that do not divide the band rate: integer decimation in the engine, then a resampler bank")
    ap.add_argument("--overlap", action="store_true", help="a block's rows reach the sinks during the next block's call")
    ap.add_argument("--cs16-out", action="store_true",
                    help="with --variant native | optimized: write <id>.cs16[.gz], the cf32 family's streams narrowed by the delivery")
    ap.add_argument("--gain", type=int, default=None, metavar="G",
                    help="with --cs16-out: deliver y * 2^(15 + G), G in -48 .. 48; also writes <id>.gain")
    ap.add_argument("--auto-gain", action="store_true",
                    help="with --cs16-out: the object picks each client's gain from its level; also writes <id>.gain")
    ap.add_argument("--tune", default=None, metavar="FILE",
                    help="lines 'client_index seconds shift_hz ramp_hz_per_s': tune running clients; also writes <id>.tune")
    ap.add_argument("--squelch", default=None, metavar="OPEN_DB[:CLOSE_DB[:HANG]]",
                    help="deliver a client's call only while its gate is open: marks in dBFS of its mean power, hang time in calls; "
                         "also writes <id>.squelch")
    return ap.parse_args(argv)


def parse_squelch(text):
    """"OPEN_DB[:CLOSE_DB[:HANG]]" -> (open_power, close_power, hang_calls): dBFS to mean power on the host"""
    f = text.split(":")
    if not 1 <= len(f) <= 3:
        raise ValueError("--squelch OPEN_DB[:CLOSE_DB[:HANG]]")
    open_db = float(f[0])
    close_db = float(f[1]) if len(f) > 1 and f[1] != "" else open_db
    hang = int(f[2]) if len(f) > 2 else 0
    if close_db > open_db or hang < 0:
        raise ValueError("--squelch: CLOSE_DB may not lie above OPEN_DB, HANG may not be negative")
    return 10.0 ** (open_db / 10.0), 10.0 ** (close_db / 10.0), hang


def read_tune_file(path):
    """-> [(client index, seconds, shift_hz, ramp_hz_per_s)]"""
    out = []
    for line in open(path):
        f = line.split("#")[0].split()
        if f:
            out.append((int(f[0]), float(f[1]), float(f[2]), float(f[3])))
    return out


def main(argv=None):
    a = parse_args(argv)
    clients = [tuple(int(v) for v in c.split(":")) for c in a.client]
    adm, rej, st = replay(a.iq_file, a.format, a.band_rate, a.band_freq, clients, a.out, a.buffer_size, a.lpf_cutoff_rate, a.variant,
                          a.gzip, waterfall_width=a.waterfall_width, any_rate=a.any_rate, q15_kernel=a.q15_kernel, q15_nco=a.q15_nco,
                          overlap=a.overlap, cs16_out=a.cs16_out, gain=a.gain, auto_gain=a.auto_gain,
                          tune=read_tune_file(a.tune) if a.tune else None, squelch=parse_squelch(a.squelch) if a.squelch else None)
    ext = "cs16" if a.variant == "q15" or a.cs16_out else "cf32"
    for cid, (c, r) in adm.items():
        print(f"client {cid}: center {c} Hz rate {r} Hz -> {a.out}/{cid}.{ext}{'.gz' if a.gzip else ''}")
    for c, r, why in rej:
        print(f"rejected: center {c} Hz rate {r} Hz (details {why})")
    print(st)


if __name__ == "__main__":
    main()
