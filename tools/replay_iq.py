#!/usr/bin/env python3
"""tools/replay_iq.py -- end-to-end run of the batched path without the TCP server: replay a raw IQ file through
wire-format admission (include/xlating_wire.h), the batch engine (include/xlating_batch.h) and the output sinks
(include/xlating_sinks.h).  What the reference does with a dongle + N connected clients, with the file standing in for
the device (its device plugins deliver blocks of `buffer_size` bytes: cu8 rtl-sdr, cs8 hackrf, cs16 airspy;
src/sdr/*_device.c, src/tcp_server.c:257-271).

  python tools/replay_iq.py capture.cu8 --format cu8 --band-rate 2016000 --band-freq 460100000 --out /tmp/out \\
         --client 460112000:48000 --client 460050000:96000 [--gzip] [--variant optimized | native | q15 [--q15-kernel 1] [--q15-nco 1]]

Every --client CENTER_HZ:RATE_HZ goes through the 15-byte wire request, the admission rules and
xlating_wire_add_client, and ends up as <out>/<id>.cf32[.gz].  With --waterfall-width W every admitted client also gets a stream of a
spectrum bank (include/xlating_spectrum.h) at its own rate, fed from the engine's device rows after every block, and <out>/<id>.png:
the 8-bit gray waterfall sdr_spectrogram makes from that client's .cf32 (-w W -s RATE -d cf32; W above 8192: the bank's wide form, and
sdr_spectrogram -W).  A client slower than W gets no waterfall.
With --any-rate a client whose RATE_HZ does not divide the band rate is admitted too (xlating_wire_admit_any_rate): the engine takes it
to band_rate / D, one resampler bank (include/xlating_resample.h) from there to RATE_HZ by L / M, and its .cf32 and waterfall are at
RATE_HZ like everybody's.
With --variant q15 the engine runs the reference's cs16 output family (XL_MODE_Q15: exact Q15 arithmetic, int16 pairs), the second
stage of --any-rate is the Q15 resampler bank (include/xlating_resample_q15.h), the waterfall is that of cs16 samples, and every
client's samples are written by this tool itself as <out>/<id>.cs16 (raw int16 pairs): the sinks library writes the cf32 family's
files, so --gzip, which is its work, is refused together with q15."""
import argparse
import os
import struct
import sys
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import sdr_server_amd as xl  # noqa: E402

DTYPES = {"cu8": np.uint8, "cs8": np.int8, "cs16": np.int16}


def write_gray_png(path, pixels):
    """pixels: uint8 [H, W] -> an 8-bit grayscale PNG (filter type 0 on every line)"""
    h, w = pixels.shape

    def chunk(typ, body):
        return struct.pack(">I", len(body)) + typ + body + struct.pack(">I", zlib.crc32(typ + body) & 0xFFFFFFFF)

    lines = np.concatenate([np.zeros((h, 1), np.uint8), np.ascontiguousarray(pixels, dtype=np.uint8)], axis=1)
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 0, 0, 0, 0)) +
                chunk(b"IDAT", zlib.compress(lines.tobytes())) + chunk(b"IEND", b""))


def replay(path, fmt, band_rate, band_freq, clients, out_dir, buffer_size=262144, lpf_cutoff_rate=5, variant="optimized",
           gzip=False, writer_threads=2, waterfall_width=None, any_rate=False, q15_kernel=0, q15_nco=0):
    """clients: [(center_hz, rate_hz)].  Returns {client_id: (center_hz, rate_hz)} of the admitted ones, the list of
    (center, rate, failure_details) of the rejected ones and the run's counters.  waterfall_width: also write <out>/<id>.png per
    admitted client whose output holds at least one row (rate samples).  any_rate: admit rates that do not divide the band rate through
    a resampler bank behind the engine.  variant "q15": the cs16 family throughout, <out>/<id>.cs16 written here, no gzip; q15_kernel:
    the engine option of that name (1: the eligible clients' FIR on the matrix cores, the same bits); q15_nco: likewise (1: the Q15 phase
    table tabulated a call ahead on the side stream, the same bits)."""
    q15 = variant == "q15"
    if q15 and gzip:
        raise ValueError("gzip is the sinks library's, which writes the cf32 family: not with variant q15")
    os.makedirs(out_dir, exist_ok=True)
    # (a width above 8192 is the bank's wide form: xlating_spectrum_bank_create_wide)
    bank = xl.SpectrumBank(waterfall_width, "cs16" if q15 else "cf32", wide=waterfall_width > 8192) if waterfall_width else None
    streams, rows, samples = {}, {}, {}  # client id -> bank stream, its rows so far, its output samples so far
    eng = xl.BatchEngine(band_rate, fmt, buffer_size)
    if q15:
        eng.set_option("q15_kernel", q15_kernel)
        if q15_nco:
            eng.set_option("q15_nco", q15_nco)
    sinks = None if q15 else xl.Sinks(writer_threads=writer_threads, queue_bytes=64 * (buffer_size // 2 // 8 + 64) * 8)
    files, written = {}, 0  # q15: client id -> its open <id>.cs16, the bytes written to them
    admitted, rejected = {}, []
    rbank, rsinks, rstreams = None, None, {}  # the second stage: client id -> resampler stream; those clients' sinks are written, not submitted
    for center, rate in clients:
        code, req = xl.wire_parse_request(xl.wire_build_request(center, rate, band_freq, 0)[2:])
        assert code == 0
        rs = None
        if any_rate:
            code, adm, rs, why = xl.wire_admit_any_rate(req, band_rate, band_freq if admitted else 0, lpf_cutoff_rate)
        else:
            code, adm, why = xl.wire_admit(req, band_rate, band_freq if admitted else 0, lpf_cutoff_rate)
        if code != 0:
            rejected.append((center, rate, why))
            continue
        rtaps = None
        if rs is not None and (rs.L, rs.M) != (1, 1):
            code, rtaps = xl.wire_resample_taps(req, rs, lpf_cutoff_rate)
            if code != 0:
                rejected.append((center, rate, 3))  # INTERNAL_ERROR
                continue
        cid = xl.wire_add_client(eng, adm, band_rate)
        if cid < 0:
            rejected.append((center, rate, 3))  # INTERNAL_ERROR
            continue
        if rtaps is not None:
            if rbank is None and q15:
                rbank = xl.ResamplerBankQ15()
            elif rbank is None:
                rbank = xl.ResamplerBank()
                rsinks = xl.Sinks(writer_threads=writer_threads, queue_bytes=64 * (buffer_size // 2 // 8 + 64) * 8)
            rstreams[cid] = rbank.add(rs.L, rs.M, rtaps)
            if not q15:
                assert rsinks.attach_file(cid, out_dir, use_gzip=gzip) == 0
        elif not q15:
            assert sinks.attach_file(cid, out_dir, use_gzip=gzip) == 0
        if q15:
            files[cid] = open(os.path.join(out_dir, f"{cid}.cs16"), "wb")
        admitted[cid] = (center, rate)
        if bank is not None and rate >= waterfall_width:
            streams[cid], rows[cid], samples[cid] = bank.add(rate), [], 0
    elem = np.dtype(DTYPES[fmt]).itemsize
    per_block = buffer_size // elem  # the devices deliver buffer_size BYTES per callback
    data = np.fromfile(path, dtype=DTYPES[fmt])
    nblocks = 0
    for off in range(0, data.size, per_block):
        blk = data[off:off + per_block]
        if blk.size % 2:
            blk = blk[:-1]
        if blk.size == 0:
            break
        eng.process_host(blk, variant)
        eng.fetch()
        if q15:
            for cid, f in files.items():
                if cid not in rstreams:
                    written += f.write(eng.output_cs16(cid).tobytes())
        else:
            sinks.submit(eng)
        if rstreams:  # (fetch has waited for the block; the device rows hold until the next process call)
            rbank.feed_engine(eng, rstreams)
            rbank.fetch()
            for cid, rid in rstreams.items():
                if q15:
                    written += files[cid].write(rbank.output(rid).tobytes())
                else:
                    rsinks.write(cid, rbank.output(rid))
        if streams:
            direct = {cid: sid for cid, sid in streams.items() if cid not in rstreams}
            if direct:
                bank.feed_engine(eng, direct)
            second = [(streams[cid], *rbank.output_device(rid)) for cid, rid in rstreams.items() if cid in streams]
            if second:  # (the resampler's device rows hold until its next feed)
                bank.feed([sid for sid, _, _ in second], [p or 0 for _, p, _ in second], [n for _, _, n in second])
            for cid, sid in streams.items():
                samples[cid] += rbank.output_device(rstreams[cid])[1] if cid in rstreams else eng.output_len(cid)
                if bank.rows_pending(sid):
                    rows[cid].append(bank.take_rows(sid)[1])
        for cid in [] if q15 else sinks.failed() + (rsinks.failed() if rsinks is not None else []):
            (rsinks if cid in rstreams else sinks).detach(cid)
            eng.remove_client(cid)
            admitted.pop(cid, None)
            if cid in streams:
                bank.remove(streams.pop(cid))
            if cid in rstreams:
                rbank.remove(rstreams.pop(cid))
        nblocks += 1
    if sinks is not None:
        sinks.flush()
    if rsinks is not None:
        rsinks.flush()
    for cid, sid in streams.items():
        rows[cid].append(bank.take_rows(sid)[1])
        px = np.concatenate(rows[cid])[:samples[cid] // admitted[cid][1]]  # (a last row whose skipped tail never came is no row)
        if px.shape[0] > 0:
            write_gray_png(os.path.join(out_dir, f"{cid}.png"), px)
    if bank is not None:
        bank.close()
    for f in files.values():
        f.close()
    dropped = 0
    if sinks is not None:
        for cid in list(admitted):
            (rsinks if cid in rstreams else sinks).detach(cid)
        written, dropped = sinks.stats()
        sinks.close()
    if rsinks is not None:
        written, dropped = (a + b for a, b in zip((written, dropped), rsinks.stats()))
        rsinks.close()
    if rbank is not None:
        rbank.close()
    eng.close()
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
                    help="q15: the cs16 output family; every client's samples are written as <id>.cs16 (raw int16 pairs)")
    ap.add_argument("--q15-kernel", type=int, default=0, choices=[0, 1],
                    help="with --variant q15: engine option q15_kernel (1: the FIR of every eligible client on the matrix cores)")
    ap.add_argument("--q15-nco", type=int, default=0, choices=[0, 1],
                    help="with --variant q15: engine option q15_nco (1: the phase table of the next call tabulated on the side stream)")
    ap.add_argument("--gzip", action="store_true", help="gzip the .cf32 files (the sinks library's work: refused with --variant q15)")
    ap.add_argument("--waterfall-width", type=int, default=None, help="also write <id>.png: each client's waterfall, this many bins wide")
    ap.add_argument("--any-rate", action="store_true",
                    help="admit rates that do not divide the band rate: integer decimation in the engine, then a resampler bank")
    a = ap.parse_args(argv)
    if a.gzip and a.variant == "q15":
        ap.error("--gzip is refused with --variant q15: the .cs16 files are written raw by this tool, not by the sinks library")
    return a


def main(argv=None):
    a = parse_args(argv)
    clients = [tuple(int(v) for v in c.split(":")) for c in a.client]
    adm, rej, st = replay(a.iq_file, a.format, a.band_rate, a.band_freq, clients, a.out, a.buffer_size, a.lpf_cutoff_rate,
                          a.variant, a.gzip, waterfall_width=a.waterfall_width, any_rate=a.any_rate, q15_kernel=a.q15_kernel, q15_nco=a.q15_nco)
    for cid, (c, r) in adm.items():
        print(f"client {cid}: center {c} Hz rate {r} Hz -> {a.out}/{cid}.{'cs16' if a.variant == 'q15' else 'cf32'}{'.gz' if a.gzip else ''}")
    for c, r, why in rej:
        print(f"rejected: center {c} Hz rate {r} Hz (details {why})")
    print(st)


if __name__ == "__main__":
    main()
