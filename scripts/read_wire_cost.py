#!/usr/bin/env python3
"""What tlsgpu_read_wire costs next to the two-call read path it replaces for
TLS 1.2 tables, on the same build, box and process:

  B  1,024 streams x 64 records x 16 KiB, AES-128-GCM       (config B's bytes as wire)
  C  4,096 streams x 256 records x 1,400 B, ChaCha20-Poly1305 (config C's)

The wire is made by tlsgpu_seal_wire (one session per stream).  Timed between
events on the engine stream, `--steps` launches each after a warm-up of both
sides, alternating, `--rounds` times in this one process:

  (a) tlsgpu_read_wire: every stream opened straight into its packed run; d_wire
      is never written, so nothing is restored between launches;
  (b) the pair: a restore copy of the sealed wire (the open is in place), then
      tlsgpu_open_wire, then tlsgpu_gather_wire into the same packed runs;
  (c) the restore copy alone, so (b) can be read with or without it.

Prints one JSON line per shape with every round's times, the medians and the
min-max spreads.

    python scripts/read_wire_cost.py [--shape B|C|BC] [--steps 20] [--warmup 5] [--rounds 5]

Under `rocprofv3 --kernel-trace --stats -- python scripts/read_wire_cost.py
--rounds 1 --steps 3` the stats list tg::wire_read_plan_kernel,
tg::wire_read_finish_kernel and the cipher kernels of both sides on their own.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import talos_amd as ta  # noqa: E402
from talos_amd.workload import KEY_TAG, IV_TAG, fill_bytes  # noqa: E402

SHAPES = {"B": (ta.AES_128_GCM, 1024, 64, 16384, 0x5EED0001),
          "C": (ta.CHACHA20_POLY1305, 4096, 256, 1400, 0x5EED0002)}


def timed(engine, steps, launch):
    e0, e1 = ta.Event(engine), ta.Event(engine)
    e0.record()
    for _ in range(steps):
        launch()
    e1.record()
    engine.sync()
    ms = e0.elapsed_ms(e1) / steps
    e0.close()
    e1.close()
    return ms


def run(engine, shape, steps, warmup, rounds):
    kind, nstreams, per, reclen, seed = SHAPES[shape]
    stream_bytes = per * reclen
    wire_len = ta.seal_wire_size(kind, stream_bytes, reclen)
    nrec, app_bytes = nstreams * per, nstreams * stream_bytes
    wire_bytes = nstreams * wire_len + 64
    table = ta.SessionTable(engine, nstreams)
    table.install(0, [ta.SessionParams(kind, fill_bytes(seed ^ KEY_TAG, s, ta.KEY_LEN[kind]),
                                       fill_bytes(seed ^ IV_TAG, s, ta.FIXED_IV_LEN[kind]))
                      for s in range(nstreams)])
    B = lambda n: ta.DeviceBuffer(engine, n)  # noqa: E731
    d_data, d_wire, d_sealed, d_app = B(app_bytes), B(wire_bytes), B(wire_bytes), B(app_bytes)
    d_recs, d_status, d_total = B(32 * nrec), B(4 * nrec), B(4)
    engine.fill_synthetic(d_data.ptr, stream_bytes, stream_bytes, nstreams, seed)
    wst = np.zeros(nstreams, dtype=ta.WRITE_STREAM_DTYPE)
    wst["data_off"] = np.arange(nstreams, dtype=np.uint64) * np.uint64(stream_bytes)
    wst["wire_off"] = np.arange(nstreams, dtype=np.uint64) * np.uint64(wire_len)
    wst["seq"], wst["data_len"], wst["session"] = 1 << 20, stream_bytes, np.arange(nstreams)
    wst["version"], wst["type"], wst["max_fragment"] = 0x0303, 23, reclen
    rst = np.zeros(nstreams, dtype=ta.WIRE_STREAM_DTYPE)
    rst["wire_off"], rst["wire_len"], rst["session"] = wst["wire_off"], wire_len, wst["session"]
    rst["seq"], rst["version"] = 1 << 20, 0x0303
    reads = np.zeros(nstreams, dtype=ta.READ_STREAM_DTYPE)
    reads["app_off"] = np.arange(nstreams, dtype=np.uint64) * np.uint64(stream_bytes)
    reads["app_cap"] = stream_bytes
    d_wst, d_wres, d_rst, d_rres, d_reads, d_out = (
        B(wst.nbytes), B(32 * nstreams), B(rst.nbytes), B(32 * nstreams), B(reads.nbytes),
        B(32 * nstreams))
    d_wst.upload(wst.view(np.uint8))
    d_rst.upload(rst.view(np.uint8))
    d_reads.upload(reads.view(np.uint8))
    ta.seal_wire(table, d_wst.ptr, nstreams, d_data.ptr, app_bytes, d_wire.ptr, wire_bytes, nrec,
                 d_recs.ptr, d_status.ptr, d_wres.ptr, d_total.ptr)
    engine.sync()
    d_sealed.copy_from(d_wire)

    def read():
        ta.read_wire(table, d_rst.ptr, nstreams, d_sealed.ptr, wire_bytes, nrec, d_recs.ptr,
                     d_status.ptr, d_rres.ptr, d_total.ptr, d_reads.ptr, d_app.ptr, app_bytes,
                     d_out.ptr)

    def restore():
        d_wire.copy_from(d_sealed)

    def pair():
        restore()
        ta.open_wire(table, d_rst.ptr, nstreams, d_wire.ptr, nrec, d_recs.ptr, d_status.ptr,
                     d_rres.ptr, d_total.ptr)
        ta.gather_wire(table, d_rst.ptr, d_rres.ptr, nstreams, d_recs.ptr, d_status.ptr, nrec,
                       d_wire.ptr, wire_bytes, d_reads.ptr, d_app.ptr, app_bytes, d_out.ptr)

    def check(what):
        res = d_rres.download().view(ta.WIRE_RESULT_DTYPE)
        out = d_out.download().view(ta.READ_RESULT_DTYPE)
        if not ((res["delivered"] == per).all() and (res["alert"] == 0).all()
                and (out["stop"] == ta.READ_END).all() and (out["app_len"] == stream_bytes).all()
                and (out["records"] == per).all()):
            raise RuntimeError(f"{shape}: {what}: results")
        for s in (0, nstreams // 2, nstreams - 1):      # the stream's run is the sealed data
            if not np.array_equal(d_app.download(stream_bytes, s * stream_bytes),
                                  d_data.download(stream_bytes, s * stream_bytes)):
                raise RuntimeError(f"{shape}: {what}: stream {s} holds wrong bytes")

    for side, what in ((pair, "open_wire + gather_wire"), (read, "read_wire")):
        d_app.fill(0)
        for _ in range(warmup):
            side()
        engine.sync()
        check(what)
    a, b, c = [], [], []
    for _ in range(rounds):
        a.append(timed(engine, steps, read))
        b.append(timed(engine, steps, pair))
        c.append(timed(engine, steps, restore))
    check("after the rounds")
    ma, mb, mc = (statistics.median(x) for x in (a, b, c))
    r4 = lambda xs: [round(x, 4) for x in xs]  # noqa: E731
    print(json.dumps({"shape": shape, "streams": nstreams, "records": nrec, "record_bytes": reclen,
                      "app_bytes": app_bytes, "wire_bytes": wire_bytes - 64, "steps": steps,
                      "warmup": warmup, "library": ta.LIBPATH,
                      "read_wire_ms": r4(a), "pair_with_restore_ms": r4(b), "restore_ms": r4(c),
                      "read_wire_median_ms": round(ma, 4),
                      "pair_with_restore_median_ms": round(mb, 4),
                      "restore_median_ms": round(mc, 4),
                      "pair_median_ms": round(mb - mc, 4),
                      "read_wire_spread_ms": r4([min(a), max(a)]),
                      "pair_with_restore_spread_ms": r4([min(b), max(b)]),
                      "restore_spread_ms": r4([min(c), max(c)]),
                      "read_wire_over_pair_time": round(ma / (mb - mc), 4)}), flush=True)
    for buf in (d_data, d_wire, d_sealed, d_app, d_recs, d_status, d_total, d_wst, d_wres, d_rst,
                d_rres, d_reads, d_out):
        buf.free()
    table.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="BC")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    ta.load_library()
    engine = ta.Engine(0)
    for shape in a.shape:
        run(engine, shape, a.steps, a.warmup, a.rounds)
    engine.close()


if __name__ == "__main__":
    main()
