#!/usr/bin/env python3
"""What tlsgpu_gather_wire (plan + copy) costs next to a plain device copy of
the same application bytes, on the same build, box and process:

  B  1,024 streams x 64 records x 16 KiB, AES-128-GCM       (config B's bytes as wire)
  C  4,096 streams x 256 records x 1,400 B, ChaCha20-Poly1305 (config C's)

The wire is made by tlsgpu_seal_wire (one session per stream) and opened once
by tlsgpu_open_wire.  Then, timed between events on the engine stream after a
warm-up of both: `--steps` gathers of every stream into one packed region, and
`--steps` tlsgpu_memcpy device-to-device copies of as many bytes — alternating,
`--rounds` times in this one process.  Prints one JSON line per shape with
every round's times, the medians, the spread and the ratio.

    python scripts/gather_wire_cost.py [--shape B|C|BC] [--steps 20] [--warmup 5] [--rounds 5]

--open: times tlsgpu_open_wire instead (the existing path; each launch opens a
fresh copy of the sealed wire, events around the open alone), for a before /
after comparison of two builds; it uses nothing the parent build lacks.

TLSGPU_GATHER_PIECE=2048|16384 selects the copy kernel's measured alternatives
(DESIGN.md §4.6b).  Under `rocprofv3 --kernel-trace --stats -- python
scripts/gather_wire_cost.py --rounds 1 --steps 3` the stats list
tg::wire_gather_copy_kernel and tg::wire_gather_plan_kernel on their own.
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
GIB = float(1 << 30)


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


def run(engine, shape, steps, warmup, rounds, open_only):
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
    d_data, d_wire, d_app = B(app_bytes), B(wire_bytes), B(app_bytes)
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
    d_wst, d_wres, d_rst, d_rres = B(wst.nbytes), B(32 * nstreams), B(rst.nbytes), B(32 * nstreams)
    d_wst.upload(wst.view(np.uint8))
    d_rst.upload(rst.view(np.uint8))
    ta.seal_wire(table, d_wst.ptr, nstreams, d_data.ptr, app_bytes, d_wire.ptr, wire_bytes, nrec,
                 d_recs.ptr, d_status.ptr, d_wres.ptr, d_total.ptr)
    engine.sync()

    def open_wire():
        ta.open_wire(table, d_rst.ptr, nstreams, d_wire.ptr, nrec, d_recs.ptr, d_status.ptr,
                     d_rres.ptr, d_total.ptr)

    def check_open():
        res = d_rres.download().view(ta.WIRE_RESULT_DTYPE)
        if not ((res["delivered"] == per).all() and (res["alert"] == 0).all()):
            raise RuntimeError(f"{shape}: open_wire did not deliver every record")

    base = {"shape": shape, "streams": nstreams, "records": nrec, "record_bytes": reclen,
            "app_bytes": app_bytes, "wire_bytes": wire_bytes - 64, "steps": steps, "warmup": warmup}
    if open_only:
        d_sealed = B(wire_bytes)
        d_sealed.copy_from(d_wire)
        times = []
        for r in range(warmup + rounds):
            total = 0.0
            for _ in range(steps):
                d_wire.copy_from(d_sealed)
                total += timed(engine, 1, open_wire)
            check_open()
            if r >= warmup:
                times.append(total / steps)
        print(json.dumps({**base, "op": "open_wire", "library": ta.LIBPATH,
                          "ms_per_launch": [round(t, 4) for t in times],
                          "median_ms": round(statistics.median(times), 4),
                          "spread_ms": [round(min(times), 4), round(max(times), 4)]}), flush=True)
        d_sealed.free()
    else:
        open_wire()
        engine.sync()
        check_open()
        reads = np.zeros(nstreams, dtype=ta.READ_STREAM_DTYPE)
        reads["app_off"] = np.arange(nstreams, dtype=np.uint64) * np.uint64(stream_bytes)
        reads["app_cap"] = stream_bytes
        d_reads, d_out = B(reads.nbytes), B(32 * nstreams)
        d_reads.upload(reads.view(np.uint8))
        d_copy = B(app_bytes)

        def gather():
            ta.gather_wire(table, d_rst.ptr, d_rres.ptr, nstreams, d_recs.ptr, d_status.ptr, nrec,
                           d_wire.ptr, wire_bytes, d_reads.ptr, d_app.ptr, app_bytes, d_out.ptr)

        def copy():
            d_copy.copy_from(d_data, app_bytes)
        for _ in range(warmup):
            gather()
            copy()
        engine.sync()
        out = d_out.download().view(ta.READ_RESULT_DTYPE)
        if not ((out["stop"] == ta.READ_END).all() and (out["app_len"] == stream_bytes).all()
                and (out["records"] == per).all()):
            raise RuntimeError(f"{shape}: gather results")
        for s in (0, nstreams // 2, nstreams - 1):      # the gathered stream is the sealed data
            if not np.array_equal(d_app.download(stream_bytes, s * stream_bytes),
                                  d_data.download(stream_bytes, s * stream_bytes)):
                raise RuntimeError(f"{shape}: stream {s} gathered wrong bytes")
        g, c = [], []
        for _ in range(rounds):
            g.append(timed(engine, steps, gather))
            c.append(timed(engine, steps, copy))
        mg, mc = statistics.median(g), statistics.median(c)
        print(json.dumps({**base, "op": "gather_wire",
                          "piece": int(os.environ.get("TLSGPU_GATHER_PIECE") or 0) or "default",
                          "gather_ms": [round(t, 4) for t in g], "copy_ms": [round(t, 4) for t in c],
                          "gather_median_ms": round(mg, 4), "copy_median_ms": round(mc, 4),
                          "gather_spread_ms": [round(min(g), 4), round(max(g), 4)],
                          "copy_spread_ms": [round(min(c), 4), round(max(c), 4)],
                          "gather_GiBps": round(app_bytes / (mg / 1e3) / GIB, 1),
                          "copy_GiBps": round(app_bytes / (mc / 1e3) / GIB, 1),
                          "gather_over_copy_time": round(mg / mc, 4)}), flush=True)
        for b in (d_reads, d_out, d_copy):
            b.free()
    for b in (d_data, d_wire, d_app, d_recs, d_status, d_total, d_wst, d_wres, d_rst, d_rres):
        b.free()
    table.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="BC")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--open", action="store_true", help="time tlsgpu_open_wire instead")
    a = ap.parse_args()
    ta.load_library()
    engine = ta.Engine(0)
    for shape in a.shape:
        run(engine, shape, a.steps, a.warmup, a.rounds, a.open)
    engine.close()


if __name__ == "__main__":
    main()
