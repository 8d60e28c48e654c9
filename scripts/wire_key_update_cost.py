#!/usr/bin/env python3
"""What tlsgpu_open_wire's KeyUpdate switch costs: the peek is
one cipher block per record and the switch adds two launches.  TLS 1.3 streams
without any KeyUpdate, the wire shapes of scripts/tls13_cost.py's B and C:

  B  1,024 streams x 64 records x 16 KiB, AES-128-GCM       (TLS 1.3)
  C  4,096 streams x 256 records x 1,400 B, ChaCha20-Poly1305 (TLS 1.3)

The wire is made by tlsgpu_seal_wire (one session per stream).  Every timed
launch opens a fresh copy of the sealed wire, device events around the open
alone; `--warmup` rounds of `--steps` opens, then `--rounds` rounds with the
switch off and on alternating in this one process.  Prints one JSON line per
shape: every round's mean time per open for both, medians, spreads, the ratio.

    python scripts/wire_key_update_cost.py [--shape B|C|BC] [--steps 10] [--warmup 3] [--rounds 5]

--off-only never touches the switch and uses nothing a build without it lacks:
for comparing two builds (TLSGPU_LIBRARY selects the library) with the switch
off.  Under `rocprofv3 --kernel-trace --stats -- python
scripts/wire_key_update_cost.py --rounds 1 --steps 3` the stats list
tg::wire_peek13_kernel and tg::wire_ku_confirm_kernel on their own.
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
          "C": (ta.CHACHA20_POLY1305_TLS13, 4096, 256, 1400, 0x5EED0002)}
TLS13 = 0x0304


def timed_open(engine, launch):
    e0, e1 = ta.Event(engine), ta.Event(engine)
    e0.record()
    launch()
    e1.record()
    engine.sync()
    ms = e0.elapsed_ms(e1)
    e0.close()
    e1.close()
    return ms


def run(engine, shape, steps, warmup, rounds, off_only):
    kind, nstreams, per, reclen, seed = SHAPES[shape]
    stream_bytes = per * reclen
    wire_len = ta.seal_wire_size(kind, stream_bytes, reclen, version=TLS13)
    nrec, app_bytes = nstreams * per, nstreams * stream_bytes
    wire_bytes = nstreams * wire_len + 64
    table = ta.SessionTable(engine, nstreams)
    table.install(0, [ta.SessionParams(kind, fill_bytes(seed ^ KEY_TAG, s, ta.KEY_LEN[kind]),
                                       fill_bytes(seed ^ IV_TAG, s, 12), version=TLS13)
                      for s in range(nstreams)])
    B = lambda n: ta.DeviceBuffer(engine, n)  # noqa: E731
    d_data, d_wire, d_sealed = B(app_bytes), B(wire_bytes), B(wire_bytes)
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
    ta.seal_wire(table, d_wst.ptr, nstreams, d_data.ptr, app_bytes, d_sealed.ptr, wire_bytes, nrec,
                 d_recs.ptr, d_status.ptr, d_wres.ptr, d_total.ptr)
    engine.sync()

    def open_wire():
        ta.open_wire(table, d_rst.ptr, nstreams, d_wire.ptr, nrec, d_recs.ptr, d_status.ptr,
                     d_rres.ptr, d_total.ptr)

    def one_round(on):
        if not off_only:
            ta.sessions_wire_key_update(table, on)
        total = 0.0
        for _ in range(steps):
            d_wire.copy_from(d_sealed)
            total += timed_open(engine, open_wire)
        res = d_rres.download().view(ta.WIRE_RESULT_DTYPE)
        if not ((res["delivered"] == per).all() and (res["alert"] == 0).all()
                and (res["reserved"] == 0).all()):
            raise RuntimeError(f"{shape}: open_wire did not deliver every record (switch {on})")
        return total / steps

    modes = (False,) if off_only else (False, True)
    times = {m: [] for m in modes}
    for r in range(warmup + rounds):
        for m in modes:
            t = one_round(m)
            if r >= warmup:
                times[m].append(t)
    out = {"shape": shape, "streams": nstreams, "records": nrec, "record_bytes": reclen,
           "app_bytes": app_bytes, "steps": steps, "warmup_rounds": warmup, "library": ta.LIBPATH}
    for m in modes:
        k = "on" if m else "off"
        out[f"{k}_ms"] = [round(t, 4) for t in times[m]]
        out[f"{k}_median_ms"] = round(statistics.median(times[m]), 4)
        out[f"{k}_spread_ms"] = [round(min(times[m]), 4), round(max(times[m]), 4)]
    if not off_only:
        out["on_over_off_time"] = round(statistics.median(times[True]) /
                                        statistics.median(times[False]), 4)
    print(json.dumps(out), flush=True)
    for b in (d_data, d_wire, d_sealed, d_recs, d_status, d_total, d_wst, d_wres, d_rst, d_rres):
        b.free()
    table.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="BC")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--off-only", action="store_true",
                    help="switch never touched: for comparing builds")
    a = ap.parse_args()
    ta.load_library()
    engine = ta.Engine(0)
    for shape in a.shape:
        run(engine, shape, a.steps, a.warmup, a.rounds, a.off_only)
    engine.close()


if __name__ == "__main__":
    main()
