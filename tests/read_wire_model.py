"""The rule of tlsgpu_gather_wire (include/tlsgpu.h), restated over host copies
of what tlsgpu_open_wire returned: ssl3_read_bytes (ssl/s3_pkt.c:840-1130) per
stream — application-data records are handed over in order as one contiguous run
(:938-969), an empty one is read past (:486-488), any other type stops the
stream (:973-) — with whole records only.  Pure data movement: nothing here
decrypts, so every comparison with the device is exact.
"""
import numpy as np

import talos_amd as ta

APP_DATA = 23


def gather_model(streams, results, recs, status, max_records, wire, wire_bytes, reads, app):
    """streams / results / recs / reads: arrays of WIRE_STREAM_DTYPE, WIRE_RESULT_DTYPE,
    RECORD_DTYPE and READ_STREAM_DTYPE; status: int32 per record slot; wire: the
    opened wire buffer (uint8), wire_bytes the size the call is told; app: the
    application buffer before the call (uint8, its length is app_bytes).
    Returns (app after the call, READ_RESULT_DTYPE array)."""
    app = np.array(app, dtype=np.uint8, copy=True)
    app_bytes = len(app)
    out = np.zeros(len(streams), dtype=ta.READ_RESULT_DTYPE)
    for s in range(len(streams)):
        first, delivered = int(results[s]["first"]), int(results[s]["delivered"])
        app_off, cap, start = (int(reads[s][f]) for f in ("app_off", "app_cap", "start"))
        r = out[s]
        r["next"] = start
        if start > delivered or first + delivered > max_records:
            r["stop"] = ta.READ_OUT_OF_BOUNDS
            continue
        room = 0 if app_off > app_bytes else min(cap, app_bytes - app_off)
        total, i, stop = 0, start, ta.READ_END
        while i < delivered:
            d, n = recs[first + i], int(status[first + i])
            off, rtype = int(d["out_off"]), int(d["len_type"]) >> 24
            if n < 0 or off > wire_bytes or n > wire_bytes - off:
                stop = ta.READ_OUT_OF_BOUNDS
                break
            if rtype != APP_DATA:
                stop, r["stop_type"], r["stop_len"] = ta.READ_NOT_APP_DATA, rtype, n
                break
            if total + n > room:
                stop, r["stop_type"], r["stop_len"] = ta.READ_FULL, rtype, n
                break
            app[app_off + total:app_off + total + n] = wire[off:off + n]
            total += n
            i += 1
        r["app_len"], r["records"], r["next"], r["stop"] = total, i - start, i, stop
        if i:  # the end of record i - 1's fragment, from the stream's first byte
            last = recs[first + i - 1]
            r["consumed"] = (int(last["in_off"]) + (int(last["len_type"]) & 0xFFFFFF)
                             - int(streams[s]["wire_off"])) & 0xFFFFFFFF
    return app, out
