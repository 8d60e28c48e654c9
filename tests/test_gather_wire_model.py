"""tlsgpu_gather_wire without a GPU: the rule's model (read_wire_model.py) on
hand-written descriptor and status tables, one per stop code, and the parts of
the ABI that need no device — the two struct layouts and the argument check."""
import ctypes as C

import numpy as np
import pytest

import talos_amd as ta
from read_wire_model import gather_model

TAG = 16


def tables(streams_spec, delivered=None):
    """Hand-written open_wire output for streams of (type, length) records laid
    out like a ChaCha20-Poly1305 TLS 1.2 wire: header(5) || plaintext || tag, the
    plaintext left at the fragment start.  delivered: per stream, where the
    stream's first failure cut it (records from there on have status -1 / -3)."""
    n = sum(len(s) for s in streams_spec)
    streams = np.zeros(len(streams_spec), dtype=ta.WIRE_STREAM_DTYPE)
    results = np.zeros(len(streams_spec), dtype=ta.WIRE_RESULT_DTYPE)
    recs = np.zeros(n, dtype=ta.RECORD_DTYPE)
    status = np.zeros(n, dtype=np.int32)
    pos, slot = 3, 0
    for s, spec in enumerate(streams_spec):
        start, first = pos, slot
        for i, (rtype, length) in enumerate(spec):
            recs[slot] = (pos + 5, pos + 5, 100 * s + i, 0, ta.len_type(length + TAG, rtype))
            status[slot] = length
            pos += 5 + length + TAG
            slot += 1
        cut = len(spec) if delivered is None else delivered[s]
        if cut < len(spec):
            status[first + cut] = ta.REC_BAD_MAC
            status[first + cut + 1:slot] = ta.REC_SKIPPED
        streams[s] = (start, pos - start, 0, 100 * s, 0x0303, 0, 0)
        results[s] = (first, len(spec), cut, pos - start, 20 if cut < len(spec) else 0, cut, (0, 0))
        pos += 2
    wire = (np.arange(pos + 8, dtype=np.uint32) * 7 + 1).astype(np.uint8)
    return streams, results, recs, status, wire


def reads_of(*rows):
    r = np.zeros(len(rows), dtype=ta.READ_STREAM_DTYPE)
    for i, row in enumerate(rows):
        r[i] = row
    return r


def run(t, reads, app_bytes=256, max_records=None, wire_bytes=None):
    streams, results, recs, status, wire = t
    app0 = np.full(app_bytes, 0xA5, dtype=np.uint8)
    app, out = gather_model(streams, results, recs, status,
                            len(recs) if max_records is None else max_records, wire,
                            len(wire) if wire_bytes is None else wire_bytes, reads, app0)
    return app, out, wire, recs


def plain(wire, recs, slot, n):
    o = int(recs[slot]["out_off"])
    return wire[o:o + n]


def fields(r):
    return tuple(int(r[f]) for f in ("app_len", "records", "next", "consumed", "stop", "stop_type",
                                     "stop_len"))


def test_end_concatenates_in_order_and_reads_past_an_empty_record():
    t = tables([[(23, 5), (23, 0), (23, 9)]])
    app, out, wire, recs = run(t, reads_of((7, 100, 0)))
    consumed = (5 + 5 + TAG) + (5 + 0 + TAG) + (5 + 9 + TAG)
    assert fields(out[0]) == (14, 3, 3, consumed, ta.READ_END, 0, 0)
    want = np.full(256, 0xA5, dtype=np.uint8)
    want[7:12], want[12:21] = plain(wire, recs, 0, 5), plain(wire, recs, 2, 9)
    assert np.array_equal(app, want)


def test_not_app_data_stops_before_the_record_and_start_resumes_after_it():
    t = tables([[(23, 4), (21, 2), (23, 6)]])
    app, out, wire, recs = run(t, reads_of((0, 100, 0)))
    assert fields(out[0]) == (4, 1, 1, 5 + 4 + TAG, ta.READ_NOT_APP_DATA, 21, 2)
    assert np.array_equal(app[:4], plain(wire, recs, 0, 4)) and (app[4:] == 0xA5).all()
    app, out, wire, recs = run(t, reads_of((10, 100, 2)))  # start = next + 1
    assert fields(out[0]) == (6, 1, 3, int(t[0][0]["wire_len"]), ta.READ_END, 0, 0)
    assert np.array_equal(app[10:16], plain(wire, recs, 2, 6))
    assert (app[:10] == 0xA5).all() and (app[16:] == 0xA5).all()


def test_full_takes_whole_records_only():
    t = tables([[(23, 8), (23, 8)]])
    _, out, _, _ = run(t, reads_of((0, 16, 0)))
    assert fields(out[0])[:3] == (16, 2, 2) and out[0]["stop"] == ta.READ_END
    app, out, _, _ = run(t, reads_of((0, 15, 0)))
    assert fields(out[0]) == (8, 1, 1, 5 + 8 + TAG, ta.READ_FULL, 23, 8)
    assert (app[8:] == 0xA5).all()
    # the room is also bounded by the application buffer: min(app_cap, app_bytes - app_off)
    _, out, _, _ = run(t, reads_of((250, 100, 0)), app_bytes=256)
    assert fields(out[0])[:3] == (0, 0, 0) and out[0]["stop"] == ta.READ_FULL
    app, out, _, _ = run(t, reads_of((300, 100, 0)), app_bytes=256)
    assert fields(out[0]) == (0, 0, 0, 0, ta.READ_FULL, 23, 8) and (app == 0xA5).all()
    # an empty record always fits
    _, out, _, _ = run(tables([[(23, 0), (23, 0)]]), reads_of((300, 0, 0)), app_bytes=256)
    assert fields(out[0])[:3] == (0, 2, 2) and out[0]["stop"] == ta.READ_END


def test_out_of_bounds():
    t = tables([[(23, 8), (23, 8)], [(23, 3)]])
    app, out, _, _ = run(t, reads_of((0, 100, 3), (50, 100, 0)))     # start > delivered
    assert fields(out[0]) == (0, 0, 3, 0, ta.READ_OUT_OF_BOUNDS, 0, 0)
    assert fields(out[1])[:3] == (3, 1, 1) and (app[:50] == 0xA5).all()
    _, out, _, _ = run(t, reads_of((0, 100, 2), (50, 100, 0)))       # start == delivered: END
    assert fields(out[0])[:3] == (0, 0, 2) and out[0]["stop"] == ta.READ_END
    app, out, _, _ = run(t, reads_of((0, 100, 0), (50, 100, 0)), max_records=2)  # slots leave max_records
    assert out[0]["stop"] == ta.READ_END and fields(out[1]) == (0, 0, 0, 0, ta.READ_OUT_OF_BOUNDS, 0, 0)
    assert (app[50:] == 0xA5).all()
    # the second record's plaintext ends one byte past wire_bytes
    end = int(t[2][1]["out_off"]) + 8
    app, out, _, _ = run(t, reads_of((0, 100, 0), (50, 100, 0)), wire_bytes=end - 1)
    assert fields(out[0]) == (8, 1, 1, 5 + 8 + TAG, ta.READ_OUT_OF_BOUNDS, 0, 0)
    assert (app[8:] == 0xA5).all() and out[1]["stop"] == ta.READ_OUT_OF_BOUNDS


def test_truncated_delivered_hides_the_failing_and_skipped_records():
    t = tables([[(23, 4), (23, 5), (23, 6), (21, 2)]], delivered=[2])
    app, out, wire, recs = run(t, reads_of((1, 100, 0)))
    assert fields(out[0]) == (9, 2, 2, (5 + 4 + TAG) + (5 + 5 + TAG), ta.READ_END, 0, 0)
    assert np.array_equal(app[1:5], plain(wire, recs, 0, 4)) and (app[10:] == 0xA5).all()


def test_struct_layouts():
    assert ta.READ_STREAM_DTYPE.itemsize == 16 and ta.READ_RESULT_DTYPE.itemsize == 32
    assert [ta.READ_STREAM_DTYPE.fields[f][1] for f in ("app_off", "app_cap", "start")] == [0, 8, 12]
    assert [ta.READ_RESULT_DTYPE.fields[f][1] for f in
            ("app_len", "records", "next", "consumed", "stop", "stop_type", "stop_len",
             "reserved")] == list(range(0, 32, 4))
    assert (ta.READ_END, ta.READ_NOT_APP_DATA, ta.READ_FULL, ta.READ_OUT_OF_BOUNDS) == (0, 1, 2, 3)
    # the header says the same
    src = open(ta.INCLUDE + "/tlsgpu.h").read()
    for name, value in (("END", 0), ("NOT_APP_DATA", 1), ("FULL", 2), ("OUT_OF_BOUNDS", 3)):
        assert f"#define TLSGPU_READ_{name} {value}" in src


def test_null_table_is_einval_without_a_device():
    lib = ta.load_library()
    buf = (C.c_uint8 * 64)()
    p = C.addressof(buf)
    assert lib.tlsgpu_gather_wire(None, p, p, 1, p, p, 1, p, 16, p, p + 32, 16, p, None) == -1
    assert lib.tlsgpu_gather_wire(None, None, None, 0, None, None, 0, None, 0, None, None, 0, None,
                                  None) == -1
    assert b"bad arguments" in lib.tlsgpu_last_error()
