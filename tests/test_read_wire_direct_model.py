"""The model of tlsgpu_read_wire (read_wire_direct_model.py) on hand-written
tables, without a GPU: every expectation below is written out by hand from the
rule in include/tlsgpu.h, none comes from the model.  The last tests show that
the checker test_gpu_read_wire.py relies on can fail.
"""
import numpy as np
import pytest

import talos_amd as ta
from read_wire_direct_model import (BAD_MAC, OK, compare_read, overhead, read_model, slots_in_order,
                                    wanted_records)
from test_wire import header

TLS12 = 0x0303
FILL = 0xA5
GCM, CC = overhead(ta.AES_128_GCM), overhead(ta.CHACHA20_POLY1305)   # (8, 16), (0, 16)


def content(s, k, n):
    return bytes((37 * s + 11 * k + 3 * j + 1) & 0xFF for j in range(n))


class Case:
    """streams: per stream dict(over=, recs=[(type, n[, BAD_MAC])] or ("raw", type, fragment
    length), tail=bytes, version=...); a record's fragment is explicit nonce + n + tag
    bytes of filler: nothing decrypts."""

    def __init__(self, streams, reads, app_bytes, max_records=None, wire_bytes=None, gap=3):
        wire, self.verdicts, self.over = bytearray(b"\xEE" * 7), {}, []
        self.streams = np.zeros(len(streams), dtype=ta.WIRE_STREAM_DTYPE)
        self.ends = []                       # per stream: end of each record within the stream
        for s, spec in enumerate(streams):
            over = spec.get("over", GCM)
            self.over.append(over)
            eiv, tag = over or (0, 0)
            start, ends = len(wire), []
            for k, rec in enumerate(spec["recs"]):
                if rec[0] == "raw":
                    _, rtype, ln = rec
                    self.verdicts[(s, k)] = (BAD_MAC, None)      # (whatever: such fragments are garbage)
                else:
                    rtype, n = rec[0], rec[1]
                    ln = (spec.get("eiv", eiv)) + n + tag
                    self.verdicts[(s, k)] = ((BAD_MAC, None) if len(rec) > 2 else (OK, content(s, k, n)))
                wire += header(rtype, spec.get("rec_version", {}).get(k, TLS12), ln) + bytes([0xC0 + k % 16]) * ln
                ends.append(len(wire) - start)
            wire += spec.get("tail", b"")
            self.streams[s] = (start, len(wire) - start, spec.get("session", 0), 100 * s, TLS12, 0, 0)
            self.ends.append(ends)
            wire += b"\xEE" * gap
        self.wire = np.frombuffer(bytes(wire) + bytes(64), dtype=np.uint8)
        self.wire_bytes = len(wire) if wire_bytes is None else wire_bytes
        self.reads = np.zeros(len(streams), dtype=ta.READ_STREAM_DTYPE)
        for s, row in enumerate(reads):
            self.reads[s] = row
        self.app_bytes = app_bytes
        self.app = np.full(app_bytes + 64, FILL, dtype=np.uint8)
        wanted = wanted_records(self.wire, self.streams)
        self.max_records = sum(wanted) if max_records is None else max_records
        self.slots = slots_in_order(wanted, self.max_records)
        self.exp = read_model(self.streams, self.reads, self.wire, self.wire_bytes, self.over,
                              self.verdicts, self.slots, self.max_records, self.app, app_bytes)

    def read(self, s):
        return tuple(int(self.exp.reads[s][f]) for f in
                     ("app_len", "records", "next", "consumed", "stop", "stop_type", "stop_len"))

    def wres(self, s):
        return tuple(int(self.exp.results[s][f]) for f in
                     ("records", "delivered", "consumed", "alert", "alert_record"))

    def got(self):
        e = self.exp
        return dict(recs=e.recs.copy(), status=e.status.copy(), results=e.results.copy(),
                    reads=e.reads.copy(), app=e.app.copy(), total=e.total)


def test_struct_sizes_are_unchanged():
    assert ta.WIRE_STREAM_DTYPE.itemsize == 32 and ta.WIRE_RESULT_DTYPE.itemsize == 32
    assert ta.READ_STREAM_DTYPE.itemsize == 16 and ta.READ_RESULT_DTYPE.itemsize == 32
    assert ta.RECORD_DTYPE.itemsize == 32
    assert (ta.READ_END, ta.READ_NOT_APP_DATA, ta.READ_FULL, ta.READ_OUT_OF_BOUNDS) == (0, 1, 2, 3)
    assert [ta.READ_RESULT_DTYPE.fields[f][1] for f in
            ("app_len", "records", "next", "consumed", "stop", "stop_type", "stop_len")] == \
        [0, 4, 8, 12, 16, 20, 24]


def test_everything_placed_ends_with_end():
    c = Case([dict(recs=[(23, 10), (23, 0), (23, 33)]), dict(over=CC, recs=[(23, 5)])],
             [(4, 100, 0), (47, 5, 0)], app_bytes=60)
    assert c.read(0) == (43, 3, 3, c.ends[0][2], ta.READ_END, 0, 0)
    assert c.read(1) == (5, 1, 1, c.ends[1][0], ta.READ_END, 0, 0)
    assert c.wres(0) == (3, 3, c.ends[0][2], 0, 3)
    # the empty record is placed where the next one goes, and adds nothing
    assert [int(c.exp.recs[i]["out_off"]) for i in range(4)] == [4, 14, 14, 47]
    assert int(c.exp.recs[1]["in_off"]) == int(c.streams[0]["wire_off"]) + c.ends[0][0] + 5
    assert list(c.exp.status) == [10, 0, 33, 5]
    want = np.full(124, FILL, dtype=np.uint8)
    want[4:47] = np.frombuffer(content(0, 0, 10) + content(0, 2, 33), dtype=np.uint8)
    want[47:52] = np.frombuffer(content(1, 0, 5), dtype=np.uint8)
    assert np.array_equal(c.exp.app, want) and not c.exp.mask.any() and c.exp.total == 4


def test_a_record_that_is_not_application_data_cuts_the_stream():
    # an alert in mid-stream with a bad header version behind it, and a handshake record first
    c = Case([dict(recs=[(23, 10), (21, 2), (23, 7), (23, 1)], rec_version={3: 0x0301}),
              dict(over=CC, recs=[(22, 40), (23, 9)])],
             [(0, 100, 0), (50, 100, 0)], app_bytes=200)
    assert c.read(0) == (10, 1, 1, c.ends[0][0], ta.READ_NOT_APP_DATA, 21, 2)
    # framing stopped at the wrong version with alert 70 after 3 records: dropped with the cut
    assert c.wres(0) == (1, 1, c.ends[0][0], 0, 1)
    assert c.read(1) == (0, 0, 0, 0, ta.READ_NOT_APP_DATA, 22, 40)
    assert c.wres(1) == (0, 0, 0, 0, 0)
    assert c.exp.total == 3 + 2
    # slots behind a cut hold all-ones descriptors; `first` stays framing's
    ones = np.frombuffer(b"\xFF" * 32, dtype=ta.RECORD_DTYPE)[0]
    assert [c.exp.recs[i] == ones for i in range(5)] == [False, True, True, True, True]
    assert list(c.exp.status) == [10] + [ta.REC_PUBLIC_INVALID] * 4
    assert int(c.exp.results[1]["first"]) == 3
    assert (c.exp.app[10:] == FILL).all()


def test_a_header_alert_without_a_cut_is_reported():
    c = Case([dict(recs=[(23, 10), (23, 7), (23, 1)], rec_version={2: 0x0301})], [(0, 100, 0)],
             app_bytes=100)
    assert c.wres(0) == (2, 2, c.ends[0][1], 70, 2)
    assert c.read(0) == (17, 2, 2, c.ends[0][1], ta.READ_END, 0, 0)


def test_room_exact_fit_and_one_byte_short():
    recs = [(23, 100), (23, 1), (23, 27)]
    for reads, app_bytes, full in (([(9, 128, 0)], 500, False), ([(9, 127, 0)], 500, True),
                                   ([(9, 500, 0)], 137, False), ([(9, 500, 0)], 136, True)):
        c = Case([dict(over=CC, recs=recs)], reads, app_bytes=app_bytes)
        if full:
            assert c.read(0) == (101, 2, 2, c.ends[0][1], ta.READ_FULL, 23, 27)
            assert c.wres(0) == (2, 2, c.ends[0][1], 0, 2)
            assert (c.exp.app[9 + 101:] == FILL).all()
        else:
            assert c.read(0) == (128, 3, 3, c.ends[0][2], ta.READ_END, 0, 0)
            assert (c.exp.app[9 + 128:] == FILL).all()
    # no room at all, app_off at and beyond app_bytes: an empty record still needs none (past
    # the end it is placed at the buffer's end), the first byte of content does not fit
    for app_off in (500, 501, 1 << 40):
        c = Case([dict(recs=[(23, 0), (23, 1)])], [(app_off, 100, 0)], app_bytes=500)
        assert c.read(0) == (0, 1, 1, c.ends[0][0], ta.READ_FULL, 23, 1)
        assert int(c.exp.recs[0]["out_off"]) == 500 and (c.exp.app == FILL).all()
    c = Case([dict(recs=[(23, 1), (23, 0)])], [(501, 100, 0)], app_bytes=500)
    assert c.read(0) == (0, 0, 0, 0, ta.READ_FULL, 23, 1)


def test_truncated_tags_count():
    c = Case([dict(over=(8, 12), recs=[(23, 20), (23, 20)])], [(0, 40, 0)], app_bytes=64)
    assert c.read(0) == (40, 2, 2, c.ends[0][1], ta.READ_END, 0, 0)
    assert c.ends[0][0] == 5 + 8 + 20 + 12


def test_a_short_fragment_is_placed_and_fails_the_open():
    c = Case([dict(recs=[(23, 6), ("raw", 23, 23), (23, 4)])], [(2, 100, 0)], app_bytes=64)
    assert c.wres(0) == (3, 1, c.ends[0][2], 21, 1)
    assert c.read(0) == (6, 1, 1, c.ends[0][0], ta.READ_END, 0, 0)
    assert list(c.exp.status) == [6, ta.REC_PUBLIC_INVALID, ta.REC_SKIPPED]
    assert [int(c.exp.recs[i]["out_off"]) for i in range(3)] == [2, 8, 8]
    # the skipped record's 4 bytes are the unspecified range, and only they
    assert list(np.flatnonzero(c.exp.mask)) == [8, 9, 10, 11]


def test_a_failure_before_at_and_behind_a_stop():
    # before: the plan's stop is overruled, the alert says why
    c = Case([dict(recs=[(23, 10), (23, 20, BAD_MAC), (23, 30), (21, 2)])], [(0, 100, 0)],
             app_bytes=100)
    assert c.wres(0) == (3, 1, c.ends[0][2], 20, 1)
    assert c.read(0) == (10, 1, 1, c.ends[0][0], ta.READ_END, 0, 0)
    assert list(c.exp.status) == [10, ta.REC_BAD_MAC, ta.REC_SKIPPED, ta.REC_PUBLIC_INVALID]
    assert list(np.flatnonzero(c.exp.mask)) == list(range(10, 60))
    # at, and behind: the stop record and what follows are not opened, so they cannot fail
    for recs in ([(23, 10), (21, 2, BAD_MAC), (23, 5)], [(23, 10), (21, 2), (23, 5, BAD_MAC)]):
        c = Case([dict(recs=recs)], [(0, 100, 0)], app_bytes=100)
        assert c.wres(0) == (1, 1, c.ends[0][0], 0, 1)
        assert c.read(0) == (10, 1, 1, c.ends[0][0], ta.READ_NOT_APP_DATA, 21, 2)
        assert not c.exp.mask.any()
    c = Case([dict(over=CC, recs=[(23, 10), (23, 50, BAD_MAC)])], [(0, 59, 0)], app_bytes=100)
    assert c.read(0) == (10, 1, 1, c.ends[0][0], ta.READ_FULL, 23, 50)


def test_an_over_long_record():
    c = Case([dict(over=CC, recs=[(23, 3), (23, 16385), (23, 1)])], [(1, 20000, 0)], app_bytes=20000)
    assert c.wres(0) == (3, 1, c.ends[0][2], 22, 1)
    assert c.read(0) == (3, 1, 1, c.ends[0][0], ta.READ_END, 0, 0)
    assert list(c.exp.status) == [3, ta.REC_OVERFLOW, ta.REC_SKIPPED]
    assert c.exp.mask.sum() == 16386 and c.exp.placed == [3 + 16385 + 1]


def test_out_of_bounds():
    # start != 0: cut to nothing, whatever the stream holds
    c = Case([dict(recs=[(23, 10)]), dict(recs=[(23, 10)])], [(0, 10, 1), (10, 10, 0)], app_bytes=20)
    assert c.read(0) == (0, 0, 0, 0, ta.READ_OUT_OF_BOUNDS, 0, 0)
    assert c.wres(0) == (0, 0, 0, 0, 0)
    assert c.read(1)[:3] == (10, 1, 1) and (c.exp.app[:10] == FILL).all()
    # a fragment that reaches one byte past wire_bytes
    c = Case([dict(recs=[(23, 10), (23, 12)])], [(0, 100, 0)], app_bytes=100, gap=0)
    end = int(c.streams[0]["wire_off"]) + c.ends[0][1]
    assert c.read(0)[4] == ta.READ_END
    c = Case([dict(recs=[(23, 10), (23, 12)])], [(0, 100, 0)], app_bytes=100, gap=0, wire_bytes=end - 1)
    assert c.read(0) == (10, 1, 1, c.ends[0][0], ta.READ_OUT_OF_BOUNDS, 0, 0)
    assert c.wres(0) == (1, 1, c.ends[0][0], 0, 1)


def test_unknown_session_and_incomplete_tail_and_max_records():
    c = Case([dict(over=None, session=7, recs=[(23, 10)], eiv=8),
              dict(recs=[(23, 5), (23, 6)], tail=header(23, TLS12, 900) + bytes(100)),
              dict(over=CC, recs=[(23, 1), (23, 2), (23, 3)])],
             [(0, 100, 0), (100, 100, 0), (200, 100, 0)], app_bytes=300, max_records=5)
    # no overhead is known for the unknown session: its record is placed whole and not opened
    assert c.wres(0) == (1, 0, c.ends[0][0], 21, 0)
    assert c.read(0) == (0, 0, 0, 0, ta.READ_END, 0, 0) and c.exp.placed[0] == 18
    assert c.wres(1) == (2, 2, c.ends[1][1], 0, 2)
    assert c.read(1) == (11, 2, 2, c.ends[1][1], ta.READ_END, 0, 0)
    # truncated by max_records at a record boundary; d_total counts what was framed
    assert c.wres(2) == (2, 2, c.ends[2][1], 0, 2) and c.exp.total == 6
    assert c.read(2) == (3, 2, 2, c.ends[2][1], ta.READ_END, 0, 0)


# -- the checker can fail ------------------------------------------------------------

def failing_case():
    return Case([dict(recs=[(23, 10), (23, 20, BAD_MAC), (23, 30)]), dict(over=CC, recs=[(21, 2)])],
                [(3, 100, 0), (70, 10, 0)], app_bytes=100)


def test_the_checker_passes_the_model_itself_and_ignores_only_the_masked_range():
    c = failing_case()
    compare_read(c.exp, c.got())
    assert list(np.flatnonzero(c.exp.mask)) == list(range(13, 63))
    g = c.got()
    g["app"][13] ^= 1
    g["app"][62] ^= 0x80
    compare_read(c.exp, g)


@pytest.mark.parametrize("at", [0, 2, 3, 12, 63, 99, 100, 163])
def test_the_checker_sees_one_flipped_byte_outside_the_masked_range(at):
    c = failing_case()
    g = c.got()
    g["app"][at] ^= 1
    with pytest.raises(AssertionError, match="d_app byte"):
        compare_read(c.exp, g)


@pytest.mark.parametrize("name,field", [("reads", f) for f in ("app_len", "records", "next", "consumed",
                                                             "stop", "stop_type", "stop_len", "reserved")]
                         + [("results", f) for f in ("first", "records", "delivered", "consumed", "alert",
                                                     "alert_record")])
def test_the_checker_sees_one_flipped_result_field(name, field):
    c = failing_case()
    g = c.got()
    g[name][field][1] += 1
    with pytest.raises(AssertionError, match=field):
        compare_read(c.exp, g)


def test_the_checker_sees_a_descriptor_a_status_and_the_total():
    c = failing_case()
    for key, change in (("recs", lambda g: g["recs"]["out_off"].__setitem__(2, 34)),
                        ("status", lambda g: g["status"].__setitem__(3, 0)),
                        ("total", lambda g: g.__setitem__("total", 3))):
        g = c.got()
        change(g)
        with pytest.raises(AssertionError):
            compare_read(c.exp, g)
