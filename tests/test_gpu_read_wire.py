"""tlsgpu_read_wire on the GPU against the rule's model (read_wire_direct_model.py).

Wire bytes come from the engine's own write side, as in test_gpu_gather_wire.py:
every record of a read stream is one tlsgpu_seal_wire write stream (a record a
write never sends — without content, or of 16,385 bytes — is one
tlsgpu_seal_batch record under a header written here), laid back to back with
continuing sequence numbers; contents come from a seeded generator.  The model
knows what was sealed and what a test tampered with, so nothing on the host
decrypts and every comparison is exact: the whole of d_recs, d_status, d_results,
d_read_results and d_total, and all of d_app (pre-filled with 0xA5, allocated 64
bytes beyond app_bytes) but each stream's unspecified range [app_off + app_len,
app_off + T).  d_wire is downloaded before and after and must not change.
"""
import numpy as np
import pytest

from read_wire_direct_model import (BAD_MAC, OK, Verdicts, check_read_slots, compare_read, overhead,
                                    read_model, wanted_records)
from test_wire import header, model_stream

pytestmark = pytest.mark.gpu

TLS12 = 0x0303
FILL, SLACK, SENTINEL = 0xA5, 64, 0x5A5A5A5A


@pytest.fixture(scope="module")
def ta():
    import talos_amd
    talos_amd.load_library()
    return talos_amd


@pytest.fixture(scope="module")
def engine(ta):
    e = ta.Engine(0)
    yield e
    e.close()


def suites(ta):
    """(kind, the session's tag_len parameter)"""
    return {"aes128gcm": (ta.AES_128_GCM, 0), "aes256gcm": (ta.AES_256_GCM, 0),
            "aes128gcm-tag12": (ta.AES_128_GCM, 12), "chacha": (ta.CHACHA20_POLY1305, 0),
            "chacha-old": (ta.CHACHA20_POLY1305_OLD, 0)}


ALL = ["aes128gcm", "aes256gcm", "aes128gcm-tag12", "chacha", "chacha-old"]


class Wire:
    """Read streams sealed by the engine.  spec: per stream dict(recs=[(type, n) |
    ("raw", type, fragment length)], session=0, tail=b"", gap=3); tamper(sealed,
    layout) edits the sealed bytes and returns the (stream, record) pairs whose tag
    no longer verifies."""

    def __init__(self, ta, engine, suite, spec, seed, tamper=None):
        kind, tag_param = suites(ta)[suite]
        self.over = overhead(kind, tag_param or 16)
        eiv, tag = self.over
        rng = np.random.default_rng(seed)
        self.ta, self.engine = ta, engine
        self.table = ta.SessionTable(engine, 1)
        self.table.install(0, [ta.SessionParams(kind, rng.bytes(ta.KEY_LEN[kind]),
                                                rng.bytes(ta.FIXED_IV_LEN[kind]), tag_len=tag_param)])
        data, writes, byhand, raws, rstreams, pos = bytearray(b"\xC3"), [], [], [], [], 7
        self.contents, self.layout, self.verdicts, self.overs = [], [], {}, []
        for k, st in enumerate(spec):
            seq0, start = 1000 * k + 5, pos
            self.contents.append([])
            self.layout.append([])
            for j, rec in enumerate(st["recs"]):
                if rec[0] == "raw":
                    _, rtype, ln = rec
                    raws.append((pos, header(rtype, TLS12, ln) + rng.bytes(ln)))
                    size, content = 5 + ln, None
                    self.verdicts[(k, j)] = (BAD_MAC, None)
                else:
                    rtype, n = rec
                    size, content = 5 + eiv + n + tag, rng.bytes(n)
                    if 0 < n <= 16384:
                        assert ta.seal_wire_size(kind, n, 0, tag_param) == size
                        writes.append((len(data), pos, seq0 + j, n, 0, TLS12, rtype, 0, 0))
                    else:
                        byhand.append((len(data), pos, seq0 + j, rtype, n, size))
                    data += content
                    self.verdicts[(k, j)] = (OK, content)
                self.contents[k].append(content)
                self.layout[k].append((pos, size))
                pos += size
            tail = st.get("tail", b"")
            raws.append((pos, tail))
            pos += len(tail)
            session = st.get("session", 0)
            self.overs.append(self.over if session == 0 else None)
            rstreams.append((start, pos - start, session, seq0, TLS12, 0, 0))
            pos += st.get("gap", 3)
        self.wire_bytes = pos
        # the write side
        wst = np.array(writes, dtype=ta.WRITE_STREAM_DTYPE)
        est = np.zeros(len(byhand), dtype=ta.RECORD_DTYPE)
        for i, (d, o, seq, rtype, n, _) in enumerate(byhand):
            est[i] = (d, o + 5, seq, 0, ta.len_type(n, rtype))
        B = lambda n: ta.DeviceBuffer(engine, n)  # noqa: E731
        d_data, d_wst, d_srecs, d_sst, d_sres, d_total, d_est, d_wire = (
            B(len(data)), B(max(wst.nbytes, 1)), B(32 * max(len(wst), 1)),
            B(4 * (len(wst) + len(est) + 1)), B(32 * max(len(wst), 1)), B(4), B(max(est.nbytes, 1)),
            B(self.wire_bytes + SLACK))
        d_data.upload(bytes(data))
        d_wire.fill(0)
        if len(wst):
            d_wst.upload(wst.view(np.uint8))
            ta.seal_wire(self.table, d_wst.ptr, len(wst), d_data.ptr, len(data), d_wire.ptr,
                         self.wire_bytes, len(wst), d_srecs.ptr, d_sst.ptr, d_sres.ptr, d_total.ptr)
        if len(est):
            d_est.upload(est.view(np.uint8))
            ta.seal_batch(self.table, d_est.ptr, len(est), d_data.ptr, len(data), d_wire.ptr,
                          self.wire_bytes, d_sst.ptr + 4 * len(wst))
        engine.sync()
        assert (d_sst.download().view(np.int32)[:len(wst) + len(est)] > 0).all()
        sealed = d_wire.download()
        for _, o, _, rtype, _, size in byhand:
            sealed[o:o + 5] = (rtype, 3, 3, (size - 5) >> 8, (size - 5) & 0xFF)
        for o, raw in raws:
            sealed[o:o + len(raw)] = np.frombuffer(raw, dtype=np.uint8)
        for key in (tamper(sealed, self.layout) if tamper else ()):
            self.verdicts[key] = (BAD_MAC, None)
        self.sealed = sealed
        for b in (d_data, d_wst, d_srecs, d_sst, d_sres, d_total, d_est, d_wire):
            b.free()
        self.streams = np.array(rstreams, dtype=ta.WIRE_STREAM_DTYPE)
        self.wanted = wanted_records(self.sealed, self.streams)

    def read(self, reads, app_bytes, max_records=None, wire_bytes=None, equivalence=True):
        """One tlsgpu_read_wire, compared with the model in full; then the follow-up
        open of every stream the plan cut, and the equivalence with the two-call
        path.  Returns (got, exp)."""
        ta, engine, n = self.ta, self.engine, len(self.streams)
        wire_bytes = self.wire_bytes if wire_bytes is None else wire_bytes
        max_records = sum(self.wanted) if max_records is None else max_records
        rd = np.zeros(n, dtype=ta.READ_STREAM_DTYPE)
        for i, row in enumerate(reads):
            rd[i] = row
        B = lambda nbytes: ta.DeviceBuffer(engine, nbytes)  # noqa: E731
        self.dev = d = dict(wire=B(len(self.sealed)), streams=B(self.streams.nbytes),
                            recs=B(32 * max_records), status=B(4 * max_records), results=B(32 * n),
                            total=B(4), reads=B(rd.nbytes), app=B(app_bytes + SLACK), out=B(32 * n))
        try:
            d["wire"].upload(self.sealed)
            d["streams"].upload(self.streams.view(np.uint8))
            d["reads"].upload(rd.view(np.uint8))
            d["app"].fill(FILL)
            d["recs"].fill(0x11)
            d["status"].upload(np.full(max_records, SENTINEL, dtype=np.uint32).view(np.uint8))
            for k in ("results", "out", "total"):
                d[k].fill(0xEE)
            ta.read_wire(self.table, d["streams"].ptr, n, d["wire"].ptr, wire_bytes, max_records,
                         d["recs"].ptr, d["status"].ptr, d["results"].ptr, d["total"].ptr,
                         d["reads"].ptr, d["app"].ptr, app_bytes, d["out"].ptr)
            engine.sync()
            got = dict(recs=d["recs"].download().view(ta.RECORD_DTYPE)[:max_records].copy(),
                       status=d["status"].download().view(np.int32)[:max_records].copy(),
                       results=d["results"].download().view(ta.WIRE_RESULT_DTYPE).copy(),
                       reads=d["out"].download().view(ta.READ_RESULT_DTYPE).copy(),
                       app=d["app"].download(), total=int(d["total"].download().view(np.uint32)[0]))
            assert np.array_equal(d["wire"].download(), self.sealed), "tlsgpu_read_wire wrote d_wire"
            kept = check_read_slots(self.wanted, got["results"], max_records, got["total"])
            slots = [(int(r["first"]), k) for r, k in zip(got["results"], kept)]
            exp = read_model(self.streams, rd, self.sealed, wire_bytes, self.overs, self.verdicts,
                             slots, max_records, np.full(app_bytes + SLACK, FILL, dtype=np.uint8),
                             app_bytes)
            compare_read(exp, got)
            self.follow_up(got, kept)
            if equivalence and got["total"] <= max_records:
                self.two_calls(rd, got, exp, app_bytes, wire_bytes, max_records)
        finally:
            for b in d.values():
                b.free()
        return got, exp

    def follow_up(self, got, kept):
        """Every stream the plan cut, opened again by tlsgpu_open_wire from wire_off +
        consumed with seq + next on a copy of the wire: the stop record and what lies
        behind it open as ssl3_get_record has them."""
        ta, engine = self.ta, self.engine
        cut = [s for s in range(len(self.streams))
               if int(got["results"][s]["records"]) < kept[s] and self.overs[s] is not None
               and int(got["results"][s]["delivered"]) == int(got["results"][s]["records"])]
        if not cut:
            return
        st = self.streams[cut].copy()
        for i, s in enumerate(cut):
            c, nx = int(got["reads"][s]["consumed"]), int(got["reads"][s]["next"])
            assert c == int(got["results"][s]["consumed"]) and nx == int(got["results"][s]["records"])
            st[i]["wire_off"] += c
            st[i]["wire_len"] -= c
            st[i]["seq"] += nx
        nrec = sum(self.wanted)
        B = lambda nbytes: ta.DeviceBuffer(engine, nbytes)  # noqa: E731
        d_wire, d_st, d_recs, d_status, d_res, d_total = (
            B(len(self.sealed)), B(st.nbytes), B(32 * nrec), B(4 * nrec), B(32 * len(cut)), B(4))
        try:
            d_wire.upload(self.sealed)
            d_st.upload(st.view(np.uint8))
            ta.open_wire(self.table, d_st.ptr, len(cut), d_wire.ptr, nrec, d_recs.ptr, d_status.ptr,
                         d_res.ptr, d_total.ptr)
            engine.sync()
            wire = d_wire.download()
            recs = d_recs.download().view(ta.RECORD_DTYPE)
            status = d_status.download().view(np.int32)
            res = d_res.download().view(ta.WIRE_RESULT_DTYPE)
        finally:
            for b in (d_wire, d_st, d_recs, d_status, d_res, d_total):
                b.free()
        oracle = Verdicts(self.verdicts, self.overs)
        for i, s in enumerate(cut):
            off, ln = int(st[i]["wire_off"]), int(st[i]["wire_len"])
            want, consumed, alert, alert_rec, delivered = model_stream(
                oracle, (s, int(self.streams[s]["seq"])), 0, self.sealed[off:off + ln].tobytes(), TLS12,
                False, 0, int(st[i]["seq"]))
            assert len(want) >= 1, ("stream", s, "nothing behind the cut")
            first = int(res[i]["first"])
            assert tuple(int(res[i][f]) for f in ("records", "delivered", "consumed", "alert",
                                                  "alert_record")) == \
                (len(want), delivered, consumed, alert, alert_rec), ("stream", s)
            for k, (stt, pt) in enumerate(want):
                assert int(status[first + k]) == stt, ("stream", s, "record", k)
                if stt >= 0:
                    at = int(recs[first + k]["out_off"])
                    assert wire[at:at + stt].tobytes() == pt, ("stream", s, "record", k)

    def two_calls(self, rd, got, exp, app_bytes, wire_bytes, max_records):
        """tlsgpu_open_wire + tlsgpu_gather_wire on a copy of the same wire with the same
        d_reads: on failure-free streams that stop with END or FULL, the same bytes
        in [app_off, app_off + app_len) and the same read result."""
        ta, engine, d, n = self.ta, self.engine, self.dev, len(self.streams)
        d["wire"].upload(self.sealed)
        d["app"].fill(FILL)
        d["out"].fill(0xEE)
        ta.open_wire(self.table, d["streams"].ptr, n, d["wire"].ptr, max_records, d["recs"].ptr,
                     d["status"].ptr, d["results"].ptr, d["total"].ptr)
        ta.gather_wire(self.table, d["streams"].ptr, d["results"].ptr, n, d["recs"].ptr,
                       d["status"].ptr, max_records, d["wire"].ptr, wire_bytes, d["reads"].ptr,
                       d["app"].ptr, app_bytes, d["out"].ptr)
        engine.sync()
        app = d["app"].download()
        out = d["out"].download().view(ta.READ_RESULT_DTYPE)
        res = d["results"].download().view(ta.WIRE_RESULT_DTYPE)
        compared = 0
        for s in range(n):
            r, w = got["reads"][s], got["results"][s]
            if (int(w["alert"]) > 0 and int(w["delivered"]) < int(w["records"])) or \
                    int(res[s]["delivered"]) < int(res[s]["records"]) or int(rd[s]["start"]) or \
                    int(r["stop"]) not in (ta.READ_END, ta.READ_FULL):
                continue
            for f in ("app_len", "records", "next", "consumed", "stop", "stop_type", "stop_len"):
                assert int(out[s][f]) == int(r[f]), ("stream", s, f, int(out[s][f]), int(r[f]))
            a, ln = int(rd[s]["app_off"]), int(r["app_len"])
            assert np.array_equal(app[a:a + ln], got["app"][a:a + ln]), ("stream", s)
            compared += 1
        self.compared = compared

    def close(self):
        self.table.close()


def res(r):
    return tuple(int(r[f]) for f in ("app_len", "records", "next", "stop", "stop_type", "stop_len"))


# content lengths around the cipher kernels' boundaries: the 16-byte block, the wave's
# 64 blocks (1 KiB), the short-record pack limit (992), 4 KiB, the record limit; 33 makes
# a stream's total 1 modulo 16, so 16 packed streams start at every residue
LENGTHS = [0, 1, 15, 16, 17, 63, 64, 65, 991, 992, 993, 1023, 1024, 1025, 4095, 4097, 16383, 16384,
           33]


@pytest.mark.parametrize("suite", ALL)
def test_placement(ta, engine, suite):
    """16 streams, one per app_off residue 0..15, packed edge to edge with an exact fit
    each: a stray byte at either end of any record lands in a neighbour or a canary."""
    total, lead = sum(LENGTHS), 32
    assert total % 16 == 1
    spec = [dict(recs=[(23, n) for n in LENGTHS[k:] + LENGTHS[:k]]) for k in range(16)]
    w = Wire(ta, engine, suite, spec, seed=21)
    reads = [(lead + k * total, total, 0) for k in range(16)]
    assert sorted(r[0] % 16 for r in reads) == list(range(16))
    got, exp = w.read(reads, lead + 16 * total)
    for k in range(16):
        assert res(got["reads"][k]) == (total, len(LENGTHS), len(LENGTHS), ta.READ_END, 0, 0)
        assert int(got["reads"][k]["consumed"]) == int(w.streams[k]["wire_len"])
        at = reads[k][0]
        assert got["app"][at:at + total].tobytes() == b"".join(w.contents[k])
    assert not exp.mask.any() and w.compared == 16
    assert (got["app"][:lead] == FILL).all() and (got["app"][lead + 16 * total:] == FILL).all()
    w.close()


def test_scan_carry_and_the_second_framing_walk(ta, engine):
    """130 records (the scan's carry over three steps), 1,030 empty records (more than
    the framing kernel's list: its second walk), a stream without records, and a
    FULL in the third step."""
    lens = [1 + (7 * i) % 40 for i in range(130)]
    spec = [dict(recs=[(23, n) for n in lens]), dict(recs=[(23, 0)] * 1030), dict(recs=[]),
            dict(recs=[(23, 5)]), dict(recs=[(23, n) for n in lens]), dict(recs=[(23, 9), (23, 2)])]
    w = Wire(ta, engine, "aes128gcm", spec, seed=22)
    total, short = sum(lens), sum(lens[:129])
    reads = [(3, total, 0), (3 + total, 0, 0), (3 + total, 0, 0), (3 + total, 5, 0),
             (8 + total, short + lens[129] - 1, 0), (8 + total + short, 11, 0)]
    got, exp = w.read(reads, 8 + total + short + 11)
    assert res(got["reads"][0]) == (total, 130, 130, ta.READ_END, 0, 0)
    assert res(got["reads"][1]) == (0, 1030, 1030, ta.READ_END, 0, 0)
    assert res(got["reads"][2]) == (0, 0, 0, ta.READ_END, 0, 0)
    assert res(got["reads"][3]) == (5, 1, 1, ta.READ_END, 0, 0)
    assert res(got["reads"][4]) == (short, 129, 129, ta.READ_FULL, 23, lens[129])
    assert res(got["reads"][5]) == (11, 2, 2, ta.READ_END, 0, 0)
    assert got["app"][3:3 + total].tobytes() == b"".join(w.contents[0])
    assert w.compared == 6
    w.close()


def stop_spec():
    return [dict(recs=[(23, 300), (23, 17), (21, 2), (23, 100), (23, 1)]),      # 0 an alert in mid-stream
            dict(recs=[(22, 40), (23, 9)]),                                      # 1 a handshake record first
            dict(recs=[(23, 100), (23, 1), (23, 27)]),                           # 2 an exact fit
            dict(recs=[(23, 100), (23, 1), (23, 27)]),                           # 3 one byte short
            dict(recs=[(23, 40)]),                                               # 4 app_off > app_bytes
            dict(recs=[(23, 40), (23, 2)]),                                      # 5 start = 1
            dict(recs=[(23, 5), (23, 6)], tail=header(23, TLS12, 900) + bytes(100)),  # 6 incomplete tail
            dict(recs=[(23, 50), (21, 2), (23, 60), (23, 70)]),                  # 7 wrong version behind a cut
            dict(recs=[(23, 50), (23, 60), (23, 70)]),                           # 8 ... and without a cut
            dict(recs=[(23, 10)], session=7),                                    # 9 an unknown session
            dict(recs=[(23, 64), (23, 0), (23, 3)])]                             # 10 nothing special


@pytest.mark.parametrize("suite", ["aes128gcm", "chacha", "aes128gcm-tag12"])
def test_stops_and_cuts(ta, engine, suite):
    def wrong_version(sealed, layout):
        for s, k in ((7, 3), (8, 2)):
            sealed[layout[s][k][0] + 2] = 1         # 0x0301
        return ()
    w = Wire(ta, engine, suite, stop_spec(), seed=23, tamper=wrong_version)
    app_bytes = 1400
    reads = [(0, 500, 0), (500, 100, 0), (600, 128, 0), (728, 127, 0), (app_bytes + 1, 100, 0),
             (900, 100, 1), (1000, 100, 0), (1100, 80, 0), (1180, 110, 0), (1290, 40, 0),
             (1330, 67, 0)]
    got, exp = w.read(reads, app_bytes)
    r, wr = got["reads"], got["results"]
    end = lambda s, k: w.layout[s][k][0] + w.layout[s][k][1] - int(w.streams[s]["wire_off"])  # noqa: E731
    assert res(r[0]) == (317, 2, 2, ta.READ_NOT_APP_DATA, 21, 2) and int(r[0]["consumed"]) == end(0, 1)
    assert res(r[1]) == (0, 0, 0, ta.READ_NOT_APP_DATA, 22, 40) and int(r[1]["consumed"]) == 0
    assert res(r[2]) == (128, 3, 3, ta.READ_END, 0, 0)
    assert res(r[3]) == (101, 2, 2, ta.READ_FULL, 23, 27)
    assert res(r[4]) == (0, 0, 0, ta.READ_FULL, 23, 40)
    assert res(r[5]) == (0, 0, 0, ta.READ_OUT_OF_BOUNDS, 0, 0)
    assert (int(wr[5]["records"]), int(wr[5]["consumed"])) == (0, 0)
    assert res(r[6]) == (11, 2, 2, ta.READ_END, 0, 0) and int(r[6]["consumed"]) == end(6, 1)
    assert res(r[7]) == (50, 1, 1, ta.READ_NOT_APP_DATA, 21, 2)
    assert (int(wr[7]["alert"]), int(wr[7]["alert_record"])) == (0, 1)           # dropped
    assert res(r[8]) == (110, 2, 2, ta.READ_END, 0, 0)
    assert (int(wr[8]["alert"]), int(wr[8]["alert_record"])) == (70, 2)          # reported
    assert res(r[9]) == (0, 0, 0, ta.READ_END, 0, 0)
    assert (int(wr[9]["alert"]), int(wr[9]["delivered"])) == (21, 0)
    assert res(r[10]) == (67, 3, 3, ta.READ_END, 0, 0)
    assert got["total"] == 5 + 2 + 3 + 3 + 1 + 2 + 2 + 3 + 2 + 1 + 3
    assert w.compared == 6                  # streams 2, 3, 4, 6, 8, 10
    w.close()


@pytest.mark.parametrize("suite", ["aes256gcm", "chacha-old"])
def test_a_fragment_that_reaches_past_wire_bytes(ta, engine, suite):
    spec = [dict(recs=[(23, 30), (23, 31)]) for _ in range(5)]
    spec[4]["gap"] = 0
    w = Wire(ta, engine, suite, spec, seed=24)
    reads = [(100 * k, 100, 0) for k in range(5)]
    got, _ = w.read(reads, 500, wire_bytes=w.wire_bytes - 1, equivalence=False)
    for k in range(4):
        assert res(got["reads"][k]) == (61, 2, 2, ta.READ_END, 0, 0)
    assert res(got["reads"][4]) == (30, 1, 1, ta.READ_OUT_OF_BOUNDS, 0, 0)
    assert int(got["results"][4]["records"]) == 1
    w.close()


def test_max_records_truncates_a_stream(ta, engine):
    """Fewer slots than records: one stream is cut at a record boundary, the ones
    whose range starts behind max_records get nothing, d_total counts them all."""
    spec = [dict(recs=[(23, 20 + k + j) for j in range(5)]) for k in range(6)]
    w = Wire(ta, engine, "chacha", spec, seed=25)
    got, exp = w.read([(200 * k, 200, 0) for k in range(6)], 1200, max_records=17)
    assert got["total"] == 30 and int(got["results"]["records"].sum()) == 17
    for k in range(6):
        n = int(got["results"][k]["records"])
        want = sum(20 + k + j for j in range(n))
        assert res(got["reads"][k]) == (want, n, n, ta.READ_END, 0, 0)
    w.close()


@pytest.mark.parametrize("suite", ["aes128gcm", "chacha", "aes128gcm-tag12"])
def test_failures(ta, engine, suite):
    kind, tag_param = suites(ta)[suite]
    eiv, tag = overhead(kind, tag_param or 16)

    def flip_tag(sealed, layout):
        pos, size = layout[0][2]
        sealed[pos + size - 3] ^= 0x20
        return [(0, 2)]
    spec = [dict(recs=[(23, 50), (23, 60), (23, 70), (23, 80), (23, 90)]),       # a flipped tag byte
            dict(recs=[(23, 3), (23, 16385), (23, 1)]),                          # an over-long plaintext
            dict(recs=[(23, 6), ("raw", 23, eiv + tag - 1), (23, 4)]),           # a short fragment
            dict(recs=[(23, 10)]), dict(recs=[(23, 11)]), dict(recs=[(23, 12)])]
    w = Wire(ta, engine, suite, spec, seed=26, tamper=flip_tag)
    reads = [(0, 400, 0), (400, 17000, 0), (17400, 50, 0), (17450, 10, 0), (17460, 11, 0),
             (17471, 12, 0)]
    got, exp = w.read(reads, 17483)
    r, wr = got["reads"], got["results"]
    end = lambda s, k: w.layout[s][k][0] + w.layout[s][k][1] - int(w.streams[s]["wire_off"])  # noqa: E731
    assert res(r[0]) == (110, 2, 2, ta.READ_END, 0, 0) and int(r[0]["consumed"]) == end(0, 1)
    assert (int(wr[0]["alert"]), int(wr[0]["alert_record"]), int(wr[0]["delivered"])) == (20, 2, 2)
    f = int(wr[0]["first"])
    assert list(got["status"][f:f + 5]) == [50, 60, ta.REC_BAD_MAC, ta.REC_SKIPPED, ta.REC_SKIPPED]
    assert res(r[1]) == (3, 1, 1, ta.READ_END, 0, 0)
    assert (int(wr[1]["alert"]), int(wr[1]["alert_record"])) == (22, 1)
    f = int(wr[1]["first"])
    assert list(got["status"][f:f + 3]) == [3, ta.REC_OVERFLOW, ta.REC_SKIPPED]
    assert res(r[2]) == (6, 1, 1, ta.READ_END, 0, 0)
    assert (int(wr[2]["alert"]), int(wr[2]["alert_record"])) == (21, 1)
    # exactly the unspecified ranges are masked: the failing record and what lies behind it
    assert exp.mask.sum() == (70 + 80 + 90) + (16385 + 1) + 4
    assert got["app"][0:110].tobytes() == b"".join(w.contents[0][:2])
    assert w.compared == 3
    w.close()


def test_a_tls13_table_is_refused(ta, engine):
    table = ta.SessionTable(engine, 1)
    table.install(0, [ta.SessionParams(ta.AES_128_GCM, bytes(16), bytes(12), version=0x0304)])
    bufs = [ta.DeviceBuffer(engine, n) for n in (32, 256, 32, 4, 32, 4, 16, 64, 32)]
    d_st, d_wire, d_recs, d_status, d_res, d_total, d_reads, d_app, d_out = bufs
    d_total.fill(0xEE)
    rc = table.lib.tlsgpu_read_wire(table.handle, d_st.ptr, 1, d_wire.ptr, 256, 1, d_recs.ptr,
                                    d_status.ptr, d_res.ptr, d_total.ptr, d_reads.ptr, d_app.ptr, 64,
                                    d_out.ptr, None)
    assert rc == -1 and b"tlsgpu_gather_wire" in table.lib.tlsgpu_last_error()
    engine.sync()
    assert (d_total.download() == 0xEE).all()
    for b in bufs:
        b.free()
    table.close()


def test_argument_errors_and_the_empty_call(ta, engine):
    w = Wire(ta, engine, "chacha", [dict(recs=[(23, 40)])], seed=27)
    B = lambda n: ta.DeviceBuffer(engine, n)  # noqa: E731
    d_wire, d_st, d_recs, d_status, d_res, d_total, d_reads, d_app, d_out = bufs = (
        B(len(w.sealed)), B(32), B(32), B(4), B(32), B(4), B(16), B(64), B(32))
    d_wire.upload(w.sealed)
    d_st.upload(w.streams.view(np.uint8))
    d_reads.upload(np.array([(0, 64, 0)], dtype=ta.READ_STREAM_DTYPE).view(np.uint8))
    d_app.fill(FILL)
    d_total.fill(0xEE)
    lib, t = w.table.lib, w.table.handle

    def call(n_streams, app, reads=d_reads.ptr):
        return lib.tlsgpu_read_wire(t, d_st.ptr, n_streams, d_wire.ptr, w.wire_bytes, 1, d_recs.ptr,
                                    d_status.ptr, d_res.ptr, d_total.ptr, reads, app, 64, d_out.ptr,
                                    None)
    assert call(1, d_wire.ptr + w.wire_bytes - 1) == -1     # d_app's first byte inside d_wire
    assert call(1, d_wire.ptr - 63) == -1                   # its last byte
    assert b"overlaps" in lib.tlsgpu_last_error()
    assert call(1, d_app.ptr, reads=None) == -1
    engine.sync()
    assert (d_total.download() == 0xEE).all() and (d_app.download() == FILL).all()
    assert call(0, d_app.ptr) == 0                          # the empty call clears d_total
    engine.sync()
    assert (d_total.download() == 0).all() and (d_app.download() == FILL).all()
    assert call(1, d_app.ptr) == 0                          # and the call itself works
    engine.sync()
    assert d_app.download()[:40].tobytes() == w.contents[0][0]
    assert np.array_equal(d_wire.download(), w.sealed)
    for b in bufs:
        b.free()
    w.close()
