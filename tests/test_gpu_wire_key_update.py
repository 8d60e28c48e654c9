"""tlsgpu_open_wire's KeyUpdate cut on the GPU against the rule's model
(wire_key_update_model.py), for AES-128-GCM, AES-256-GCM and ChaCha20-Poly1305
TLS 1.3 sessions in one table (session ids 0, 1, 2).

Streams are sealed by tests/tls13_helper.py over the oracle's AEAD (the
reference's where oracle/_ref is built); the next key generations come from
hkdf_expand_label(secret, "traffic upd").  Every comparison is exact: each
result field, every delivered plaintext and inner type, every descriptor slot
(the ones no stream holds are all ones) and the whole of d_wire outside the
consumed spans — the streams lie between canary bytes, and what a call leaves
behind its cut is the next call's ciphertext.
"""
import os

import numpy as np
import pytest

import pyoracle as po
import tls13_helper as t13
import wire_key_update_model as ku

pytestmark = pytest.mark.gpu

ORDER = ["aes128", "aes256", "chacha"]           # session id = index
ENGINE_KIND = {"aes128": 1, "aes256": 2, "chacha": 5}
HASHLEN = {"aes128": 32, "aes256": 48, "chacha": 32}
SENTINEL = 0x5A5A5A5A
CANARY = 0xC3
BIG_SEQ = (1 << 32) + 5


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


@pytest.fixture(scope="module")
def aead(oracle):
    return po.Reference() if os.path.exists(po.LIBREF) else oracle


class Table:
    """One TLS 1.3 session per suite, each with its current key generation."""

    def __init__(self, ta, engine, aead, seed, switch):
        rng = np.random.default_rng(seed)
        self.ta = ta
        self.table = ta.SessionTable(engine, 3)
        self.gens = [None] * 3
        for sid, suite in enumerate(ORDER):
            self.install(sid, ku.Generation(aead, suite, rng.bytes(HASHLEN[suite])))
        if switch:      # (a table never told otherwise has the switch off)
            ta.sessions_wire_key_update(self.table, True)

    def install(self, sid, gen):
        self.gens[sid] = gen
        self.table.install(sid, [self.ta.SessionParams(ENGINE_KIND[gen.suite], gen.key, gen.iv,
                                                       version=t13.VERSION)])

    def close(self):
        self.table.close()


class Wire:
    """A wire buffer on the device: streams (dict(wire, sid, seq[, shift])) laid
    between canary bytes, stream k's first fragment byte at residue `shift`
    modulo 16.  open() is one tlsgpu_open_wire over spans of it."""

    def __init__(self, ta, engine, streams):
        self.ta, self.engine = ta, engine
        image = bytearray([CANARY] * 7)
        for s in streams:
            image += bytes([CANARY] * ((-len(image) - 5 + s.get("shift", 0)) % 16))
            s["off"] = len(image)
            image += s["wire"] + bytes([CANARY] * 3)
        image += bytes([CANARY] * 64)
        self.image = bytes(image)            # what the device holds now
        self.d_wire = ta.DeviceBuffer(engine, len(image))
        self.d_wire.upload(self.image)

    def open(self, table, spans, max_records):
        """spans: [(off, length, sid, seq)].  Returns the call's outputs; the
        image before the call stays in got["before"]."""
        ta, engine = self.ta, self.engine
        descs = np.zeros(len(spans), dtype=ta.WIRE_STREAM_DTYPE)
        for i, (off, length, sid, seq) in enumerate(spans):
            descs[i] = (off, length, sid, seq, 0x0303, 0, 0)
        bufs = [ta.DeviceBuffer(engine, n) for n in (descs.nbytes, 32 * max_records, 4 * max_records,
                                                     32 * len(spans), 4)]
        d_streams, d_recs, d_status, d_results, d_total = bufs
        d_streams.upload(descs.view(np.uint8))
        d_status.upload(np.full(max_records, SENTINEL, dtype=np.uint32).view(np.uint8))
        d_results.fill(0xEE)
        ta.open_wire(table.table, d_streams.ptr, len(spans), self.d_wire.ptr, max_records,
                     d_recs.ptr, d_status.ptr, d_results.ptr, d_total.ptr)
        engine.sync()
        got = dict(before=self.image, wire=self.d_wire.download().tobytes(), spans=spans,
                   max_records=max_records, bufs=bufs,
                   recs=d_recs.download().view(ta.RECORD_DTYPE).copy(),
                   status=d_status.download().view(np.int32).copy(),
                   results=d_results.download().view(ta.WIRE_RESULT_DTYPE).copy(),
                   total=int(d_total.download().view(np.uint32)[0]))
        self.image = got["wire"]
        return got

    def close(self):
        self.d_wire.free()


def free(got):
    for b in got["bufs"]:
        b.free()


def key_update_of(results):
    """The key_update field (the first reserved word of the old layout)."""
    return [int(r["reserved"][0]) for r in results]


def check(ta, table, got, switch, slots=None):
    """One call's outputs against the model, in full.  slots: descriptor slots
    left for the (single) stream of a call that max_records truncates."""
    before, after = got["before"], got["wire"]
    recs_raw = got["recs"].view(np.uint8).reshape(-1, 32)
    covered = np.zeros(got["max_records"], dtype=bool)
    may_change = np.zeros(len(before), dtype=bool)
    models, total = [], 0
    kus = key_update_of(got["results"])
    for i, (off, length, sid, seq) in enumerate(got["spans"]):
        m = table.gens[sid].model(before[off:off + length], seq, switch, slots)
        models.append(m)
        r = got["results"][i]
        have = (int(r["records"]), int(r["delivered"]), int(r["consumed"]), int(r["alert"]),
                int(r["alert_record"]), kus[i], int(r["reserved"][1]))
        want = (m["records"], m["delivered"], m["consumed"], m["alert"], m["alert_record"],
                m["key_update"], 0)
        assert have == want, (i, have, want)
        total += m["walked"]
        first = int(r["first"])
        assert not covered[first:first + m["records"]].any(), "two streams share a slot"
        covered[first:first + m["records"]] = True
        may_change[off:off + m["consumed"]] = True
        for k, ((st, region, itype), (pos, ln)) in enumerate(zip(m["recs"], m["framed"])):
            d, frag = got["recs"][first + k], off + pos + 5
            assert int(d["in_off"]) == frag == int(d["out_off"]), (i, k)
            assert (int(d["seq"]), int(d["session"])) == (seq + k, sid), (i, k)
            assert int(d["len_type"]) & 0xFFFFFF == ln
            assert int(got["status"][first + k]) == st, (i, k, int(got["status"][first + k]), st)
            if region is not None:      # delivered, or zero-filled by a failed tag
                assert after[frag:frag + len(region)] == region, (i, k)
                assert int(d["len_type"]) >> 24 == itype, (i, k)
    # the slots no stream holds (behind a cut, or never reserved) are all ones
    assert (recs_raw[~covered] == 0xFF).all()
    assert got["total"] == total
    # not a byte outside the consumed spans has changed: behind every cut lies
    # the ciphertext that was there, and the canaries between the streams
    a, b = np.frombuffer(after, dtype=np.uint8), np.frombuffer(before, dtype=np.uint8)
    bad = np.flatnonzero((a != b) & ~may_change)
    assert bad.size == 0, f"{bad.size} bytes outside the consumed spans changed, first at {bad[0]}"
    return models


def spans_of(streams):
    return [(s["off"], len(s["wire"]), s["sid"], s["seq"]) for s in streams]


def short(i):
    return bytes((7 * i + j) & 0xFF for j in range(1 + i % 9))


def stream_with_key_update(gen, sid, seq, at, n, rr=0, pad=0):
    """n records: application data under `gen`, a KeyUpdate at index `at`, the rest
    under the next generation from sequence number 0."""
    nxt = gen.next()
    parts = [gen.rec(seq + i, short(i)) for i in range(at)]
    parts.append(gen.key_update(seq + at, rr, pad))
    parts += [nxt.rec(i, short(at + 1 + i)) for i in range(n - at - 1)]
    return dict(wire=b"".join(parts), sid=sid, seq=seq, cut=sum(map(len, parts[:at + 1])))


def test_position(ta, engine, aead):
    """The KeyUpdate at the wave-step boundaries of a stream of 131 records, and
    as its last record; the sequence numbers cross 2^32 inside the stream."""
    t = Table(ta, engine, aead, 1, True)
    streams = []
    for sid in range(3):
        for at in (0, 1, 62, 63, 64, 65, 129, 130):
            streams.append(stream_with_key_update(t.gens[sid], sid, (1 << 32) - 60 + sid, at, 131,
                                                  rr=at & 1, pad=at % 3))
    w = Wire(ta, engine, streams)
    got = w.open(t, spans_of(streams), 131 * len(streams))
    models = check(ta, t, got, True)
    for s, m in zip(streams, models):
        assert (m["delivered"], m["consumed"]) == (m["records"], s["cut"])
        assert m["key_update"] in (ku.KU_UPDATE, ku.KU_UPDATE_REQUESTED) and m["walked"] == 131
    assert sorted({m["records"] for m in models}) == [1, 2, 63, 64, 65, 66, 130, 131]
    free(got)
    w.close()
    t.close()


def test_shape_of_the_candidate(ta, engine, aead):
    """Inner lengths 6, 15, 16, 17 and 512, request_update 0 and 1, sequence numbers
    0 and 2^32 + 5, and the candidate's first byte at every residue modulo 16."""
    t = Table(ta, engine, aead, 2, True)
    streams, want = [], []
    for sid in range(3):
        for pad in (0, 9, 10, 11, 506):
            for res in range(16):
                rr, seq = res & 1, BIG_SEQ if res & 2 else 0
                s = stream_with_key_update(t.gens[sid], sid, seq, 0, 2, rr, pad)
                s["shift"] = res
                streams.append(s)
                want.append(ku.KU_UPDATE + rr)
    w = Wire(ta, engine, streams)
    assert sorted({(s["off"] + 5) % 16 for s in streams}) == list(range(16))
    got = w.open(t, spans_of(streams), 2 * len(streams))
    models = check(ta, t, got, True)
    assert key_update_of(got["results"]) == want
    assert all(m["records"] == 1 and m["walked"] == 2 for m in models)
    free(got)
    w.close()
    t.close()


def test_full_rekey(ta, engine, aead):
    """data, KeyUpdate, data under the next keys, a second KeyUpdate (update
    requested), data under the third keys: each call stops at the KeyUpdate, the
    caller installs the next generation and goes on at wire_off + consumed with
    seq = 0; every record opens bit-exact.  tlsgpu_gather_wire after the first
    call stops at the KeyUpdate record."""
    t = Table(ta, engine, aead, 3, True)
    streams, contents = [], []
    for sid in range(3):
        g0 = t.gens[sid]
        g1 = g0.next()
        g2 = g1.next()
        c = [[short(i) + bytes(40 * sid) for i in range(3)], [short(5), short(6) * 200],
             [short(7) * 9, short(8)]]
        parts = ([g0.rec(9 + i, x) for i, x in enumerate(c[0])] + [g0.key_update(12, 0, 3)] +
                 [g1.rec(i, x) for i, x in enumerate(c[1])] + [g1.key_update(2, 1)] +
                 [g2.rec(i, x) for i, x in enumerate(c[2])])
        streams.append(dict(wire=b"".join(parts), sid=sid, seq=9, gens=[g0, g1, g2]))
        contents.append(c)
    w = Wire(ta, engine, streams)
    spans = spans_of(streams)
    for phase, (nrec, verdict) in enumerate([(4, ku.KU_UPDATE), (3, ku.KU_UPDATE_REQUESTED),
                                             (2, ku.KU_NONE)]):
        got = w.open(t, spans, 32)
        models = check(ta, t, got, True)
        assert key_update_of(got["results"]) == [verdict] * 3
        assert [int(r["delivered"]) for r in got["results"]] == [nrec] * 3
        for sid, (m, r) in enumerate(zip(models, got["results"])):
            for k, content in enumerate(contents[sid][phase]):
                st, region, itype = m["recs"][k]
                assert (st, region[:st], itype) == (len(content), content, 23)
        if phase == 0:      # the read path stops at the KeyUpdate record
            rd = np.zeros(3, dtype=ta.READ_STREAM_DTYPE)
            for sid in range(3):
                rd[sid] = (256 * sid, 256, 0)
            d_reads, d_app, d_out = (ta.DeviceBuffer(engine, n) for n in (rd.nbytes, 768, 96))
            d_reads.upload(rd.view(np.uint8))
            d_streams, d_recs, d_status, d_results, _ = got["bufs"]
            ta.gather_wire(t.table, d_streams.ptr, d_results.ptr, 3, d_recs.ptr, d_status.ptr, 32,
                           w.d_wire.ptr, len(w.image), d_reads.ptr, d_app.ptr, 768, d_out.ptr)
            engine.sync()
            out = d_out.download().view(ta.READ_RESULT_DTYPE)
            app = d_app.download().tobytes()
            for sid in range(3):
                assert (int(out[sid]["stop"]), int(out[sid]["stop_type"]), int(out[sid]["stop_len"]),
                        int(out[sid]["next"])) == (ta.READ_NOT_APP_DATA, 22, 5, 3)
                data = b"".join(contents[sid][0])
                assert app[256 * sid:256 * sid + len(data)] == data
            for b in (d_reads, d_app, d_out):
                b.free()
        # the caller's part: the next generation into the read slot, on from `consumed`, seq 0
        spans = [(off + int(r["consumed"]), length - int(r["consumed"]), sid, 0)
                 for (off, length, sid, _), r in zip(spans, got["results"])]
        free(got)
        if phase < 2:
            for sid in range(3):
                t.install(sid, streams[sid]["gens"][phase + 1])
    assert all(length == 0 for _, length, _, _ in spans)
    w.close()
    t.close()


def test_look_alikes_are_held(ta, engine, aead):
    """What the peek takes for a KeyUpdate and the open does not confirm:
    TLSGPU_WIRE_KU_HELD, the bytes behind intact, and on under the same keys."""
    t = Table(ta, engine, aead, 4, True)
    like = bytes.fromhex("180000010016") + bytes(40)
    streams = []
    for sid in range(3):
        g = t.gens[sid]
        # application data that begins like a KeyUpdate
        streams.append(dict(wire=g.rec(0, short(1)) + g.rec(1, like) + g.rec(2, short(2)) +
                            g.rec(3, short(3)), sid=sid, seq=0))
        # a true KeyUpdate with one tag bit flipped
        forged = bytearray(g.key_update(21, 0, 2))
        forged[-3] ^= 0x20
        streams.append(dict(wire=g.rec(20, short(4)) + bytes(forged) + g.next().rec(0, short(5)),
                            sid=sid, seq=20))
        # an authentic handshake record: the message's bytes, ten zeros, four more bytes
        more = bytes.fromhex("180000010016") + bytes(10) + b"\x09\x08\x07\x06"
        streams.append(dict(wire=g.rec(BIG_SEQ, more, 22, 5) + g.rec(BIG_SEQ + 1, short(6)), sid=sid,
                            seq=BIG_SEQ))
    w = Wire(ta, engine, streams)
    got = w.open(t, spans_of(streams), 32)
    check(ta, t, got, True)
    assert key_update_of(got["results"]) == [ku.KU_HELD] * 9
    res = [(int(r["records"]), int(r["delivered"]), int(r["alert"])) for r in got["results"]]
    assert res == [(2, 2, 0), (2, 1, 20), (1, 1, 0)] * 3
    third = got["results"][2]
    assert int(got["status"][int(third["first"])]) == 20      # its status is not 5
    # the look-alike streams go on under the same keys with seq + records
    spans = [(off + int(r["consumed"]), length - int(r["consumed"]), sid, seq + int(r["records"]))
             for (off, length, sid, seq), r in zip(got["spans"], got["results"])]
    free(got)
    keep = [0, 2, 3, 5, 6, 8]      # (a stream ended by its alert does not go on)
    got = w.open(t, [spans[i] for i in keep], 32)
    check(ta, t, got, True)
    assert key_update_of(got["results"]) == [ku.KU_NONE] * 6
    assert [(int(r["records"]), int(r["delivered"])) for r in got["results"]] == [(2, 2), (1, 1)] * 3
    free(got)
    w.close()
    t.close()


def outputs(got):
    return (got["wire"], got["recs"].tobytes(), got["status"].tobytes(), got["results"].tobytes(),
            got["total"])


def on_and_off(ta, engine, table, streams, max_records):
    """The same call with the switch on and off, from the same wire image and the
    same preset buffers: both calls' outputs."""
    both = []
    for on in (True, False):
        ta.sessions_wire_key_update(table.table, on)
        w = Wire(ta, engine, streams)
        got = w.open(table, spans_of(streams), max_records)
        both.append(got)
        w.close()
    return both


@pytest.mark.parametrize("sid", range(3))
def test_not_candidates(ta, engine, aead, sid):
    """request_update 2, byte 5 not 0x16, an inner plaintext of 5 bytes, and a
    non-zero byte 15: no cut, every output equal to the switch-off run's."""
    t = Table(ta, engine, aead, 5, True)
    g = t.gens[sid]
    streams = []
    for k, inner in enumerate(["180000010216", "180000010017", "1800000116",
                               "180000010016" + "00" * 9 + "17"]):
        seq = 100 * k
        streams.append(dict(wire=g.rec(seq, short(k)) + g.rec(seq + 1, None, inner=bytes.fromhex(inner))
                            + g.rec(seq + 2, short(k + 1)), sid=sid, seq=seq))
    on, off = on_and_off(ta, engine, t, streams, 16)
    assert outputs(on) == outputs(off)
    models = check(ta, t, on, True)
    assert all(m["records"] == 3 and m["delivered"] == 3 and m["key_update"] == 0 for m in models)
    free(on)
    free(off)
    t.close()


def test_neutral_without_a_key_update(ta, engine, aead):
    """A TLS 1.3 batch without any KeyUpdate, a failing tag and a stream naming a
    session out of range included: identical outputs with the switch on and off."""
    t = Table(ta, engine, aead, 6, True)
    streams = []
    for sid in range(3):
        g = t.gens[sid]
        parts = [g.rec(i, short(i) * (1 + 300 * (i % 3))) for i in range(70)]
        if sid == 1:    # one flipped ciphertext bit in record 35
            parts[35] = parts[35][:7] + bytes([parts[35][7] ^ 1]) + parts[35][8:]
        streams.append(dict(wire=b"".join(parts), sid=sid, seq=0))
    streams.append(dict(wire=t.gens[0].key_update(0) + t.gens[0].rec(1, short(1)), sid=7, seq=0))
    on, off = on_and_off(ta, engine, t, streams, 256)
    assert outputs(on) == outputs(off)
    assert key_update_of(on["results"]) == [0] * 4
    assert [(int(r["delivered"]), int(r["alert"])) for r in on["results"]][:3] == \
        [(70, 0), (35, 20), (70, 0)]
    free(on)
    free(off)
    t.close()


def test_neutral_on_a_tls12_table(ta, engine, oracle):
    """On a TLS 1.2 table the switch is accepted and changes nothing, whatever the
    plaintext looks like."""
    rng = np.random.default_rng(7)
    table = ta.SessionTable(engine, 2)
    params, sess = [], []
    for kind, okind in ((ta.AES_128_GCM, po.AES_128_GCM), (ta.CHACHA20_POLY1305, po.CHACHA20_POLY1305)):
        key, iv = rng.bytes(po.KEY_LEN[okind]), rng.bytes(po.FIXED_IV_LEN[okind])
        params.append(ta.SessionParams(kind, key, iv))
        sess.append(oracle.tls_session(okind, key, iv))
    table.install(0, params)
    streams = []
    for sid in range(2):
        wire = b""
        for i, (rtype, pt) in enumerate([(23, short(3)), (22, ku.key_update_message(0)),
                                         (23, bytes.fromhex("180000010016") + bytes(10)), (23, short(4))]):
            body = oracle.tls_seal(sess[sid], 5 + i, rtype, pt)
            wire += bytes([rtype, 3, 3, len(body) >> 8, len(body) & 0xFF]) + body
        streams.append(dict(wire=wire, sid=sid, seq=5))

    class T:
        pass
    t = T()
    t.table = table
    on, off = on_and_off(ta, engine, t, streams, 16)
    assert outputs(on) == outputs(off)
    assert [(int(r["records"]), int(r["delivered"]), int(r["alert"])) for r in on["results"]] == \
        [(4, 4, 0)] * 2
    assert key_update_of(on["results"]) == [0, 0]
    free(on)
    free(off)
    table.close()


def test_switch_off_is_todays_outcome(ta, engine, aead):
    """Never told about the switch, a stream with a KeyUpdate ends as it always
    has: bad_record_mac at the record behind it, whose ciphertext is gone."""
    t = Table(ta, engine, aead, 8, False)
    streams = [stream_with_key_update(t.gens[sid], sid, 4, 2, 5) for sid in range(3)]
    w = Wire(ta, engine, streams)
    got = w.open(t, spans_of(streams), 16)
    check(ta, t, got, False)
    res = [(int(r["records"]), int(r["delivered"]), int(r["alert"]), int(r["alert_record"]))
           for r in got["results"]]
    assert res == [(5, 3, 20, 3)] * 3 and key_update_of(got["results"]) == [0] * 3
    for s in streams:       # the zero-fill has destroyed the record behind the KeyUpdate
        at = s["off"] + s["cut"] + 5
        assert got["wire"][at:at + 4] == bytes(4) != got["before"][at:at + 4]
    free(got)
    w.close()
    t.close()


@pytest.mark.parametrize("sid", range(3))
def test_truncation(ta, engine, aead, sid):
    """max_records cutting the stream in front of, at and behind the candidate."""
    t = Table(ta, engine, aead, 9, True)
    s = stream_with_key_update(t.gens[sid], sid, 0, 2, 5, rr=1)
    want = {2: (2, ku.KU_NONE), 3: (3, ku.KU_UPDATE_REQUESTED), 4: (3, ku.KU_UPDATE_REQUESTED)}
    for max_records, (records, verdict) in want.items():
        w = Wire(ta, engine, [s])
        got = w.open(t, spans_of([s]), max_records)
        check(ta, t, got, True, slots=max_records)
        assert (int(got["results"][0]["records"]), key_update_of(got["results"])[0]) == (records, verdict)
        free(got)
        w.close()
    t.close()
