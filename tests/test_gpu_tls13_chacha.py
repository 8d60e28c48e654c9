"""TLS 1.3 ChaCha20-Poly1305 (TLSGPU_CHACHA20_POLY1305_TLS13, kind 5) on the
GPU: batch, wire and host paths against tests/tls13_helper.py over the
oracle's RFC 7905 AEAD (kind 3; the reference's where oracle/_ref is built).
test_tls13_chacha_helper.py checks that pairing against records captured from
an OpenSSL TLS_CHACHA20_POLY1305_SHA256 connection.

Conventions of test_gpu_tls13.py: output and status buffers start from a
sentinel, the whole output buffer is compared, every batch runs twice and both
images are equal, sequence numbers carry bits in both nonce words, and for a
seal d_in is 0xC3 around every content, so a type byte read from d_in shows.

The staged ChaCha kernel runs one record per lane, 64 per wave, 256 per
workgroup, moves 16-byte pieces of 64-byte ChaCha blocks in 128-byte steps, and
a wave runs as many steps as its longest record.  So the shapes are small:
about 700 records per batch (not a multiple of 64, several workgroups), and
content lengths around every piece, block and step boundary, where the type
byte (inner plaintext = content + 1) is last in a piece, alone in a new piece,
block or step, or second in one; 16383 / 16384 are the record bound.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import pyoracle as po
import tls13_helper as t13
import test_gpu_tls13 as gcm13   # the wire runner and model, and the pinned allocator

from conftest import ROOT

pytestmark = pytest.mark.gpu

LENS = [0, 1, 14, 15, 16, 17, 47, 48, 62, 63, 64, 65, 111, 112, 126, 127, 128, 129, 255, 256,
        1023, 1024, 16383, 16384]
SHORT = LENS[:-2]
PADS = gcm13.PADS
NSESS = 5
SENTINEL = 0x5A5A5A5A
GOOD, TAMPER, OOB, SHORT15, EMPTY_SESSION, ALL_ZERO, EMPTY_INNER = range(7)
GOLDEN = os.path.join(os.path.dirname(t13.GOLDEN), "tls13_wire_chacha.json")


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


# engine kind -> the oracle kind whose AEAD the helper runs under
ORACLE_KIND = {5: po.CHACHA20_POLY1305, 1: po.AES_128_GCM, 2: po.AES_256_GCM}


def _sessions(ta, aead, kinds, seed):
    """[(SessionParams, oracle ctx)] for engine kinds `kinds`."""
    rng = np.random.default_rng(seed)
    out = []
    for k in kinds:
        p = ta.SessionParams(k, rng.bytes(ta.KEY_LEN[k]), rng.bytes(12), version=t13.VERSION)
        out.append((p, aead.aead(ORACLE_KIND[k], p.key)))
    return out


_cache = {}


def _material(aead, sessions, key, plan):
    """plan: [(session, inner type, content length, padding, what)] -> per record
    the content, the inner plaintext and the helper's fragment, once per key."""
    if key not in _cache:
        rng = np.random.default_rng(len(plan))
        recs = []
        for i, (sid, itype, n, pad, what) in enumerate(plan):
            seq = (1 << 33) + 1000 + i          # both nonce words carry sequence bits
            content = rng.bytes(n)
            if what == ALL_ZERO:
                inner = bytes(n + 1 + pad)
            elif what == EMPTY_INNER:
                inner = b""
            else:
                inner = t13.inner_plaintext(content, itype, pad)
            p, ctx = sessions[sid]
            frag = t13.seal_inner(aead, ctx, p.fixed_iv, seq, inner)
            recs.append(dict(sid=sid, seq=seq, itype=itype, content=content, inner=inner, frag=frag,
                             what=what))
        _cache[key] = recs
    return _cache[key]


def _run_case(ta, engine, aead, sessions, mode, key, plan, in_shifts=None, out_shifts=None,
              hints=None):
    """One table of `sessions` (+ one empty slot), one batch laid out here: slot
    i at a 16-byte boundary + its shift, with gaps, d_in 0xC3 and d_out 0xA5."""
    recs = _material(aead, sessions, key, plan)
    n = len(recs)
    table = ta.SessionTable(engine, len(sessions) + 1)
    table.install(0, [p for p, _ in sessions])
    if hints is not None:
        table.hint(hints)
    payloads = []
    for i, r in enumerate(recs):
        payload = r["content"] if mode == "seal" else r["frag"]
        if r["what"] == TAMPER:
            b = bytearray(payload)
            b[(7 * i) % len(b)] ^= 1 << (i % 8)
            payload = bytes(b)
        elif r["what"] == SHORT15:
            payload = payload[:15]
        payloads.append(payload)
    descs = np.zeros(n, dtype=ta.RECORD_DTYPE)
    ip = op = 0
    for i, (r, payload) in enumerate(zip(recs, payloads)):
        ip += (-ip) % 16 + (in_shifts[i] if in_shifts else 0)
        op += (-op) % 16 + (out_shifts[i] if out_shifts else 0)
        sid = len(sessions) if r["what"] == EMPTY_SESSION else r["sid"]
        descs[i] = (ip, op, r["seq"], sid, ta.len_type(len(payload), r["itype"]))
        ip += len(payload) + 3
        op += (len(payload) + 17 if mode == "seal" else max(len(payload) - 16, 0)) + 3
    in_bytes, out_bytes = ip - 3 if n else 1, op + 16       # the last payload ends d_in
    host_in = np.full(max(in_bytes, 1), 0xC3, dtype=np.uint8)
    for d, payload in zip(descs, payloads):
        o = int(d["in_off"])
        host_in[o:o + len(payload)] = np.frombuffer(payload, dtype=np.uint8)
    out_offs = [int(d["out_off"]) for d in descs]
    for i, r in enumerate(recs):
        if r["what"] == OOB:
            descs[i]["in_off"] = in_bytes + 16
    exp_out = np.full(out_bytes, 0xA5, dtype=np.uint8)
    exp_st = np.zeros(n, dtype=np.int32)
    for i, r in enumerate(recs):
        what, o = r["what"], out_offs[i]
        if what == OOB:
            exp_st[i] = ta.REC_OUT_OF_BOUNDS
        elif what == EMPTY_SESSION or (what == SHORT15 and mode == "open"):
            exp_st[i] = ta.REC_PUBLIC_INVALID
        elif mode == "seal":
            res = r["frag"]                  # plans for seal carry no padding
            exp_st[i] = len(r["content"]) + 1 + 16
            assert len(res) == exp_st[i]
            exp_out[o:o + len(res)] = np.frombuffer(res, dtype=np.uint8)
        elif what == TAMPER:
            exp_st[i] = ta.REC_BAD_MAC
            exp_out[o:o + len(r["inner"])] = 0          # the whole inner span
        else:
            cl = t13.content_length(r["inner"])
            exp_st[i] = ta.REC_NO_CONTENT_TYPE if cl is None else cl
            exp_out[o:o + len(r["inner"])] = np.frombuffer(r["inner"], dtype=np.uint8)
    bufs = [ta.DeviceBuffer(engine, b) for b in (len(host_in), out_bytes, max(descs.nbytes, 32),
                                                 4 * max(n, 1))]
    d_in, d_out, d_recs, d_status = bufs
    d_in.upload(host_in)
    d_recs.upload(descs.view(np.uint8))
    images = []
    for _ in range(2):
        d_out.fill(0xA5)
        d_status.upload(np.full(max(n, 1), SENTINEL, dtype=np.uint32).view(np.uint8))
        fn = ta.seal_batch if mode == "seal" else ta.open_batch
        fn(table, d_recs.ptr, n, d_in.ptr, in_bytes, d_out.ptr, out_bytes, d_status.ptr, None)
        engine.sync()
        out = d_out.download()[:out_bytes].copy()
        st = d_status.download().view(np.int32)[:n].copy()
        images.append((out, st))
        bad = np.flatnonzero(st != exp_st)
        assert bad.size == 0, (mode, key, "status", bad[:8].tolist(), st[bad[:8]].tolist(),
                               exp_st[bad[:8]].tolist(), [plan[j] for j in bad[:8]])
        diff = np.flatnonzero(out != exp_out)
        if diff.size:
            rec = int(np.searchsorted(np.asarray(out_offs), diff[0], side="right")) - 1
            raise AssertionError((mode, key, "output byte", int(diff[0]), "record", rec, plan[rec],
                                  int(diff[0]) - out_offs[rec]))
    assert (images[0][1] == images[1][1]).all() and (images[0][0] == images[1][0]).all()
    for b in bufs:
        b.free()
    table.close()


def _lengths_plan():
    """700 records = 10 whole waves and a partial one of 60, three workgroups.
    Waves 0-3: the short lengths in turn, lanes alternating among the five
    sessions.  Waves 4 and 5: one 16 KiB record (16383, 16384) among short ones.
    Waves 6 and 7: a single active lane (129 and 1024 bytes), every other lane
    names the empty session.  Waves 8 and 9: whole waves of one session (the key
    words come through the scalar path), every length up to 1024.  The last wave
    holds all of LENS, the two 16 KiB ones included, in 60 lanes."""
    plan = []
    for i in range(4 * 64):
        plan.append((i % NSESS, 21 + i % 3, SHORT[(i + i // 64) % len(SHORT)], 0, GOOD))
    for w, (big, lane) in enumerate(((16383, 17), (16384, 40))):
        for j in range(64):
            n = big if j == lane else SHORT[(3 * j + w) % 18]       # short ones: <= 129
            plan.append(((j + w) % NSESS, 21 + j % 3, n, 0, GOOD))
    for n, lane in ((129, 29), (1024, 63)):
        for j in range(64):
            plan.append((2, 23, n if j == lane else 40, 0, GOOD if j == lane else EMPTY_SESSION))
    for w in range(2):
        for j in range(64):
            plan.append((3 + w, 21 + j % 3, SHORT[(j + 5 * w) % len(SHORT)], 0, GOOD))
    for j in range(60):
        plan.append((j % NSESS, 21 + j % 3, LENS[(j + 7) % len(LENS)], 0, GOOD))
    assert len(plan) == 700
    return plan


@pytest.mark.parametrize("layout", ["aligned", "in-shifted", "out-shifted"])
@pytest.mark.parametrize("mode", ["seal", "open"])
def test_content_lengths(ta, engine, aead, mode, layout):
    """A table of kind 5 only (fused: the NARROW kernel checks bounds and writes
    the statuses of the empty-session lanes itself).  16-byte aligned slots, and
    byte shifts 1-15 of in_off or of out_off on every other record."""
    plan = _lengths_plan()
    shifts = [0 if i % 2 == 0 else 1 + (i // 2) % 15 for i in range(len(plan))]
    sessions = _sessions(ta, aead, [ta.CHACHA20_POLY1305_TLS13] * NSESS, 11)
    _run_case(ta, engine, aead, sessions, mode, "lengths", plan,
              in_shifts=shifts if layout == "in-shifted" else None,
              out_shifts=shifts if layout == "out-shifted" else None)


def _open_plan(nsess, n_runs=32):
    """Runs of 22 records: every padding of PADS against contents of 0, 1, 37,
    200 and 1000 bytes, and in every run an all-zero inner plaintext, an empty
    one (a 16-byte fragment), a tampered record, a 15-byte fragment, an
    out-of-bounds descriptor or an empty session, each next to good records."""
    plan = []
    contents = [0, 1, 37, 200, 1000]
    for run in range(n_runs):
        sid = run % nsess
        for j in range(16):
            k = 16 * run + j
            plan.append(((sid + (j % 2) * (run % 3)) % nsess, 21 + k % 3,
                         contents[(run + j) % len(contents)], PADS[(k + run // 5) % len(PADS)], GOOD))
        plan.append((sid, 23, 40 + run % 50, PADS[run % len(PADS)], ALL_ZERO))
        plan.append((sid, 23, 0, 0, EMPTY_INNER))
        plan.append((sid, 22, 300 + run, PADS[(run + 3) % len(PADS)], TAMPER))
        plan.append((sid, 23, 100, 0, SHORT15))
        plan.append((sid, 23, 64, 16, OOB if run % 2 else EMPTY_SESSION))
        plan.append((sid, 21, 2, 1100, GOOD))
    return plan


def test_open_padding_and_statuses(ta, engine, aead):
    """The ChaCha unpad pass on a kind-5 table: the content length whatever the
    padding, NO_CONTENT_TYPE with the region as decrypted, BAD_MAC with the whole
    inner span zero, PUBLIC_INVALID / OUT_OF_BOUNDS untouched."""
    sessions = _sessions(ta, aead, [ta.CHACHA20_POLY1305_TLS13] * NSESS, 12)
    plan = _open_plan(NSESS)
    assert len(plan) == 704
    shifts = [0 if i % 3 else i % 16 for i in range(len(plan))]
    _run_case(ta, engine, aead, sessions, "open", "open", plan, in_shifts=shifts)


@pytest.mark.parametrize("mode", ["seal", "open"])
def test_mixed_table_with_gcm(ta, engine, aead, mode):
    """Kind 5 beside TLS 1.3 AES-128 and AES-256 sessions in one table and one
    batch, hints 0: the wide ChaCha kernel after check_record_bounds, and on open
    three unpad passes, each record taken by its own session's pass only."""
    kinds = [ta.CHACHA20_POLY1305_TLS13, ta.AES_128_GCM, ta.AES_256_GCM,
             ta.CHACHA20_POLY1305_TLS13, ta.AES_128_GCM, ta.CHACHA20_POLY1305_TLS13]
    sessions = _sessions(ta, aead, kinds, 13)
    if mode == "open":
        plan = _open_plan(len(kinds))
    else:
        plan = [((i // 7 + i % 2) % len(kinds), 21 + i % 3, LENS[i % 22], 0,
                 OOB if i % 97 == 50 else EMPTY_SESSION if i % 89 == 30 else GOOD)
                for i in range(690)]
        plan += [(0, 23, 16384, 0, GOOD), (1, 23, 16383, 0, GOOD), (3, 22, 16383, 0, GOOD)]
    shifts = [0 if i % 2 else (5 * i) % 16 for i in range(len(plan))]
    _run_case(ta, engine, aead, sessions, mode, "mixed-" + mode, plan, in_shifts=shifts, hints=0)


def test_open_content_ending_in_zero_bytes(ta, engine, aead):
    """Content that ends in 1, 15, 16 or 17 zero bytes, with and without
    padding: the scan stops at the type byte, not inside the content."""
    from talos_amd.batch import RecordBatch
    kind = ta.CHACHA20_POLY1305_TLS13
    sessions = _sessions(ta, aead, [kind] * NSESS, 14)
    table = ta.SessionTable(engine, NSESS)
    table.install(0, [p for p, _ in sessions])
    entries, want = [], []
    for i, (n, zeros, pad) in enumerate((n, z, p) for n in (1, 16, 17, 100, 2000)
                                        for z in (1, 15, 16, 17) for p in PADS):
        content = bytes([1 + i % 250]) * max(n - zeros, 0) + bytes(min(zeros, n))
        inner = t13.inner_plaintext(content, 21 + i % 3, pad)
        p, ctx = sessions[i % NSESS]
        entries.append((i % NSESS, i, 23, t13.seal_inner(aead, ctx, p.fixed_iv, i, inner), kind))
        want.append((len(content), inner))
    batch = RecordBatch(engine, entries, "open", tls13=True)    # accepts kind 5 entries
    batch.run(table)
    engine.sync()
    out = batch.d_out.download()
    st = batch.d_status.download().view(np.int32)[:batch.n]
    for i, (cl, inner) in enumerate(want):
        o = batch.out_offs[i]
        assert int(st[i]) == cl and out[o:o + len(inner)].tobytes() == inner, (i, int(st[i]), cl)
        assert out[o + cl] == inner[cl] in (21, 22, 23)
    batch.free()
    table.close()


def test_install_rules(ta, engine):
    """Kind 5 needs version 0x0304, key 32, the 12-byte IV and a 16-byte tag, and
    is a TLS 1.3 session for the table's generation rule."""
    key16, key32, iv12 = bytes(16), bytes(32), bytes(range(12))
    k5 = ta.CHACHA20_POLY1305_TLS13

    def rc(table, slot, p):
        return table.lib.tlsgpu_sessions_install(table.handle, slot, 1, C.byref(p.to_c()))

    table = ta.SessionTable(engine, 4)
    for p in (ta.SessionParams(k5, key32, iv12, version=0x0303),
              ta.SessionParams(k5, key32, iv12),                     # the default version
              ta.SessionParams(k5, key32, iv12[:4], version=0x0304),
              ta.SessionParams(k5, key32, b"", version=0x0304),
              ta.SessionParams(k5, key32, iv12, tag_len=12, version=0x0304),
              ta.SessionParams(k5, key16, iv12, version=0x0304)):
        assert rc(table, 0, p) == -1, p                              # TLSGPU_EINVAL
    # beside 0x0304 GCM sessions: accepted, in either order
    table.install(0, [ta.SessionParams(ta.AES_128_GCM, key16, iv12, version=0x0304),
                      ta.SessionParams(k5, key32, iv12, version=0x0304),
                      ta.SessionParams(ta.AES_256_GCM, key32, iv12, tag_len=16, version=0x0304)])
    table.install(3, [ta.SessionParams(k5, key32, iv12, tag_len=16, version=0x0304)])
    # kind 3 into a TLS 1.3 table
    assert rc(table, 3, ta.SessionParams(ta.CHACHA20_POLY1305, key32, iv12)) == -1
    table.close()
    table = ta.SessionTable(engine, 2)      # kind 5 into a TLS 1.2 table
    table.install(0, [ta.SessionParams(ta.CHACHA20_POLY1305, key32, iv12)])
    assert rc(table, 1, ta.SessionParams(k5, key32, iv12, version=0x0304)) == -1
    table.close()
    table = ta.SessionTable(engine, 2)      # a table that kind 5 opened is TLS 1.3
    table.install(0, [ta.SessionParams(k5, key32, iv12, version=0x0304)])
    assert rc(table, 1, ta.SessionParams(ta.AES_128_GCM, key16, iv12[:4])) == -1
    table.install(1, [ta.SessionParams(ta.AES_128_GCM, key16, iv12, version=0x0304)])
    table.close()


# -- wire paths ----------------------------------------------------------------

def _fixture_table(ta, engine, aead):
    fx = t13.load_fixture(GOLDEN)
    assert fx["suite"] == "TLS_CHACHA20_POLY1305_SHA256"
    dirs = fx["directions"]
    table = ta.SessionTable(engine, len(dirs))
    table.install(0, [ta.SessionParams(ta.CHACHA20_POLY1305_TLS13, d["key"], d["iv"],
                                       version=t13.VERSION) for d in dirs])
    keys = [(aead.aead(po.CHACHA20_POLY1305, d["key"]), d["iv"]) for d in dirs] if aead else None
    return dirs, table, keys


def test_open_wire_fixture_streams(ta, engine, aead):
    """The captured OpenSSL connection, each direction one stream (and once more
    from its third record, at another alignment): contents, inner types (the
    server's NewSessionTickets arrive as type 22 in the descriptors), consumed."""
    dirs, table, keys = _fixture_table(ta, engine, aead)
    streams = []
    for sid, d in enumerate(dirs):
        wires = [r["wire"] for r in d["records"]]
        streams.append(dict(wire=b"".join(wires), seq=0, session=sid))
        streams.append(dict(wire=b"".join(wires[2:]) + wires[0][:9], seq=2, session=sid, shift=7))
    got = gcm13._run_open_wire(ta, engine, table, streams, 64)
    gcm13._check_open_wire(ta, aead, keys, streams, got)
    types = set()
    for sid, d in enumerate(dirs):
        r = got["results"][2 * sid]
        assert int(r["alert"]) == 0 and int(r["records"]) == len(d["records"]) == int(r["delivered"])
        for k, rec in enumerate(d["records"]):
            idx = int(r["first"]) + k
            o = int(got["recs"][idx]["out_off"])
            assert int(got["status"][idx]) == len(rec["content"])
            assert got["wire"][o:o + len(rec["content"])] == rec["content"]
            assert int(got["recs"][idx]["len_type"]) >> 24 == rec["inner_type"]
            types.add(rec["inner_type"])
    assert types >= {22, 23}
    table.close()


def test_open_wire_failures(ta, engine, aead):
    """A non-23 outer type, an over-long fragment and a record without a content
    type end their streams with alerts 10, 22 and 10; later records are SKIPPED."""
    rng = np.random.default_rng(6)
    key, iv = rng.bytes(32), rng.bytes(12)
    ctx = aead.aead(po.CHACHA20_POLY1305, key)
    table = ta.SessionTable(engine, 1)
    table.install(0, [ta.SessionParams(ta.CHACHA20_POLY1305_TLS13, key, iv, version=t13.VERSION)])

    def rec(seq, n, itype=23, pad=0, inner=None):
        inner = t13.inner_plaintext(rng.bytes(n), itype, pad) if inner is None else inner
        f = t13.seal_inner(aead, ctx, iv, seq, inner)
        return t13.header(len(f)) + f

    def stream(parts, seq):
        return dict(wire=b"".join(parts), seq=seq, session=0)

    S = []
    S.append(stream([rec(0, 10), rec(1, 0, 21, 5), rec(2, 16384), rec(3, 300, 22, 255)], 0))
    outer22 = bytearray(rec(12, 40))
    outer22[0] = 22
    S.append(stream([rec(10, 100), rec(11, 7), bytes(outer22), rec(13, 9)], 10))        # alert 10
    S.append(stream([rec(20, 50), bytes([23, 3, 3]) + (16641).to_bytes(2, "big") + bytes(16641),
                     rec(22, 5)], 20))                                                # alert 22
    S.append(stream([rec(30, 1), rec(31, 0, inner=bytes(33)), rec(32, 8), rec(33, 8)], 30))  # alert 10
    S.append(stream([rec(40, 2), rec(41, 0, inner=b""), rec(42, 8)], 40))              # alert 10
    S.append(stream([rec(50, 16384, 23, 239)], 50))     # a fragment of 16384 + 256 bytes: accepted
    tampered = bytearray(rec(61, 700, 23, 17))
    tampered[300] ^= 2
    S.append(stream([rec(60, 5), bytes(tampered), rec(62, 5)], 60))                    # alert 20
    S.append(stream([rec(70, 30), bytes([23, 3, 3, 0, 15]) + bytes(15), rec(72, 1)], 70))   # alert 21
    got = gcm13._run_open_wire(ta, engine, table, S, 64)
    gcm13._check_open_wire(ta, aead, [(ctx, iv)], S, got)
    assert [int(r["alert"]) for r in got["results"]] == [0, 10, 22, 10, 10, 0, 20, 21]
    assert [int(r["delivered"]) for r in got["results"]] == [4, 2, 1, 1, 1, 1, 1, 1]
    r = got["results"][3]
    st = got["status"][int(r["first"]):int(r["first"]) + 4].tolist()
    assert st == [1, ta.REC_NO_CONTENT_TYPE, ta.REC_SKIPPED, ta.REC_SKIPPED]
    table.close()


def test_seal_wire_reproduces_the_captured_wire(ta, engine):
    """Every write of the captured connection (and the server's tickets, inner
    type 22) through tlsgpu_seal_wire: byte-identical records, next_seq and
    wire_len of the TLS 1.3 framing."""
    kind = ta.CHACHA20_POLY1305_TLS13
    dirs, table, _ = _fixture_table(ta, engine, None)
    jobs = []       # (session, seq, inner type, data, expected wire)
    for sid, d in enumerate(dirs):
        app = [r for r in d["records"] if r["inner_type"] == 23]
        for r in d["records"]:
            if r["inner_type"] != 23:
                jobs.append((sid, r["seq"], r["inner_type"], r["content"], r["wire"]))
        k = 0
        for w in d["writes"]:
            n = len(t13.frame(bytes(w)))
            recs = app[k:k + n]
            k += n
            jobs.append((sid, recs[0]["seq"], 23, b"".join(r["content"] for r in recs),
                         b"".join(r["wire"] for r in recs)))
    data, wire_off, streams = bytearray(), 0, np.zeros(len(jobs), dtype=ta.WRITE_STREAM_DTYPE)
    for i, (sid, seq, itype, content, want) in enumerate(jobs):
        data += b"\xC3" * (1 + i % 5)          # non-zero bytes before every write
        size = ta.seal_wire_size(kind, len(content))
        assert size == len(want)
        streams[i] = (len(data), wire_off, seq, len(content), sid, 0x0303, itype, 0, 0)
        data += content
        wire_off += size + 3
    nrec = sum(len(t13.frame(j[3])) for j in jobs)
    bufs = [ta.DeviceBuffer(engine, n) for n in (len(data), wire_off + 64, streams.nbytes,
                                                 32 * nrec, 4 * nrec, 32 * len(jobs), 4)]
    d_data, d_wire, d_streams, d_recs, d_status, d_results, d_total = bufs
    d_data.upload(bytes(data))
    d_wire.fill(0xA5)
    d_streams.upload(streams.view(np.uint8))
    ta.seal_wire(table, d_streams.ptr, len(jobs), d_data.ptr, len(data), d_wire.ptr, wire_off + 64,
                 nrec, d_recs.ptr, d_status.ptr, d_results.ptr, d_total.ptr)
    engine.sync()
    wire = d_wire.download().tobytes()
    res = d_results.download().view(ta.WRITE_RESULT_DTYPE)
    st = d_status.download().view(np.int32)[:nrec]
    assert int(d_total.download().view(np.uint32)[0]) == nrec
    exp = bytearray(b"\xA5" * len(wire))
    for i, (sid, seq, itype, content, want) in enumerate(jobs):
        o = int(streams[i]["wire_off"])
        exp[o:o + len(want)] = want
        n = len(t13.frame(content))
        assert (int(res[i]["records"]), int(res[i]["wire_len"]), int(res[i]["next_seq"])) == \
            (n, len(want), seq + n), (i, res[i])
        for k, piece in enumerate(t13.frame(content)):
            assert int(st[int(res[i]["first"]) + k]) == len(piece) + 17
    assert wire == bytes(exp)
    for b in bufs:
        b.free()
    table.close()


# -- host paths ----------------------------------------------------------------

def test_host_seal_open_round_trip(ta, engine, aead):
    """tlsgpu_seal_host then tlsgpu_open_host (in place, with a read hook) of a
    few hundred records: the seal span grows by the type byte, the hook sees
    every record's content."""
    rng = np.random.default_rng(92)
    sessions = _sessions(ta, aead, [ta.CHACHA20_POLY1305_TLS13] * NSESS, 15)
    table = ta.SessionTable(engine, NSESS)
    table.install(0, [p for p, _ in sessions])
    lens = [LENS[i % 22] for i in range(300)] + [16384, 16383, 0, 1]
    recs, ip, op = [], 0, 0
    for i, n in enumerate(lens):
        sid, seq, itype = (i // 9) % NSESS, 5000 + i, 21 + i % 3
        content = rng.bytes(n)
        ip += (-ip) % 16 + (i % 4)
        op += (-op) % 16 + (i % 3)
        p, ctx = sessions[sid]
        recs.append((sid, seq, itype, content, ip, op,
                     t13.seal(aead, ctx, p.fixed_iv, seq, itype, content)))
        ip += n + 2
        op += n + 17 + 2
    keep = []
    in_bytes, out_bytes, n = ip, op, len(recs)
    h_in, h_out = (gcm13._pinned(engine, b, keep) for b in (in_bytes, out_bytes))
    h_recs, h_status = gcm13._pinned(engine, 32 * n, keep), gcm13._pinned(engine, 4 * n, keep)
    C.memset(h_in, 0xC3, in_bytes)
    C.memset(h_out, 0xA5, out_bytes)
    descs = np.zeros(n, dtype=ta.RECORD_DTYPE)
    for i, (sid, seq, itype, content, io, oo, frag) in enumerate(recs):
        C.memmove(h_in + io, content, len(content))
        descs[i] = (io, oo, seq, sid, ta.len_type(len(content), itype))
    C.memmove(h_recs, descs.tobytes(), descs.nbytes)
    seen = []

    def on_read(ssl, data, plen):
        seen.append(C.string_at(data, plen[0]))

    ta.host_pipeline(engine, 4, 64 << 10)
    try:
        ta.seal_host(table, h_recs, n, h_in, in_bytes - 2, h_out, out_bytes, h_status)
        st = np.ctypeslib.as_array((C.c_int32 * n).from_address(h_status)).copy()
        for i, (sid, seq, itype, content, io, oo, frag) in enumerate(recs):
            assert st[i] == len(content) + 17 and C.string_at(h_out + oo, len(frag)) == frag, i
        for i, (sid, seq, itype, content, io, oo, frag) in enumerate(recs):
            descs[i] = (oo, oo, seq, sid, ta.len_type(len(frag), 23))
        C.memmove(h_recs, descs.tobytes(), descs.nbytes)
        cbs = ta.talos_register(on_read, None)
        try:
            ta.open_host(table, h_recs, n, h_out, out_bytes, h_out, out_bytes, h_status)
        finally:
            ta.talos_register(None, None)
            del cbs
        st = np.ctypeslib.as_array((C.c_int32 * n).from_address(h_status)).copy()
        for i, (sid, seq, itype, content, io, oo, frag) in enumerate(recs):
            assert st[i] == len(content), (i, st[i])
            assert C.string_at(h_out + oo, len(content) + 1) == content + bytes([itype]), i
        assert [len(s) for s in seen] == lens and seen == [r[3] for r in recs]
    finally:
        ta.host_pipeline(engine, 2, 32 << 20)
        for p in keep:
            engine.lib.tlsgpu_host_free(engine.handle, p)
        table.close()


# -- the legacy switch -----------------------------------------------------------

_LEGACY_CHILD = r"""
import os, sys
root = sys.argv[1]
sys.path[:0] = [root, os.path.join(root, "oracle"), os.path.join(root, "tests")]
import numpy as np
import pyoracle as po
import tls13_helper as t13
import talos_amd as ta
from talos_amd.batch import RecordBatch
assert os.environ["TLSGPU_CHACHA_LEGACY"] == "1"
ta.load_library()
po.build()
aead = po.Reference() if os.path.exists(po.LIBREF) else po.Oracle()
rng = np.random.default_rng(16)
kind = ta.CHACHA20_POLY1305_TLS13
params = [ta.SessionParams(kind, rng.bytes(32), rng.bytes(12), version=t13.VERSION) for _ in range(3)]
ctxs = [aead.aead(po.CHACHA20_POLY1305, p.key) for p in params]
eng = ta.Engine(0)
table = ta.SessionTable(eng, 3)
table.install(0, params)
lens = [0, 1, 15, 16, 17, 63, 64, 127, 128, 129, 1024, 16384] * 6 + [5]
recs = [(i % 3, (1 << 33) + i, 21 + i % 3, rng.bytes(n)) for i, n in enumerate(lens)]
frags = [t13.seal(aead, ctxs[s], params[s].fixed_iv, q, t, c) for s, q, t, c in recs]
sb = RecordBatch(eng, [(s, q, t, c, kind) for s, q, t, c in recs], "seal", tls13=True)
sb.run(table)
for (st, body), f in zip(sb.results(), frags):
    assert st == len(f) and body == f, "seal"
padded = [t13.seal(aead, ctxs[s], params[s].fixed_iv, q, t, c, pad=i % 40)
          for i, (s, q, t, c) in enumerate(recs)]
ob = RecordBatch(eng, [(s, q, 23, f, kind) for (s, q, t, c), f in zip(recs, padded)], "open", tls13=True)
ob.run(table)
for (st, pt), (s, q, t, c) in zip(ob.results(), recs):
    assert st == len(c) and pt == c, "open"
table.close()
eng.close()
print("OK")
"""


def test_legacy_switch_leaves_kind5_alone():
    """TLSGPU_CHACHA_LEGACY=1 is an A/B switch for TLS 1.2: in a fresh process
    with it set, kind-5 seals and opens give the same results (the staged
    kernel runs them whatever the switch says)."""
    env = dict(os.environ, TLSGPU_CHACHA_LEGACY="1")
    r = subprocess.run([sys.executable, "-c", _LEGACY_CHILD, ROOT], env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0 and "OK" in r.stdout, \
        f"rc={r.returncode}\n" + r.stdout[-2000:] + r.stderr[-3000:]
