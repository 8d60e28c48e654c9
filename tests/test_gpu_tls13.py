"""TLS 1.3 record protection (RFC 8446 5.2-5.4) on the GPU: batch, wire and
host paths of a TLS 1.3 session table against tests/tls13_helper.py (the
oracle's AEAD, or the reference's where oracle/_ref is built, under the RFC's
nonce, additional data and inner plaintext; the helper itself is checked
against captured OpenSSL records in test_tls13_helper.py).

As in test_gpu_record_handover.py: output and status buffers start from a
sentinel, the whole output buffer is compared, every batch runs twice, batches
hold more than 4,096 records so that waves take a second record, and the
hints 3 / 0 / 2 select the fused no-pack kernel, the device-side selection and
the fused pack variant of the queue kernel; split and ttable get a smaller
case each.

Content lengths are the smallest at which each path can go wrong: the inner
plaintext is content + 1 byte, so 15 / 16 / 17 put the type byte last in a
block, alone in a block and second in one; 991 / 992 are 62 / 63 blocks of
inner plaintext (the pack boundary); 1023 / 1024, 2047 / 2048, 4095 / 4096 and
16383 / 16384 are inner lengths of a whole step, step pair, group and record,
and one byte more — the type byte then takes a tail path of its own.

A session table holds one record generation, so instead of mixed batches the
install rule is tested.
"""
import ctypes as C
import os

import numpy as np
import pytest

import pyoracle as po
import tls13_helper as t13

pytestmark = pytest.mark.gpu

KINDS = {"aes-128-gcm": po.AES_128_GCM, "aes-256-gcm": po.AES_256_GCM}
LENS = [0, 1, 14, 15, 16, 17, 31, 991, 992, 1007, 1008, 1023, 1024, 2047, 2048, 4095, 4096,
        16383, 16384]
NEIGHBOURS = [0, 1, 15, 16, 991, 992, 1008, 1024, 2047, 4096]   # every ordered pair of these
PADS = [0, 1, 15, 16, 17, 63, 64, 65, 255, 1100]
VARIANTS = [3, 0, 2]
NSESS = 5
SENTINEL = 0x5A5A5A5A
GOOD, TAMPER, OOB, SHORT15, EMPTY_SESSION, ALL_ZERO, EMPTY_INNER = range(7)


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
    """The AEAD under the helper: the reference's EVP_AEAD where it is built."""
    return po.Reference() if os.path.exists(po.LIBREF) else oracle


@pytest.fixture
def impl(ta, request):
    prev = ta.get_gcm_impl()
    ta.set_gcm_impl(getattr(request, "param", "queue"))
    yield
    ta.set_gcm_impl(prev)


def _params(ta, name, seed):
    kind = KINDS[name]
    rng = np.random.default_rng(seed + kind)
    return [ta.SessionParams(kind, rng.bytes(po.KEY_LEN[kind]), rng.bytes(12), version=t13.VERSION)
            for _ in range(NSESS)]


_cache = {}


def _material(ta, aead, name, key, plan):
    """plan: [(session, inner type, content length, padding, what)].  Keys,
    contents and the helper's fragments, computed once per plan and key size."""
    if (name, key) not in _cache:
        params = _params(ta, name, len(plan))
        ctxs = [aead.aead(p.aead, p.key) for p in params]
        rng = np.random.default_rng(3 * len(plan) + KINDS[name])
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
            frag = t13.seal_inner(aead, ctxs[sid], params[sid].fixed_iv, seq, inner)
            recs.append(dict(sid=sid, seq=seq, itype=itype, content=content, inner=inner,
                             frag=frag, what=what))
        _cache[(name, key)] = (params, recs)
    return _cache[(name, key)]


def _run_case(ta, engine, aead, name, mode, hints, key, plan, shifts=0):
    from talos_amd.batch import RecordBatch
    params, recs = _material(ta, aead, name, key, plan)
    kind = KINDS[name]
    table = ta.SessionTable(engine, NSESS + 1)
    table.install(0, params)
    table.hint(hints)
    entries = []
    for i, r in enumerate(recs):
        what = r["what"]
        payload = r["content"] if mode == "seal" else r["frag"]
        if what == TAMPER:
            b = bytearray(payload)
            b[(7 * i) % len(b)] ^= 1 << (i % 8)
            payload = bytes(b)
        elif what == SHORT15:
            payload = payload[:15]
        entries.append((NSESS if what == EMPTY_SESSION else r["sid"], r["seq"], r["itype"], payload,
                        kind))
    images = []
    for _ in range(2):
        batch = RecordBatch(engine, entries, mode, in_shift=shifts, tls13=True)
        descs = batch.d_recs.download().view(ta.RECORD_DTYPE).copy()
        if mode == "seal":
            # d_in ends with the last record's content, and every content is
            # preceded (and followed) by non-zero bytes that are no content type:
            # a type byte read from d_in gives a wrong ciphertext
            end = max(int(descs[-1]["in_off"]) + len(entries[-1][3]), 1)
            host_in = np.full(end, 0xC3, dtype=np.uint8)
            for d, e in zip(descs, entries):
                o = int(d["in_off"])
                host_in[o:o + len(e[3])] = np.frombuffer(e[3], dtype=np.uint8)
            batch.d_in.free()
            batch.d_in = ta.DeviceBuffer(engine, end)
            batch.d_in.upload(host_in)
        for i, r in enumerate(recs):
            if r["what"] == OOB:
                descs[i]["in_off"] = batch.d_in.nbytes + 16
        batch.d_recs.upload(descs.view(np.uint8))
        batch.d_status.upload(np.full(max(batch.n, 1), SENTINEL, dtype=np.uint32).view(np.uint8))
        batch.run(table)
        engine.sync()
        out = batch.d_out.download().copy()
        st = batch.d_status.download().view(np.int32)[:batch.n].copy()
        images.append((out, st))
        exp_out = np.full(out.shape, 0xA5, dtype=np.uint8)
        exp_st = np.zeros(batch.n, dtype=np.int32)
        for i, r in enumerate(recs):
            what, o = r["what"], batch.out_offs[i]
            if what == OOB:
                exp_st[i] = ta.REC_OUT_OF_BOUNDS
            elif what in (SHORT15, EMPTY_SESSION) and (mode == "open" or what == EMPTY_SESSION):
                exp_st[i] = ta.REC_PUBLIC_INVALID
            elif mode == "seal":
                res = r["frag"]          # plans for seal carry no padding
                exp_st[i] = len(r["content"]) + 1 + 16
                assert len(res) == exp_st[i]
                exp_out[o:o + len(res)] = np.frombuffer(res, dtype=np.uint8)
            elif what == TAMPER:
                exp_st[i] = ta.REC_BAD_MAC
                exp_out[o:o + len(r["inner"])] = 0          # the whole inner span
            else:
                inner = r["inner"]
                cl = t13.content_length(inner)
                exp_st[i] = ta.REC_NO_CONTENT_TYPE if cl is None else cl
                if cl is not None:
                    assert cl == len(r["content"]) or r["content"].endswith(b"\0") or what != GOOD
                exp_out[o:o + len(inner)] = np.frombuffer(inner, dtype=np.uint8)
        bad = np.flatnonzero(st != exp_st)
        assert bad.size == 0, (name, mode, hints, "status", bad[:8].tolist(), st[bad[:8]].tolist(),
                               exp_st[bad[:8]].tolist(), [plan[j] for j in bad[:8]])
        diff = np.flatnonzero(out != exp_out)
        if diff.size:
            rec = int(np.searchsorted(np.asarray(batch.out_offs), diff[0], side="right")) - 1
            raise AssertionError((name, mode, hints, "output byte", int(diff[0]), "record", rec,
                                  plan[rec], int(diff[0]) - batch.out_offs[rec]))
        batch.free()
    assert (images[0][1] == images[1][1]).all() and (images[0][0] == images[1][0]).all()
    table.close()


def _lengths_plan():
    """Every ordered pair of NEIGHBOURS as neighbours and all of LENS, one such
    sequence per session run (rotated from run to run), 20 runs over the five
    sessions: 4,380 records, so workgroup ranges end inside runs.  Inner types
    21, 22, 23 in turn."""
    seq = [n for a in NEIGHBOURS for b in NEIGHBOURS for n in (a, b)] + LENS
    plan = []
    for run in range(20):
        rot = (37 * run) % len(seq)
        for n in seq[rot:] + seq[:rot]:
            plan.append((run % NSESS, 21 + len(plan) % 3, n, 0, GOOD))
    assert len(plan) > 4096
    return plan


@pytest.mark.parametrize("shifted", [False, True])
@pytest.mark.parametrize("hints", VARIANTS)
@pytest.mark.parametrize("mode", ["seal", "open"])
@pytest.mark.parametrize("name", list(KINDS))
def test_content_lengths(ta, engine, aead, impl, name, mode, hints, shifted):
    """16-B aligned slots (the wide step loops run, and stop before the block
    that holds the type byte), and aligned slots alternating with byte-shifted
    ones (dword and byte tails)."""
    plan = _lengths_plan()
    shifts = [0 if i % 2 == 0 or not shifted else 1 + (i // 2) % 15 for i in range(len(plan))]
    _run_case(ta, engine, aead, name, mode, hints, "lengths", plan, shifts=shifts)


def _open_plan():
    """4,400 records in runs of 22: every padding with contents of 0, 1, 37 and
    a few hundred bytes, contents that end in zero bytes (made below), and in
    every run an all-zero inner plaintext, an empty one, a tampered record, a
    15-byte fragment, an out-of-bounds descriptor and an empty session, each
    next to good records."""
    plan = []
    contents = [0, 1, 37, 200, 600, 1000, 1024, 5000]
    for run in range(200):
        sid = run % NSESS
        for j in range(16):
            k = 16 * run + j
            plan.append((sid, 21 + k % 3, contents[(run + j) % len(contents)],
                         PADS[(k + run // 8) % len(PADS)], GOOD))
        plan.append((sid, 23, 40 + run % 50, PADS[run % len(PADS)], ALL_ZERO))
        plan.append((sid, 23, 0, 0, EMPTY_INNER))
        plan.append((sid, 22, 300 + run, PADS[(run + 3) % len(PADS)], TAMPER))
        plan.append((sid, 23, 100, 0, SHORT15))
        plan.append((sid, 23, 64, 16, OOB if run % 2 else EMPTY_SESSION))
        plan.append((sid, 21, 2, 1100, GOOD))
    return plan


@pytest.mark.parametrize("hints", VARIANTS)
@pytest.mark.parametrize("name", list(KINDS))
def test_open_padding_and_statuses(ta, engine, aead, impl, name, hints):
    """The unpad pass: the content length is the index of the last non-zero
    byte whatever the padding, NO_CONTENT_TYPE leaves the region as decrypted,
    BAD_MAC zeroes the whole inner span, negative statuses stay."""
    _run_case(ta, engine, aead, name, "open", hints, "open", _open_plan())


def test_open_content_ending_in_zero_bytes(ta, engine, aead, impl):
    """Content whose last bytes are zero, with and without padding: the scan
    stops at the type byte, not inside the content."""
    name = "aes-128-gcm"
    params = _params(ta, name, 77)
    ctxs = [aead.aead(p.aead, p.key) for p in params]
    table = ta.SessionTable(engine, NSESS + 1)
    table.install(0, params)
    from talos_amd.batch import RecordBatch
    entries, want = [], []
    for i, (n, zeros, pad) in enumerate((n, z, p) for n in (1, 16, 17, 100, 2000)
                                        for z in (1, 15, 16, 17) for p in PADS):
        content = bytes([1 + i % 250]) * max(n - zeros, 0) + bytes(min(zeros, n))
        inner = t13.inner_plaintext(content, 21 + i % 3, pad)
        entries.append((i % NSESS, i, 23, t13.seal_inner(aead, ctxs[i % NSESS],
                                                         params[i % NSESS].fixed_iv, i, inner),
                        KINDS[name]))
        want.append((len(content), inner))
    batch = RecordBatch(engine, entries, "open", tls13=True)
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


@pytest.mark.parametrize("impl", ["split", "ttable"], indirect=True)
@pytest.mark.parametrize("mode", ["seal", "open"])
@pytest.mark.parametrize("name", list(KINDS))
def test_split_and_ttable(ta, engine, aead, impl, name, mode):
    """The split kernel (the record's blocks over 16 waves: the type byte lies
    in the last wave's range) and the T-table kernel through parse_tls."""
    plan = [(i % NSESS if i % 40 < 33 else (i + 1) % NSESS, 21 + i % 3, LENS[i % len(LENS)],
             PADS[i % len(PADS)] if mode == "open" else 0, GOOD) for i in range(190)]
    plan += [(0, 23, 48000, 0, GOOD), (0, 23, 65000 + 15, 0, GOOD)]   # several steps per wave
    if mode == "open":
        plan += [(1, 23, 50, 17, ALL_ZERO), (1, 23, 0, 0, EMPTY_INNER), (1, 23, 500, 3, TAMPER),
                 (1, 23, 100, 0, SHORT15), (2, 23, 9, 0, OOB), (2, 23, 9, 0, EMPTY_SESSION)]
    shifts = [0 if i % 3 else i % 16 for i in range(len(plan))]
    _run_case(ta, engine, aead, name, mode, 0, "small-" + mode, plan, shifts=shifts)


def test_install_rules(ta, engine):
    """0x0304 needs AES-GCM, the 12-byte IV and a 16-byte tag; a table holds
    one record generation."""
    key16, key32, iv12 = bytes(16), bytes(32), bytes(range(12))
    table = ta.SessionTable(engine, 4)
    bad = [ta.SessionParams(ta.AES_128_GCM, key16, iv12[:4], version=0x0304),
           ta.SessionParams(ta.AES_128_GCM, key16, b"", version=0x0304),
           ta.SessionParams(ta.CHACHA20_POLY1305, key32, iv12, version=0x0304),
           ta.SessionParams(ta.CHACHA20_POLY1305_OLD, key32, b"", version=0x0304),
           ta.SessionParams(ta.AES_256_GCM, key32, iv12, tag_len=12, version=0x0304)]
    for p in bad:
        rc = table.lib.tlsgpu_sessions_install(table.handle, 0, 1, C.byref(p.to_c()))
        assert rc == -1, (p, rc)          # TLSGPU_EINVAL
    table.install(0, [ta.SessionParams(ta.AES_128_GCM, key16, iv12, version=0x0304),
                      ta.SessionParams(ta.AES_256_GCM, key32, iv12, tag_len=16, version=0x0304)])
    for p in (ta.SessionParams(ta.AES_128_GCM, key16, iv12[:4]),
              ta.SessionParams(ta.CHACHA20_POLY1305, key32, iv12)):
        assert table.lib.tlsgpu_sessions_install(table.handle, 2, 1, C.byref(p.to_c())) == -1
    table.close()
    table = ta.SessionTable(engine, 2)      # and the other way round
    table.install(0, [ta.SessionParams(ta.AES_128_GCM, key16, iv12[:4])])
    p = ta.SessionParams(ta.AES_128_GCM, key16, iv12, version=0x0304)
    assert table.lib.tlsgpu_sessions_install(table.handle, 1, 1, C.byref(p.to_c())) == -1
    table.close()


# -- wire paths ----------------------------------------------------------------

def _run_open_wire(ta, engine, table, streams, max_records):
    """streams: [dict(wire, seq, session)] -> wire image, statuses, results, descriptors."""
    wire = bytearray()
    descs = np.zeros(len(streams), dtype=ta.WIRE_STREAM_DTYPE)
    offs = []
    for i, s in enumerate(streams):
        wire += bytes((-len(wire) - 5 + s.get("shift", 0)) % 16)
        offs.append(len(wire))
        descs[i] = (len(wire), len(s["wire"]), s["session"], s["seq"], 0x0303, 0, 0)
        wire += s["wire"]
    bufs = [ta.DeviceBuffer(engine, n) for n in (len(wire) + 64, descs.nbytes, 32 * max_records,
                                                 4 * max_records, 32 * len(streams), 4)]
    d_wire, d_streams, d_recs, d_status, d_results, d_total = bufs
    d_wire.upload(bytes(wire) + bytes(64))
    d_streams.upload(descs.view(np.uint8))
    d_status.upload(np.full(max_records, SENTINEL, dtype=np.uint32).view(np.uint8))
    ta.open_wire(table, d_streams.ptr, len(streams), d_wire.ptr, max_records, d_recs.ptr,
                 d_status.ptr, d_results.ptr, d_total.ptr)
    engine.sync()
    got = dict(wire=d_wire.download()[:len(wire)].tobytes(), offs=offs,
               status=d_status.download().view(np.int32)[:max_records].copy(),
               results=d_results.download().view(ta.WIRE_RESULT_DTYPE).copy(),
               total=int(d_total.download().view(np.uint32)[0]),
               recs=d_recs.download().view(ta.RECORD_DTYPE)[:max_records].copy())
    for b in bufs:
        b.free()
    return got


def _model_stream(aead, ctx, iv, s):
    """RFC 8446 5.1-5.4 over one stream as include/tlsgpu.h states it ->
    ([(status, region)], consumed, alert, alert_record, delivered)."""
    wire, framed, pos, alert = s["wire"], [], 0, 0
    while pos + 5 <= len(wire):
        rtype, ver, ln = wire[pos], (wire[pos + 1] << 8) | wire[pos + 2], (wire[pos + 3] << 8) | wire[pos + 4]
        if ver != 0x0303:
            alert = 70
            break
        if rtype != 23:
            alert = 10
            break
        if pos + 5 + ln > len(wire):
            break
        if ln > t13.MAX_FRAGMENT:
            alert = 22
            break
        framed.append((pos, ln))
        pos += 5 + ln
    out, dead, alert_rec, delivered = [], False, len(framed), len(framed)
    for i, (p, ln) in enumerate(framed):
        if dead:
            out.append((t13.SKIPPED, None))
            continue
        st, region = t13.open_fragment(aead, ctx, iv, s["seq"] + i, bytes(wire[p + 5:p + 5 + ln]))
        a = {t13.BAD_MAC: 20, t13.PUBLIC_INVALID: 21, t13.NO_CONTENT_TYPE: 10}.get(st, 0)
        if st > t13.MAX_PLAIN:
            st, a = t13.OVERFLOW, 22
        out.append((st, region))
        if a:
            dead, alert, alert_rec, delivered = True, a, i, i
    return out, pos, alert, alert_rec, delivered


def _check_open_wire(ta, aead, keys, streams, got):
    total = 0
    for i, s in enumerate(streams):
        ctx, iv = keys[s["session"]]
        recs, consumed, alert, alert_rec, delivered = _model_stream(aead, ctx, iv, s)
        r = got["results"][i]
        assert (int(r["records"]), int(r["consumed"]), int(r["alert"]), int(r["delivered"]),
                int(r["alert_record"])) == (len(recs), consumed, alert, delivered, alert_rec), (i, r)
        total += len(recs)
        pos = 0
        for k, (st, region) in enumerate(recs):
            idx = int(r["first"]) + k
            assert int(got["status"][idx]) == st, (i, k, int(got["status"][idx]), st)
            d = got["recs"][idx]
            ln = int(d["len_type"]) & 0xFFFFFF
            frag_off = got["offs"][i] + pos + 5
            assert int(d["in_off"]) == frag_off == int(d["out_off"])
            assert int(d["seq"]) == s["seq"] + k and int(d["session"]) == s["session"]
            if st >= 0:      # delivered: the content, and the inner type in the descriptor
                assert got["wire"][frag_off:frag_off + len(region)] == region, (i, k)
                assert int(d["len_type"]) >> 24 == region[st], (i, k)
            elif st in (t13.BAD_MAC, t13.NO_CONTENT_TYPE, t13.OVERFLOW):
                assert got["wire"][frag_off:frag_off + len(region)] == region, (i, k)
                assert int(d["len_type"]) >> 24 == 23
            pos += 5 + ln
    assert got["total"] == total


def test_open_wire_fixture_streams(ta, engine, aead):
    """The captured OpenSSL connection, each direction one stream (and once
    more from its third record, at another alignment): contents, inner types
    (the server's NewSessionTickets are handshake records), consumed."""
    fx = t13.load_fixture()
    kind = t13.SUITES[fx["suite"]][0]
    dirs = fx["directions"]
    table = ta.SessionTable(engine, len(dirs))
    table.install(0, [ta.SessionParams(kind, d["key"], d["iv"], version=t13.VERSION) for d in dirs])
    keys = [(aead.aead(kind, d["key"]), d["iv"]) for d in dirs]
    streams = []
    for sid, d in enumerate(dirs):
        wires = [r["wire"] for r in d["records"]]
        streams.append(dict(wire=b"".join(wires), seq=0, session=sid))
        streams.append(dict(wire=b"".join(wires[2:]) + wires[0][:9], seq=2, session=sid, shift=7))
    got = _run_open_wire(ta, engine, table, streams, 64)
    _check_open_wire(ta, aead, keys, streams, got)
    for sid, d in enumerate(dirs):
        r = got["results"][2 * sid]
        assert int(r["alert"]) == 0 and int(r["records"]) == len(d["records"]) == int(r["delivered"])
        for k, rec in enumerate(d["records"]):
            idx = int(r["first"]) + k
            o = int(got["recs"][idx]["out_off"])
            assert int(got["status"][idx]) == len(rec["content"])
            assert got["wire"][o:o + len(rec["content"])] == rec["content"]
            assert int(got["recs"][idx]["len_type"]) >> 24 == rec["inner_type"]
    table.close()


def test_open_wire_failures(ta, engine, aead):
    """Header and inner-plaintext failures end a stream with the RFC's alert;
    later records are SKIPPED; a cut last record is left for the next call."""
    rng = np.random.default_rng(5)
    kind = po.AES_128_GCM
    key, iv = rng.bytes(16), rng.bytes(12)
    ctx = aead.aead(kind, key)
    table = ta.SessionTable(engine, 1)
    table.install(0, [ta.SessionParams(kind, key, iv, version=t13.VERSION)])

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
    S.append(stream([rec(50, 16385), rec(51, 4)], 50))                                 # alert 22
    S.append(stream([rec(60, 64), rec(61, 65), rec(62, 900)[:400]], 60))               # cut
    S.append(stream([rec(70, 30), bytes([23, 3, 3, 0, 15]) + bytes(15), rec(72, 1)], 70))   # alert 21
    tampered = bytearray(rec(81, 700, 23, 17))
    tampered[300] ^= 2
    S.append(stream([rec(80, 5), bytes(tampered), rec(82, 5)], 80))                    # alert 20
    S.append(stream([rec(90 + i, 33 + i % 3) for i in range(150)], 90))                # bulk-accepted run
    got = _run_open_wire(ta, engine, table, S, 256)
    _check_open_wire(ta, aead, [(ctx, iv)], S, got)
    alerts = [int(r["alert"]) for r in got["results"]]
    assert alerts == [0, 10, 22, 10, 10, 22, 0, 21, 20, 0]
    assert [int(r["delivered"]) for r in got["results"]] == [4, 2, 1, 1, 1, 0, 2, 1, 1, 150]
    r = got["results"][3]
    st = got["status"][int(r["first"]):int(r["first"]) + 4].tolist()
    assert st == [1, ta.REC_NO_CONTENT_TYPE, ta.REC_SKIPPED, ta.REC_SKIPPED]
    r = got["results"][5]
    assert got["status"][int(r["first"]):int(r["first"]) + 2].tolist() == [ta.REC_OVERFLOW,
                                                                         ta.REC_SKIPPED]
    table.close()


def test_seal_wire_reproduces_the_captured_wire(ta, engine):
    """Every write of the captured connection (and the server's tickets, inner
    type 22) through tlsgpu_seal_wire: byte-identical records, next_seq and
    wire_len of that framing, tlsgpu_seal_wire_size_v."""
    fx = t13.load_fixture()
    kind = t13.SUITES[fx["suite"]][0]
    dirs = fx["directions"]
    table = ta.SessionTable(engine, len(dirs))
    table.install(0, [ta.SessionParams(kind, d["key"], d["iv"], version=t13.VERSION) for d in dirs])
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
        size = ta.seal_wire_size(kind, len(content), 0, 0, version=t13.VERSION)
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

def _pinned(engine, nbytes, keep):
    p = C.c_void_p()
    assert engine.lib.tlsgpu_host_alloc(engine.handle, max(nbytes, 1), C.byref(p)) == 0
    keep.append(p.value)
    return p.value


def test_host_seal_open_and_delivery(ta, engine, aead):
    """tlsgpu_seal_host and tlsgpu_open_host on one ascending batch of about
    4 MiB, pipelined in many chunks, then tlsgpu_open_batch + tlsgpu_deliver_host
    with a read hook: the hook sees every record's content (status bytes)."""
    rng = np.random.default_rng(91)
    params = _params(ta, "aes-256-gcm", 91)
    ctxs = [aead.aead(p.aead, p.key) for p in params]
    table = ta.SessionTable(engine, NSESS)
    table.install(0, params)
    lens = [LENS[i % len(LENS)] for i in range(900)] + [16384] * 60 + [991, 992, 0, 1]
    recs, ip, op = [], 0, 0
    for i, n in enumerate(lens):
        sid, seq, itype = (i // 9) % NSESS, 5000 + i, 21 + i % 3
        content = rng.bytes(n)
        ip += (-ip) % 16 + (i % 4)
        op += (-op) % 16 + (i % 3)
        recs.append((sid, seq, itype, content, ip, op,
                     t13.seal(aead, ctxs[sid], params[sid].fixed_iv, seq, itype, content)))
        ip += n + 2
        op += n + 17 + 2
    keep = []
    in_bytes, out_bytes, n = ip, op, len(recs)      # the last content ends h_in
    h_in, h_out, h_back = (_pinned(engine, b, keep) for b in (in_bytes, out_bytes, out_bytes))
    h_recs, h_status = _pinned(engine, 32 * n, keep), _pinned(engine, 4 * n, keep)
    C.memset(h_in, 0xC3, in_bytes)
    descs = np.zeros(n, dtype=ta.RECORD_DTYPE)
    for i, (sid, seq, itype, content, io, oo, frag) in enumerate(recs):
        C.memmove(h_in + io, content, len(content))
        descs[i] = (io, oo, seq, sid, ta.len_type(len(content), itype))
    C.memmove(h_recs, descs.tobytes(), descs.nbytes)
    seen = []

    def on_read(ssl, data, plen):
        seen.append(C.string_at(data, plen[0]))

    ta.host_pipeline(engine, 4, 256 << 10)
    try:
        ta.seal_host(table, h_recs, n, h_in, in_bytes - 2, h_out, out_bytes, h_status)
        st = np.ctypeslib.as_array((C.c_int32 * n).from_address(h_status)).copy()
        for i, (sid, seq, itype, content, io, oo, frag) in enumerate(recs):
            assert st[i] == len(content) + 17 and C.string_at(h_out + oo, len(frag)) == frag, i
        # open in place in a copy of the sealed buffer; padding makes no difference to the spans
        C.memmove(h_back, h_out, out_bytes)
        for i, (sid, seq, itype, content, io, oo, frag) in enumerate(recs):
            descs[i] = (oo, oo, seq, sid, ta.len_type(len(frag), 23))
        C.memmove(h_recs, descs.tobytes(), descs.nbytes)
        cbs = ta.talos_register(on_read, None)
        try:
            ta.open_host(table, h_recs, n, h_back, out_bytes, h_back, out_bytes, h_status)
        finally:
            ta.talos_register(None, None)
            del cbs
        st = np.ctypeslib.as_array((C.c_int32 * n).from_address(h_status)).copy()
        for i, (sid, seq, itype, content, io, oo, frag) in enumerate(recs):
            assert st[i] == len(content), (i, st[i])
            assert C.string_at(h_back + oo, len(content) + 1) == content + bytes([itype]), i
        assert seen == [r[3] for r in recs]
        # device-resident open, then host delivery with the hook
        del seen[:]
        d_buf = ta.DeviceBuffer(engine, out_bytes)
        d_recs, d_st = ta.DeviceBuffer(engine, 32 * n), ta.DeviceBuffer(engine, 4 * n)
        ta.load_library().tlsgpu_memcpy(engine.handle, d_buf.ptr, h_out, out_bytes, None)
        d_recs.upload(descs.view(np.uint8))
        ta.open_batch(table, d_recs.ptr, n, d_buf.ptr, out_bytes, d_buf.ptr, out_bytes, d_st.ptr)
        C.memset(h_back, 0, out_bytes)
        cbs = ta.talos_register(on_read, None)
        try:
            ta.deliver_host(table, d_recs.ptr, d_st.ptr, n, d_buf.ptr, out_bytes, h_back, h_status)
        finally:
            ta.talos_register(None, None)
            del cbs
        st = np.ctypeslib.as_array((C.c_int32 * n).from_address(h_status)).copy()
        assert st.tolist() == [len(r[3]) for r in recs]
        assert seen == [r[3] for r in recs]
        for b in (d_buf, d_recs, d_st):
            b.free()
    finally:
        ta.host_pipeline(engine, 2, 32 << 20)
        for p in keep:
            engine.lib.tlsgpu_host_free(engine.handle, p)
        table.close()
