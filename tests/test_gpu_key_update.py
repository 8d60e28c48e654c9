"""The device key schedule on the GPU (include/tlsgpu.h:
tlsgpu_sessions_install_secrets, tlsgpu_sessions_key_update,
tlsgpu_wire_key_update_ids).

Every comparison is exact.  The reference for a derived value is Python's
hmac / hashlib through tls13_helper.hkdf_expand_label and
wire_key_update_model (next_generation, keys_of, SUITES); the reference for a
slot's bytes is a second table given a plain tlsgpu_sessions_install of the
Python-derived key and IV, read back with tlsgpu_sessions_debug_read.  A slot is
compared over the bytes an install writes: its DevSession, and for AES-GCM its
GHASH tables and the bitsliced masks of its rounds + 1 round keys (an install
writes no table bytes for ChaCha20-Poly1305 and none of the masks beyond its
rounds, and the table memory is not cleared at creation).  "Unchanged" slots
are compared over all their bytes."""
import ctypes as C
import os

import numpy as np
import pytest

import pyoracle as po
import tls13_helper as t13
import wire_key_update_model as ku

pytestmark = pytest.mark.gpu

ORDER = ["aes128", "aes256", "chacha"]
ENGINE_KIND = {"aes128": 1, "aes256": 2, "chacha": 5}
HASHLEN = {"aes128": 32, "aes256": 48, "chacha": 32}
IMG = 1024 + 2048 + 65 * 256 + 15 * 512      # DevSession + DevGcmTables
SECRET_LEN_OFF, SECRET_OFF, SECRET_END = 580, 584, 632
OK, SKIPPED, EINVAL, ERANGE = 0, 1, -1, -4
NONE = 0xFFFFFFFF


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


def used_bytes(suite):
    """The bytes of a slot an install of this suite writes."""
    if suite == "chacha":
        return 1024
    rounds = 10 if suite == "aes128" else 14
    return 1024 + 2048 + 65 * 256 + 512 * (rounds + 1)


def read_slot(ta, table, slot):
    buf = (C.c_uint8 * IMG)()
    assert ta.load_library().tlsgpu_sessions_debug_read(table.handle, slot, buf, IMG) == 0
    return bytes(buf)


def snapshot(ta, table, slots):
    return {s: read_slot(ta, table, s) for s in slots}


def key_params(ta, suite, secret, pad=0):
    """What the host route installs for a secret: the Python-derived key and IV."""
    _, key_len, hashname = ku.SUITES[suite]
    key, iv = ku.keys_of(secret, key_len, hashname)
    return ta.SessionParams(ENGINE_KIND[suite], key, iv, version=t13.VERSION, pad_block=pad)


def with_secret(img, secret):
    """A key install's image with the secret fields of a secret install."""
    assert img[SECRET_LEN_OFF:SECRET_END] == bytes(SECRET_END - SECRET_LEN_OFF)
    b = bytearray(img)
    b[SECRET_LEN_OFF:SECRET_OFF] = len(secret).to_bytes(4, "little")
    b[SECRET_OFF:SECRET_OFF + len(secret)] = secret
    return bytes(b)


def reference_images(ta, engine, specs):
    """{slot: image} of a fresh table given tlsgpu_sessions_install for
    specs = {slot: (suite, secret, pad)}, the secret fields patched in."""
    if not specs:
        return {}
    slots = sorted(specs)
    ref = ta.SessionTable(engine, len(slots))
    ref.install(0, [key_params(ta, *specs[s]) for s in slots])
    out = {s: with_secret(read_slot(ta, ref, k), specs[s][1]) for k, s in enumerate(slots)}
    ref.close()
    return out


def next_secret(suite, secret):
    return ku.next_generation(secret, ku.SUITES[suite][2])


def layout(n, seed):
    """n sessions, the suites interleaved so that SHA-256 and SHA-384 lanes share
    a wave, each suite with pad_block 0 and 512: {slot: (suite, secret, pad)}."""
    rng = np.random.default_rng(seed)
    return {i: (ORDER[i % 3], rng.bytes(HASHLEN[ORDER[i % 3]]), 512 if (i // 3) % 2 else 0)
            for i in range(n)}


def secret_params(ta, spec):
    suite, secret, pad = spec
    return ta.SecretParams(ENGINE_KIND[suite], secret, pad_block=pad)


def run_key_update(ta, engine, table, ids, stream=None):
    """One tlsgpu_sessions_key_update over a host id list -> statuses."""
    ids = np.asarray(ids, dtype=np.uint32)
    d_ids, d_st = ta.DeviceBuffer(engine, ids.nbytes), ta.DeviceBuffer(engine, 4 * len(ids))
    d_ids.upload(ids.view(np.uint8))
    d_st.fill(0x5A)
    table.key_update(d_ids.ptr, len(ids), d_st.ptr, stream)
    engine.sync_stream(stream)
    st = d_st.download().view(np.int32).copy()
    d_ids.free()
    d_st.free()
    return [int(x) for x in st]


def test_install_image(ta, engine):
    """130 sessions in one call, three suites, pad_block 0 and 512."""
    specs = layout(130, 1)
    assert {(s, p) for s, _, p in specs.values()} == {(s, p) for s in ORDER for p in (0, 512)}
    table = ta.SessionTable(engine, 130)
    table.install_secrets(0, [secret_params(ta, specs[i]) for i in range(130)])
    want = reference_images(ta, engine, specs)      # also: the key install's secret fields are zero
    for i in range(130):
        suite, secret, _ = specs[i]
        got, n = read_slot(ta, table, i), used_bytes(suite)
        assert got[SECRET_LEN_OFF:SECRET_OFF] == len(secret).to_bytes(4, "little"), i
        assert got[SECRET_OFF:SECRET_END] == secret + bytes(48 - len(secret)), i
        assert got[:n] == want[i][:n], (i, suite)
    table.close()


CAP = 140               # slots 0..129 from secrets, 130..139 as tlsgpu_sessions_create leaves them
KEY_SLOT, EMPTY_SLOT, TRIPLE = 5, 135, 17


def id_list(length, gen):
    """An id list of `length`.  From 63 on it holds, beside distinct secret slots:
    TLSGPU_SESSION_NONE entries, two ids >= capacity, the key-installed slot,
    an empty slot, and one slot three times: in the first entry, in the middle
    and in the last entry (lane 63 of the first wave, or a lane of another wave)."""
    if length == 1:
        return [40 + gen]
    ids = [NONE] * length
    fixed = {0: TRIPLE, 1: CAP, 2: KEY_SLOT, 3: EMPTY_SLOT, 4: 0xFFFFFFFE, length // 2: TRIPLE,
             length - 1: TRIPLE}
    pool = [s for s in range(130) if s not in (KEY_SLOT, TRIPLE)]
    for k in range(length):
        if k in fixed:
            ids[k] = fixed[k]
        elif k % 5 != 0:            # every fifth entry stays TLSGPU_SESSION_NONE
            ids[k] = pool[(k * 7 + gen) % len(pool)] if length < 130 else pool[k % len(pool)]
    return ids


@pytest.mark.parametrize("length", [1, 63, 64, 65, 130])
def test_update_image(ta, engine, length):
    """Three generations in a row; the lane and wave boundaries of the derive kernel."""
    specs = layout(130, 2)
    table = ta.SessionTable(engine, CAP)
    table.install_secrets(0, [secret_params(ta, specs[i]) for i in range(130)])
    # a plain install over a secret slot: a key-installed slot from here on
    table.install(KEY_SLOT, [key_params(ta, *specs[KEY_SLOT])])
    secrets = {s: specs[s][1] for s in range(130) if s != KEY_SLOT}
    before = snapshot(ta, table, range(CAP))
    for gen in range(3):
        ids = id_list(length, gen)
        st = run_key_update(ta, engine, table, ids)
        listed = set()
        for k, (i, s) in enumerate(zip(ids, st)):
            if i == NONE:
                assert s == SKIPPED, (k, s)
            elif i >= CAP:
                assert s == ERANGE, (k, i, s)
            elif i in (KEY_SLOT, EMPTY_SLOT):
                assert s == EINVAL, (k, i, s)
            else:
                assert s == OK, (k, i, s)
                listed.add(i)
        if length > 1:
            assert ids.count(TRIPLE) == 3 and NONE in ids and len(listed) > length // 2
        for s in listed:            # ONE generation on, however often the id was listed
            secrets[s] = next_secret(specs[s][0], secrets[s])
        want = reference_images(ta, engine,
                                {s: (specs[s][0], secrets[s], specs[s][2]) for s in listed})
        after = snapshot(ta, table, range(CAP))
        for s in range(CAP):
            if s in listed:
                n = used_bytes(specs[s][0])
                assert after[s][:n] == want[s][:n], (gen, s)
                assert after[s][n:] == before[s][n:], (gen, s)
            else:
                assert after[s] == before[s], (gen, s, "an unlisted slot changed")
        before = after
    table.close()


def test_update_in_chunks_and_a_duplicate_across_them(ta, engine):
    """A list longer than the table's scratch runs in chunks; an id listed in two
    chunks is still rekeyed once."""
    specs = layout(6, 3)
    table = ta.SessionTable(engine, 6)
    table.install_secrets(0, [secret_params(ta, specs[i]) for i in range(6)])
    before = snapshot(ta, table, range(6))
    n = 65536 + 70
    ids = [NONE] * n
    ids[0], ids[65535], ids[65536], ids[65536 + 5], ids[n - 1] = 3, 4, 1, 3, 4
    st = run_key_update(ta, engine, table, ids)
    assert [st[k] for k in (0, 65535, 65536, 65536 + 5, n - 1)] == [OK] * 5
    assert st.count(SKIPPED) == n - 5
    want = reference_images(ta, engine, {s: (specs[s][0], next_secret(*specs[s][:2]), specs[s][2])
                                         for s in (1, 3, 4)})
    for s in range(6):
        got = read_slot(ta, table, s)
        if s in want:
            assert got[:used_bytes(specs[s][0])] == want[s][:used_bytes(specs[s][0])], s
        else:
            assert got == before[s], s
    table.close()


@pytest.mark.parametrize("suite", ORDER)
def test_ciphers_see_the_new_keys(ta, engine, aead, suite):
    from talos_amd.batch import RecordBatch
    kind = ENGINE_KIND[suite]
    secret = np.random.default_rng(4).bytes(HASHLEN[suite])
    old = ku.Generation(aead, suite, secret)
    new = old.next()
    table = ta.SessionTable(engine, 2)
    table.install_secrets(1, [ta.SecretParams(kind, secret)])
    assert run_key_update(ta, engine, table, [1]) == [OK]
    content = bytes(range(200)) * 3
    # seal with seq 0 under generation N + 1
    sb = RecordBatch(engine, [(1, 0, 23, content, kind)], "seal", tls13=True)
    sb.run(table)
    want = t13.seal(aead, new.ctx, new.iv, 0, 23, content)
    assert sb.results() == [(len(want), want)]
    # open the oracle's records: generation N + 1 opens, generation N fails its tag
    theirs = t13.seal(aead, new.ctx, new.iv, 1, 23, content)
    stale = t13.seal(aead, old.ctx, old.iv, 1, 23, content)
    ob = RecordBatch(engine, [(1, 1, 23, theirs, kind), (1, 1, 23, stale, kind)], "open", tls13=True)
    ob.run(table)
    (st_new, pt_new), (st_old, pt_old) = ob.results()
    assert (st_new, pt_new) == (len(content), content)
    assert st_old == ta.REC_BAD_MAC and pt_old == bytes(len(stale) - 16)
    for b in (sb, ob):
        b.free()
    table.close()


def short(i):
    return bytes((7 * i + j) & 0xFF for j in range(1 + i % 9))


LOOKALIKE = bytes([0x18, 0, 0, 1, 0, 22]) + bytes(10) + b"tail"   # application data, not a KeyUpdate
N_STREAMS, NO_KU, HELD = 65, 7, 13


@pytest.mark.parametrize("suite", ORDER)
def test_wire_loop_without_a_host_install(ta, engine, aead, suite):
    """open_wire -> wire_key_update_ids -> key_update on one stream, then the
    second open_wire built from `consumed`: no install from the host."""
    rng = np.random.default_rng(5)
    kind = ENGINE_KIND[suite]
    gens = [ku.Generation(aead, suite, rng.bytes(HASHLEN[suite])) for _ in range(N_STREAMS)]
    table = ta.SessionTable(engine, N_STREAMS)
    table.install_secrets(0, [ta.SecretParams(kind, g.secret) for g in gens])
    ta.sessions_wire_key_update(table, True)
    # the streams: [first call's records], [second call's records], contents of the second
    image, streams = bytearray(b"\xC3" * 16), []
    for i, g in enumerate(gens):
        seq = 3 + i
        if i == NO_KU:
            first = [g.rec(seq, short(0)), g.rec(seq + 1, short(1))]
            rest_c = [short(2), short(3)]
            rest = [g.rec(seq + 2 + k, c) for k, c in enumerate(rest_c)]
        elif i == HELD:
            first = [g.rec(seq, short(0)), g.rec(seq + 1, LOOKALIKE)]
            rest_c = [short(4), short(5)]
            rest = [g.rec(seq + 2 + k, c) for k, c in enumerate(rest_c)]
        else:
            nxt = g.next()
            first = [g.rec(seq, short(i)), g.rec(seq + 1, short(i + 1)), g.key_update(seq + 2, i & 1)]
            rest_c = [short(i + 2), short(i + 3), short(i + 4)]
            rest = [nxt.rec(k, c) for k, c in enumerate(rest_c)]
        whole = b"".join(first + rest)
        # the read-ahead holds everything, except for the stream without a KeyUpdate
        seen = len(b"".join(first)) if i == NO_KU else len(whole)
        streams.append(dict(off=len(image), seq=seq, first=first, rest=rest, rest_c=rest_c,
                            cut=len(b"".join(first)), seen=seen, total=len(whole)))
        image += whole + b"\xC3" * 16
    max_records = 6 * N_STREAMS
    d_wire = ta.DeviceBuffer(engine, len(image))
    d_wire.upload(bytes(image))
    d_streams, d_results, d_recs, d_status, d_total, d_ids, d_kst = (
        ta.DeviceBuffer(engine, n) for n in (32 * N_STREAMS, 32 * N_STREAMS, 32 * max_records,
                                             4 * max_records, 4, 4 * N_STREAMS, 4 * N_STREAMS))

    def open_wire(spans):
        descs = np.zeros(N_STREAMS, dtype=ta.WIRE_STREAM_DTYPE)
        for i, (off, length, seq) in enumerate(spans):
            descs[i] = (off, length, i, seq, 0x0303, 0, 0)
        d_streams.upload(descs.view(np.uint8))
        ta.open_wire(table, d_streams.ptr, N_STREAMS, d_wire.ptr, max_records, d_recs.ptr,
                     d_status.ptr, d_results.ptr, d_total.ptr)

    untouched = snapshot(ta, table, (NO_KU, HELD))
    d_ids.fill(0x5A)
    d_kst.fill(0x5A)
    # the first round, queued on the engine's stream with nothing read in between
    open_wire([(s["off"], s["seen"], s["seq"]) for s in streams])
    table.wire_key_update_ids(d_streams.ptr, d_results.ptr, N_STREAMS, d_ids.ptr)
    table.key_update(d_ids.ptr, N_STREAMS, d_kst.ptr)
    engine.sync()
    res = d_results.download().view(ta.WIRE_RESULT_KU_DTYPE).copy()
    ids = d_ids.download().view(np.uint32)
    kst = d_kst.download().view(np.int32)
    spans = []
    for i, s in enumerate(streams):
        r = res[i]
        assert (int(r["records"]), int(r["delivered"]), int(r["consumed"]), int(r["alert"])) == \
            (len(s["first"]), len(s["first"]), s["cut"], 0), i
        if i == NO_KU:
            want_ku = ta.WIRE_KU_NONE
        elif i == HELD:
            want_ku = ta.WIRE_KU_HELD
        else:
            want_ku = ta.WIRE_KU_UPDATE + (i & 1)
        assert int(r["key_update"]) == want_ku, i
        updated = want_ku in (ta.WIRE_KU_UPDATE, ta.WIRE_KU_UPDATE_REQUESTED)
        assert int(ids[i]) == (i if updated else NONE), i
        assert int(kst[i]) == (OK if updated else SKIPPED), i
        # the next call, from what the first one reported
        spans.append((s["off"] + int(r["consumed"]), s["total"] - int(r["consumed"]),
                      0 if updated else s["seq"] + int(r["records"])))
    # the slots: the two that saw no KeyUpdate as they were, the others one generation on
    assert snapshot(ta, table, (NO_KU, HELD)) == untouched
    want = reference_images(ta, engine, {i: (suite, g.next().secret, 0)
                                         for i, g in enumerate(gens) if i not in (NO_KU, HELD)})
    for i in want:
        assert read_slot(ta, table, i)[:used_bytes(suite)] == want[i][:used_bytes(suite)], i
    # the second round delivers every record, and the gather exactly the application bytes
    open_wire(spans)
    reads = np.zeros(N_STREAMS, dtype=ta.READ_STREAM_DTYPE)
    for i in range(N_STREAMS):
        reads[i] = (64 * i, 64, 0)
    d_reads, d_app, d_out = (ta.DeviceBuffer(engine, n) for n in (reads.nbytes, 64 * N_STREAMS,
                                                                 32 * N_STREAMS))
    d_reads.upload(reads.view(np.uint8))
    d_app.fill(0xEE)
    ta.gather_wire(table, d_streams.ptr, d_results.ptr, N_STREAMS, d_recs.ptr, d_status.ptr,
                   max_records, d_wire.ptr, len(image), d_reads.ptr, d_app.ptr, 64 * N_STREAMS,
                   d_out.ptr)
    engine.sync()
    res = d_results.download().view(ta.WIRE_RESULT_KU_DTYPE).copy()
    out = d_out.download().view(ta.READ_RESULT_DTYPE).copy()
    app = d_app.download().tobytes()
    for i, s in enumerate(streams):
        r, n = res[i], len(s["rest"])
        assert (int(r["records"]), int(r["delivered"]), int(r["consumed"]), int(r["alert"]),
                int(r["key_update"])) == (n, n, s["total"] - s["cut"], 0, ta.WIRE_KU_NONE), i
        data = b"".join(s["rest_c"])
        assert (int(out[i]["app_len"]), int(out[i]["records"]), int(out[i]["stop"])) == \
            (len(data), n, ta.READ_END), i
        assert app[64 * i:64 * (i + 1)] == data + b"\xEE" * (64 - len(data)), i
    assert snapshot(ta, table, (NO_KU, HELD)) == untouched
    for b in (d_wire, d_streams, d_results, d_recs, d_status, d_total, d_ids, d_kst, d_reads, d_app,
              d_out):
        b.free()
    table.close()


def test_a_plain_install_clears_the_secret(ta, engine):
    specs = layout(3, 6)
    table = ta.SessionTable(engine, 3)
    table.install_secrets(0, [secret_params(ta, specs[i]) for i in range(3)])
    table.install(1, [key_params(ta, *specs[1])])
    ref = ta.SessionTable(engine, 1)
    ref.install(0, [key_params(ta, *specs[1])])
    got, want, n = read_slot(ta, table, 1), read_slot(ta, ref, 0), used_bytes(specs[1][0])
    assert got[SECRET_LEN_OFF:SECRET_END] == bytes(SECRET_END - SECRET_LEN_OFF)
    assert got[:n] == want[:n]
    before = snapshot(ta, table, range(3))
    assert run_key_update(ta, engine, table, [1]) == [EINVAL]
    assert snapshot(ta, table, range(3)) == before
    # a table no secret was ever installed into: the same answers, nothing written
    before = read_slot(ta, ref, 0)
    assert run_key_update(ta, engine, ref, [0, NONE, 1, 0]) == [EINVAL, SKIPPED, ERANGE, EINVAL]
    assert read_slot(ta, ref, 0) == before
    ref.close()
    table.close()
