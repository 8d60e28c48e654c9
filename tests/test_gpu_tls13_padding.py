"""TLS 1.3 record padding on seal (tlsgpu_session_params.pad_block) on the GPU,
the AES-GCM kernels: batch, split, ttable, wire and host paths against
tests/tls13_padding.py (the block rule over tests/tls13_helper.py and the
oracle's AEAD, or the reference's where oracle/_ref is built; the rule and the
framing are checked against an OpenSSL capture in test_tls13_padding.py).

Conventions of test_gpu_tls13.py: output and status buffers start from a
sentinel, the whole output image is compared, every batch runs twice, d_in is
0xC3 around every content (a byte read past the content shows), and every buffer
is sized from the Python model, never from the engine's answer.

One table holds six sessions with pad_block 0, 16, 64, 512, 4096 and 16384, so
mixed policies and "off" sit in one batch.  Lengths per session: 0, 1, 14-17
(type byte last in a block, alone in one, second in one, then zero blocks);
B - 2 .. B + 1 and 2B - 1 (inner == B exactly, and one byte more: pad B - 1); 991 /
992 (the pack boundary reached by padding with B = 16), 1007 .. 1024, 2047 /
2048, 4095 .. 4097 (a source that ends in the first step of a record of 2, 4 and
16 steps: len 1 and 4097 with B = 4096 / 16384), 16382 .. 16384; 16400 and 48000
in the B = 512 session (never padded).
"""
import ctypes as C
import os

import numpy as np
import pytest

import pyoracle as po
import tls13_helper as t13
import tls13_padding as tp

pytestmark = pytest.mark.gpu

KINDS = {"aes-128-gcm": po.AES_128_GCM, "aes-256-gcm": po.AES_256_GCM}
BLOCKS = [0, 16, 64, 512, 4096, 16384]
COMMON = [0, 1, 14, 15, 16, 17, 991, 992, 1007, 1008, 1023, 1024, 2047, 2048, 4095, 4096, 4097,
          16382, 16383, 16384]
VARIANTS = [3, 0, 2]
SENTINEL = 0x5A5A5A5A


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


@pytest.fixture
def impl(ta, request):
    prev = ta.get_gcm_impl()
    ta.set_gcm_impl(getattr(request, "param", "queue"))
    yield
    ta.set_gcm_impl(prev)


def session_lengths(block):
    ls = set(COMMON)
    if block > 1:
        ls |= {block - 2, block - 1, block, block + 1, 2 * block - 1}
    return sorted(n for n in ls if 0 <= n <= 16384)


def make_sessions(ta, aead, kinds, blocks, seed, oracle_kind=None):
    """[(SessionParams, oracle ctx, pad_block)]"""
    rng = np.random.default_rng(seed)
    out = []
    for k, b in zip(kinds, blocks):
        p = ta.SessionParams(k, rng.bytes(ta.KEY_LEN[k]), rng.bytes(12), version=t13.VERSION,
                             pad_block=b)
        out.append((p, aead.aead((oracle_kind or {}).get(k, k), p.key), b))
    return out


_cache = {}


def material(aead, sessions, key, plan):
    """plan: [(session, inner type, content length)] -> per record the content and
    the model's fragment, computed once per key."""
    if key not in _cache:
        rng = np.random.default_rng(len(plan))
        recs = []
        for i, (sid, itype, n) in enumerate(plan):
            seq = (1 << 33) + 1000 + i          # both nonce words carry sequence bits
            content = rng.bytes(n)
            p, ctx, block = sessions[sid]
            frag = tp.seal(aead, ctx, p.fixed_iv, seq, itype, content, block)
            assert len(frag) == tp.inner_len(n, block) + 16
            recs.append(dict(sid=sid, seq=seq, itype=itype, content=content, frag=frag))
        _cache[key] = recs
    return _cache[key]


def run_seal(ta, engine, aead, sessions, key, plan, hints=None, in_shifts=None, out_shifts=None,
             cut_last=False, round_trip=False):
    """One table of `sessions`, one seal batch laid out here: slot i at a 16-byte
    boundary + its shift, 3 bytes apart, d_in 0xC3 and d_out 0xA5.  cut_last: d_out
    ends where the last record's UNPADDED fragment would end (that record is out
    of bounds if its session pads it).  round_trip: the sealed image is then opened
    in place."""
    recs = material(aead, sessions, key, plan)
    n = len(recs)
    table = ta.SessionTable(engine, len(sessions))
    table.install(0, [s[0] for s in sessions])
    if hints is not None:
        table.hint(hints)
    descs = np.zeros(n, dtype=ta.RECORD_DTYPE)
    ip = op = 0
    for i, r in enumerate(recs):
        ip += (-ip) % 16 + (in_shifts[i] if in_shifts else 0)
        op += (-op) % 16 + (out_shifts[i] if out_shifts else 0)
        descs[i] = (ip, op, r["seq"], r["sid"], ta.len_type(len(r["content"]), r["itype"]))
        ip += len(r["content"]) + 3
        op += len(r["frag"]) + 3
    in_bytes = max(ip - 3, 1)                       # the last content ends d_in
    out_offs = [int(d["out_off"]) for d in descs]
    out_bytes = out_offs[-1] + len(recs[-1]["content"]) + 17 if cut_last else op + 16
    host_in = np.full(in_bytes, 0xC3, dtype=np.uint8)
    for d, r in zip(descs, recs):
        o = int(d["in_off"])
        host_in[o:o + len(r["content"])] = np.frombuffer(r["content"], dtype=np.uint8)
    exp_out = np.full(out_bytes, 0xA5, dtype=np.uint8)
    exp_st = np.zeros(n, dtype=np.int32)
    for i, r in enumerate(recs):
        o, f = out_offs[i], r["frag"]
        if o + len(f) > out_bytes:
            assert cut_last and i == n - 1
            exp_st[i] = ta.REC_OUT_OF_BOUNDS         # and not a byte written
        else:
            exp_st[i] = len(f)
            exp_out[o:o + len(f)] = np.frombuffer(f, dtype=np.uint8)
    bufs = [ta.DeviceBuffer(engine, b) for b in (in_bytes, out_bytes + 64, descs.nbytes, 4 * n)]
    d_in, d_out, d_recs, d_status = bufs
    d_in.upload(host_in)
    d_recs.upload(descs.view(np.uint8))
    images = []
    for _ in range(2):
        d_out.fill(0xA5)
        d_status.upload(np.full(n, SENTINEL, dtype=np.uint32).view(np.uint8))
        ta.seal_batch(table, d_recs.ptr, n, d_in.ptr, in_bytes, d_out.ptr, out_bytes, d_status.ptr,
                      None)
        engine.sync()
        whole = d_out.download()
        assert (whole[out_bytes:] == 0xA5).all()          # nothing past out_bytes
        out = whole[:out_bytes].copy()
        st = d_status.download().view(np.int32)[:n].copy()
        images.append((out, st))
        bad = np.flatnonzero(st != exp_st)
        assert bad.size == 0, (key, hints, "status", bad[:8].tolist(), st[bad[:8]].tolist(),
                               exp_st[bad[:8]].tolist(), [plan[j] for j in bad[:8]])
        diff = np.flatnonzero(out != exp_out)
        if diff.size:
            rec = int(np.searchsorted(np.asarray(out_offs), diff[0], side="right")) - 1
            raise AssertionError((key, hints, "output byte", int(diff[0]), "record", rec, plan[rec],
                                  sessions[plan[rec][0]][2], int(diff[0]) - out_offs[rec]))
    assert (images[0][1] == images[1][1]).all() and (images[0][0] == images[1][0]).all()
    if round_trip:
        # open the sealed image in place: status = the content length, the type behind it
        odescs = descs.copy()
        for i, r in enumerate(recs):
            odescs[i] = (out_offs[i], out_offs[i], r["seq"], r["sid"], ta.len_type(len(r["frag"]), 23))
        d_recs.upload(odescs.view(np.uint8))
        d_status.upload(np.full(n, SENTINEL, dtype=np.uint32).view(np.uint8))
        ta.open_batch(table, d_recs.ptr, n, d_out.ptr, out_bytes, d_out.ptr, out_bytes, d_status.ptr,
                      None)
        engine.sync()
        out = d_out.download()[:out_bytes]
        st = d_status.download().view(np.int32)[:n]
        for i, r in enumerate(recs):
            o, cl = out_offs[i], len(r["content"])
            assert int(st[i]) == cl, (i, plan[i], int(st[i]))
            inner = len(r["frag"]) - 16
            assert out[o:o + inner].tobytes() == r["content"] + bytes([r["itype"]]) + \
                bytes(inner - cl - 1), (i, plan[i])
    for b in bufs:
        b.free()
    table.close()


def _sessions(ta, aead, name, seed=11):
    k = KINDS[name]
    return make_sessions(ta, aead, [k] * len(BLOCKS), BLOCKS, seed + k)


def _lengths_plan():
    """Session runs in rotation: each run is the session's lengths below 2047,
    rotated from run to run, and in every fourth round the long ones too.  The
    B = 16384 session stops at about 300 records.  More than 4,096 records, near
    10 MB of output, so workgroup ranges end inside runs and waves take several
    records."""
    plan, per_session = [], [0] * len(BLOCKS)
    run = 0
    while len(plan) <= 4200:
        sid = run % len(BLOCKS)
        rnd = run // len(BLOCKS)
        run += 1
        if BLOCKS[sid] == 16384 and per_session[sid] >= 300:
            continue
        ls = session_lengths(BLOCKS[sid])
        seq = [n for n in ls if n < 2047] + ([n for n in ls if n >= 2047] if rnd % 4 == 0 else [])
        rot = (7 * rnd) % len(seq)
        for n in seq[rot:] + seq[:rot]:
            plan.append((sid, 21 + len(plan) % 3, n))
        per_session[sid] += len(seq)
    plan += [(3, 23, 16400), (3, 22, 48000)]          # B = 512: never padded
    assert len(plan) > 4096
    for sid, b in enumerate(BLOCKS):                 # every length of every session is there
        assert {n for s, _, n in plan if s == sid} >= set(session_lengths(b))
    return plan


@pytest.mark.parametrize("shifted", [False, True])
@pytest.mark.parametrize("hints", VARIANTS)
@pytest.mark.parametrize("name", list(KINDS))
def test_padded_lengths(ta, engine, aead, impl, name, hints, shifted):
    """The queue kernel's fused no-pack variant (hints 3), the device-side
    selection (0) and the fused pack variant (2); 16-B aligned slots, and aligned
    slots alternating with byte-shifted ones.  The aligned hints-0 case also
    opens the sealed image in place."""
    plan = _lengths_plan()
    shifts = [0 if i % 2 == 0 or not shifted else 1 + (i // 2) % 15 for i in range(len(plan))]
    run_seal(ta, engine, aead, _sessions(ta, aead, name), ("lengths", name), plan, hints=hints,
             in_shifts=shifts, out_shifts=shifts[::-1] if shifted else None,
             round_trip=hints == 0 and not shifted)


@pytest.mark.parametrize("block,n", [(16, 20), (512, 100), (16384, 1), (4096, 4097)])
@pytest.mark.parametrize("hints", [3, 0])
@pytest.mark.parametrize("name", list(KINDS))
def test_output_bounds_use_the_padded_fragment(ta, engine, aead, impl, name, hints, block, n):
    """d_out ends where the last record's unpadded fragment would end: that
    record is TLSGPU_REC_OUT_OF_BOUNDS and not a byte of it is written."""
    sid = BLOCKS.index(block)
    plan = [(s % len(BLOCKS), 23, 40 + s) for s in range(600)] + [(sid, 22, n)]
    run_seal(ta, engine, aead, _sessions(ta, aead, name), ("bounds", name, block, n), plan,
             hints=hints, cut_last=True)


@pytest.mark.parametrize("impl", ["split", "ttable"], indirect=True)
@pytest.mark.parametrize("name", list(KINDS))
def test_split_and_ttable(ta, engine, aead, impl, name):
    """The split kernel: the content ends in the first, a middle and the last
    wave's range of a padded record.  And the T-table kernel through parse_tls."""
    special = [(5, 10), (5, 9000), (4, 4097), (3, 48000), (5, 16383), (5, 1023), (4, 1), (3, 511)]
    plan = [(sid, 21 + i % 3, n) for i, (sid, n) in enumerate(special)]
    i = 0
    while len(plan) < 200:
        sid = i % len(BLOCKS)
        ls = session_lengths(BLOCKS[sid])
        n = ls[(i // len(BLOCKS)) % len(ls)]
        if BLOCKS[sid] < 16384 or n < 2047:
            plan.append((sid, 21 + i % 3, n))
        i += 1
    shifts = [0 if i % 3 else i % 16 for i in range(len(plan))]
    run_seal(ta, engine, aead, _sessions(ta, aead, name), ("small", name), plan, hints=0,
             in_shifts=shifts, round_trip=True)


# -- tlsgpu_seal_wire ----------------------------------------------------------

def run_seal_wire(ta, engine, table, kind, jobs, block):
    """jobs: [(session, seq, inner type, data, max_fragment, expected wire)]"""
    data, wire_off = bytearray(), 0
    streams = np.zeros(len(jobs), dtype=ta.WRITE_STREAM_DTYPE)
    for i, (sid, seq, itype, content, frag, want) in enumerate(jobs):
        data += b"\xC3" * (1 + i % 5)          # non-zero bytes before every write
        size = tp.seal_wire_size(len(content), block, frag)
        assert size == len(want)
        assert ta.seal_wire_size(kind, len(content), frag, 0, version=t13.VERSION,
                                 pad_block=block) == size
        streams[i] = (len(data), wire_off, seq, len(content), sid, 0x0303, itype, 0, frag)
        data += content
        wire_off += size + 3
    data += b"\xC3"
    nrec = sum(len(t13.frame(j[3], j[4])) for j in jobs)
    bufs = [ta.DeviceBuffer(engine, n) for n in (len(data), wire_off + 64, streams.nbytes,
                                                 32 * nrec, 4 * nrec, 32 * len(jobs), 4)]
    d_data, d_wire, d_streams, d_recs, d_status, d_results, d_total = bufs
    d_data.upload(bytes(data))
    d_wire.fill(0xA5)
    d_streams.upload(streams.view(np.uint8))
    d_status.upload(np.full(nrec, SENTINEL, dtype=np.uint32).view(np.uint8))
    ta.seal_wire(table, d_streams.ptr, len(jobs), d_data.ptr, len(data), d_wire.ptr, wire_off + 64,
                 nrec, d_recs.ptr, d_status.ptr, d_results.ptr, d_total.ptr)
    engine.sync()
    wire = d_wire.download().tobytes()
    res = d_results.download().view(ta.WRITE_RESULT_DTYPE)
    st = d_status.download().view(np.int32)[:nrec]
    assert int(d_total.download().view(np.uint32)[0]) == nrec
    exp = bytearray(b"\xA5" * len(wire))
    for i, (sid, seq, itype, content, frag, want) in enumerate(jobs):
        o = int(streams[i]["wire_off"])
        exp[o:o + len(want)] = want
        pieces = t13.frame(content, frag)
        assert (int(res[i]["records"]), int(res[i]["wire_len"]), int(res[i]["next_seq"])) == \
            (len(pieces), len(want), seq + len(pieces)), (i, res[i])
        for k, piece in enumerate(pieces):
            assert int(st[int(res[i]["first"]) + k]) == tp.inner_len(len(piece), block) + 16
    assert wire == bytes(exp)
    for b in bufs:
        b.free()


@pytest.mark.parametrize("name", list(KINDS))
def test_seal_wire_pads_each_fragment(ta, engine, aead, name):
    kind = KINDS[name]
    (p, ctx, block), = make_sessions(ta, aead, [kind], [512], 5)
    table = ta.SessionTable(engine, 1)
    table.install(0, [p])
    rng = np.random.default_rng(9)
    jobs, seq = [], 1 << 32
    for frag in (0, 1000):
        for n in (1, 511, 512, 16383, 16384, 16385, 40000):
            data = rng.bytes(n)
            jobs.append((0, seq, 21 + len(jobs) % 3, data, frag,
                         tp.seal_wire(aead, ctx, p.fixed_iv, seq, 21 + len(jobs) % 3, data, block,
                                      frag)))
            seq += 100
    run_seal_wire(ta, engine, table, kind, jobs, block)
    table.close()


def capture_jobs(fx):
    """Every write of a captured connection (and the server's tickets, inner type
    22) as tlsgpu_seal_wire jobs."""
    jobs = []
    for sid, d in enumerate(fx["directions"]):
        app = [r for r in d["records"] if r["inner_type"] == 23]
        for r in d["records"]:
            if r["inner_type"] != 23:
                jobs.append((sid, r["seq"], r["inner_type"], r["content"], 0, r["wire"]))
        k = 0
        for w in d["writes"]:
            n = len(t13.frame(bytes(w)))
            recs = app[k:k + n]
            k += n
            jobs.append((sid, recs[0]["seq"], 23, b"".join(r["content"] for r in recs), 0,
                         b"".join(r["wire"] for r in recs)))
    return jobs


def test_seal_wire_reproduces_the_padded_capture(ta, engine):
    """Every write of the OpenSSL connection captured under RecordPadding = 512,
    byte for byte."""
    fx = t13.load_fixture(tp.GOLDEN_PADDED)
    kind, block = t13.SUITES[fx["suite"]][0], fx["record_padding"]
    dirs = fx["directions"]
    table = ta.SessionTable(engine, len(dirs))
    table.install(0, [ta.SessionParams(kind, d["key"], d["iv"], version=t13.VERSION,
                                       pad_block=block) for d in dirs])
    run_seal_wire(ta, engine, table, kind, capture_jobs(fx), block)
    table.close()


# -- tlsgpu_seal_host ----------------------------------------------------------

def pinned(engine, nbytes, keep):
    p = C.c_void_p()
    assert engine.lib.tlsgpu_host_alloc(engine.handle, max(nbytes, 1), C.byref(p)) == 0
    keep.append(p.value)
    return p.value


def run_seal_host(ta, engine, aead, sessions, lens):
    """tlsgpu_seal_host through a pipeline of many chunks, output slots two bytes
    apart (a wrong span damages a neighbour), then tlsgpu_open_host of the result."""
    rng = np.random.default_rng(91)
    table = ta.SessionTable(engine, len(sessions))
    table.install(0, [s[0] for s in sessions])
    recs, ip, op = [], 0, 0
    for i, n in enumerate(lens):
        sid, seq, itype = (i // 9) % len(sessions), 5000 + i, 21 + i % 3
        p, ctx, block = sessions[sid]
        content = rng.bytes(n)
        frag = tp.seal(aead, ctx, p.fixed_iv, seq, itype, content, block)
        ip += (-ip) % 16 + (i % 4)
        recs.append((sid, seq, itype, content, ip, op, frag))
        ip += n + 2
        op += len(frag) + 2
    keep = []
    in_bytes, out_bytes, n = ip, op, len(recs)
    h_in, h_out = pinned(engine, in_bytes, keep), pinned(engine, out_bytes, keep)
    h_recs, h_status = pinned(engine, 32 * n, keep), pinned(engine, 4 * n, keep)
    C.memset(h_in, 0xC3, in_bytes)
    C.memset(h_out, 0xA5, out_bytes)
    descs = np.zeros(n, dtype=ta.RECORD_DTYPE)
    for i, (sid, seq, itype, content, io, oo, frag) in enumerate(recs):
        C.memmove(h_in + io, content, len(content))
        descs[i] = (io, oo, seq, sid, ta.len_type(len(content), itype))
    C.memmove(h_recs, descs.tobytes(), descs.nbytes)
    ta.host_pipeline(engine, 4, 256 << 10)
    try:
        ta.seal_host(table, h_recs, n, h_in, in_bytes - 2, h_out, out_bytes, h_status)
        st = np.ctypeslib.as_array((C.c_int32 * n).from_address(h_status)).copy()
        got = C.string_at(h_out, out_bytes)
        for i, (sid, seq, itype, content, io, oo, frag) in enumerate(recs):
            assert st[i] == len(frag) and got[oo:oo + len(frag)] == frag, (i, len(content), sid)
        for i, (sid, seq, itype, content, io, oo, frag) in enumerate(recs):
            descs[i] = (oo, oo, seq, sid, ta.len_type(len(frag), 23))
        C.memmove(h_recs, descs.tobytes(), descs.nbytes)
        ta.open_host(table, h_recs, n, h_out, out_bytes, h_out, out_bytes, h_status)
        st = np.ctypeslib.as_array((C.c_int32 * n).from_address(h_status)).copy()
        for i, (sid, seq, itype, content, io, oo, frag) in enumerate(recs):
            assert st[i] == len(content), (i, st[i])
            assert C.string_at(h_out + oo, len(content) + 1) == content + bytes([itype]), i
    finally:
        ta.host_pipeline(engine, 2, 32 << 20)
        for p in keep:
            engine.lib.tlsgpu_host_free(engine.handle, p)
        table.close()


def test_seal_host_spans(ta, engine, aead):
    sessions = _sessions(ta, aead, "aes-256-gcm", 91)
    lens = [COMMON[i % 17] for i in range(960)] + [16383, 16384, 16382] * 10 + [991, 992, 0, 1]
    run_seal_host(ta, engine, aead, sessions, lens)
