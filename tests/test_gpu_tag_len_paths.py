"""tlsgpu_session_params.tag_len other than 16 on the wire and host paths, on
the GPU (the batch paths: test_gpu_tag_len.py; the model and the host code under
the stub: test_tag_len_model.py).

tlsgpu_seal_wire frames with wire_seal_frame_kernel, whose record length is
explicit nonce + fragment + the session's tag; the whole wire image (gaps
between the streams' regions included) is compared with test_seal_wire.py's
model_write over the oracle's AEAD at the session's tag length, wire_len with
tlsgpu_seal_wire_size, and tlsgpu_open_wire reads the wire back.

tlsgpu_seal_host / tlsgpu_open_host copy each chunk's output back by exact spans
(host_paths.cpp span_out).  With a pipeline of 64 KiB chunks on four streams a
span computed with another tag length either clips the last bytes of a chunk's
last record or copies over bytes that a neighbouring chunk owns.  The pinned
output starts as 0xA5 and is compared whole: a chunk's copy runs from its first
record's out_off to its last record's end, so the gaps inside a chunk come back
as the zeros of the cleared device mirror and the gaps between chunks stay 0xA5.
A chunk ends with the record at which the descriptors' lengths since the last
cut reach the chunk size (host_batch; the model below restates that).
"""
import ctypes as C

import numpy as np
import pytest

import batch_image as bi
import pyoracle as po
from test_seal_wire import TLS12, model_write

pytestmark = pytest.mark.gpu

KINDS = {"aes-128-gcm": po.AES_128_GCM, "aes-256-gcm": po.AES_256_GCM,
         "chacha20-poly1305": po.CHACHA20_POLY1305,
         "chacha20-poly1305-old": po.CHACHA20_POLY1305_OLD}
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


# -- tlsgpu_seal_wire, read back by tlsgpu_open_wire -----------------------------

WIRE_TAGS = [12, 8, 16]
WIRE_SIZES = [0, 1, 100, 16384, 16385, 40000]
WIRE_FRAGS = [0, 0, 0, 0, 4096, 1000]       # max_send_fragment (0 = 16384)


@pytest.mark.parametrize("name", list(KINDS))
def test_seal_wire_and_open_wire(ta, engine, oracle, name):
    kind = KINDS[name]
    sessions = bi.make_sessions(ta, oracle, [kind] * 3, WIRE_TAGS, 300 + kind)
    table = ta.SessionTable(engine, len(sessions))
    table.install(0, [s.params for s in sessions])
    rng = np.random.default_rng(17 * kind)
    data, streams, expected, wire_off = bytearray(), [], [], 0
    for sid, s in enumerate(sessions):
        for i, (n, mf) in enumerate(zip(WIRE_SIZES, WIRE_FRAGS)):
            data += b"\xC3" * (1 + (i + sid) % 4)          # misaligned application data
            d, seq, rtype = rng.bytes(n), (1 << 34) + 1000 * len(streams), 23 if i % 4 else 22
            exp, k = model_write(oracle, None, d, seq, rtype, TLS12, mf,
                                 seal=lambda q, t, piece, s=s: bi.model_seal(oracle, s, q, t, piece))
            size = ta.seal_wire_size(kind, n, mf, tag_len=s.t)
            assert size == len(exp) == k * (5 + s.eiv + s.t) + n
            streams.append((len(data), wire_off, seq, n, sid, TLS12, rtype, 0, mf))
            expected.append((exp, k, d))
            data += d
            wire_off += size + 1 + len(streams) % 3        # gaps between the wire regions
    data += b"\xC3"
    wire_bytes = wire_off + 64
    nrec = sum(k for _, k, _ in expected)
    desc = np.array(streams, dtype=ta.WRITE_STREAM_DTYPE)
    bufs = [ta.DeviceBuffer(engine, x) for x in
            (len(data), wire_bytes, desc.nbytes, 32 * nrec, 4 * nrec,
             ta.WRITE_RESULT_DTYPE.itemsize * len(streams), 4)]
    d_data, d_wire, d_streams, d_recs, d_status, d_results, d_total = bufs
    d_data.upload(bytes(data))
    d_wire.fill(0xA5)
    d_streams.upload(desc.view(np.uint8))
    d_status.upload(np.full(nrec, SENTINEL, dtype=np.uint32).view(np.uint8))
    ta.seal_wire(table, d_streams.ptr, len(streams), d_data.ptr, len(data), d_wire.ptr, wire_bytes,
                 nrec, d_recs.ptr, d_status.ptr, d_results.ptr, d_total.ptr)
    engine.sync()
    wire = d_wire.download().tobytes()
    res = d_results.download().view(ta.WRITE_RESULT_DTYPE)
    st = d_status.download().view(np.int32)[:nrec]
    assert int(d_total.download().view(np.uint32)[0]) == nrec
    image = bytearray(b"\xA5" * wire_bytes)
    for i, ((doff, woff, seq, n, sid, ver, rtype, _, mf), (exp, k, d)) in enumerate(
            zip(streams, expected)):
        image[woff:woff + len(exp)] = exp
        assert (int(res[i]["records"]), int(res[i]["wire_len"]), int(res[i]["next_seq"])) == \
            (k, len(exp), seq + k), (i, res[i])
        frag = mf or 16384
        s = sessions[sid]
        for j in range(k):
            assert int(st[int(res[i]["first"]) + j]) == s.eiv + min(frag, n - j * frag) + s.t
    diff = [i for i in range(wire_bytes) if wire[i] != image[i]][:4] if wire != bytes(image) else []
    assert not diff, (name, "wire bytes", diff)
    # read it back with the device ssl3_get_record
    ws = [(woff, int(res[i]["wire_len"]), sid, seq, ver, 0, 0)
          for i, (doff, woff, seq, n, sid, ver, rtype, _, mf) in enumerate(streams)]
    wdesc = np.array(ws, dtype=ta.WIRE_STREAM_DTYPE)
    d_ws = ta.DeviceBuffer(engine, wdesc.nbytes)
    d_ws.upload(wdesc.view(np.uint8))
    d_wres = ta.DeviceBuffer(engine, ta.WIRE_RESULT_DTYPE.itemsize * len(ws))
    ta.open_wire(table, d_ws.ptr, len(ws), d_wire.ptr, nrec, d_recs.ptr, d_status.ptr, d_wres.ptr,
                 d_total.ptr)
    engine.sync()
    plain = d_wire.download().tobytes()
    wres = d_wres.download().view(ta.WIRE_RESULT_DTYPE)
    recs = d_recs.download().view(ta.RECORD_DTYPE)
    st = d_status.download().view(np.int32)
    for i, (exp, k, d) in enumerate(expected):
        assert wres[i]["alert"] == 0 and wres[i]["delivered"] == k == wres[i]["records"], (i, wres[i])
        first = int(wres[i]["first"])
        got = b"".join(plain[int(recs[first + j]["out_off"]):
                             int(recs[first + j]["out_off"]) + int(st[first + j])] for j in range(k))
        assert got == d, i
    assert plain[wire_off:] == b"\xA5" * (wire_bytes - wire_off)
    for b in bufs + [d_ws, d_wres]:
        b.free()
    table.close()


# -- tlsgpu_seal_host, then tlsgpu_open_host ---------------------------------------

HOST_TAGS = [12, 5, 16]
HOST_LENS = [0, 1, 17, 1400, 4096, 16384]
CHUNK = 64 << 10


def pinned(engine, nbytes, keep):
    p = C.c_void_p()
    assert engine.lib.tlsgpu_host_alloc(engine.handle, max(nbytes, 1), C.byref(p)) == 0
    keep.append(p.value)
    return p.value


def chunk_image(out_bytes, lens, out_offs, outs):
    """The expected host output: 0xA5, and per chunk zeros from its first record's
    out_off to its last record's end with the records' outputs in them."""
    img = np.full(out_bytes, 0xA5, dtype=np.uint8)
    acc, first, chunks = 0, 0, 0
    for i, l in enumerate(lens):
        acc += l
        if (acc >= CHUNK and i + 1 < len(lens)) or i + 1 == len(lens):
            lo = out_offs[first]
            hi = max(out_offs[j] + len(outs[j]) for j in range(first, i + 1))
            img[lo:hi] = 0
            acc, first, chunks = 0, i + 1, chunks + 1
    for o, b in zip(out_offs, outs):
        img[o:o + len(b)] = np.frombuffer(b, dtype=np.uint8)
    return img, chunks


@pytest.mark.parametrize("name", list(KINDS))
def test_seal_host_then_open_host(ta, engine, oracle, name):
    kind = KINDS[name]
    sessions = bi.make_sessions(ta, oracle, [kind] * 3, HOST_TAGS, 500 + kind)
    table = ta.SessionTable(engine, len(sessions))
    table.install(0, [s.params for s in sessions])
    rng = np.random.default_rng(23 * kind)
    recs, ip, op = [], 0, 0
    for i in range(300):
        sid, n = (i // 7) % 3, HOST_LENS[(i + i // 6) % 6]
        e = bi.seal_entry(ta, oracle, sessions, sid, 9000 + i, 21 + i % 3, rng.bytes(n))
        recs.append((e, ip, op))
        ip += n + 3
        op += len(e.out) + 3
    n = len(recs)
    in_bytes, out_bytes = ip - 3, op - 3
    in_offs, frag_offs = [r[1] for r in recs], [r[2] for r in recs]
    keep = []
    h_in, h_out, h_back = (pinned(engine, b, keep) for b in (in_bytes, out_bytes, in_bytes))
    h_recs, h_status = pinned(engine, 32 * n, keep), pinned(engine, 4 * n, keep)
    C.memset(h_in, 0xC3, in_bytes)
    C.memset(h_out, 0xA5, out_bytes)
    C.memset(h_back, 0xA5, in_bytes)
    descs = np.zeros(n, dtype=ta.RECORD_DTYPE)
    for i, (e, io, oo) in enumerate(recs):
        C.memmove(h_in + io, e.inp, len(e.inp))
        descs[i] = (io, oo, e.seq, e.sid, ta.len_type(len(e.inp), e.rtype))
    C.memmove(h_recs, descs.tobytes(), descs.nbytes)
    status = lambda: np.ctypeslib.as_array((C.c_int32 * n).from_address(h_status)).copy()
    ta.host_pipeline(engine, 4, CHUNK)
    try:
        C.memset(h_status, 0x5A, 4 * n)
        ta.seal_host(table, h_recs, n, h_in, in_bytes, h_out, out_bytes, h_status)
        img, chunks = chunk_image(out_bytes, [len(r[0].inp) for r in recs], frag_offs,
                                  [r[0].out for r in recs])
        assert chunks >= 8
        assert (status() == [r[0].st for r in recs]).all()
        got = np.frombuffer(C.string_at(h_out, out_bytes), dtype=np.uint8)
        diff = np.flatnonzero(got != img)
        assert diff.size == 0, (name, "seal_host byte", int(diff[0]), int(diff.size))
        # open what was sealed, out of place, the plaintexts at the offsets they came from
        for i, (e, io, oo) in enumerate(recs):
            descs[i] = (oo, io, e.seq, e.sid, ta.len_type(len(e.out), e.rtype))
        C.memmove(h_recs, descs.tobytes(), descs.nbytes)
        C.memset(h_status, 0x5A, 4 * n)
        ta.open_host(table, h_recs, n, h_out, out_bytes, h_back, in_bytes, h_status)
        img, chunks = chunk_image(in_bytes, [len(r[0].out) for r in recs], in_offs,
                                  [r[0].inp for r in recs])
        assert chunks >= 8
        assert (status() == [len(r[0].inp) for r in recs]).all()
        got = np.frombuffer(C.string_at(h_back, in_bytes), dtype=np.uint8)
        diff = np.flatnonzero(got != img)
        assert diff.size == 0, (name, "open_host byte", int(diff[0]), int(diff.size))
    finally:
        ta.host_pipeline(engine, 2, 32 << 20)
        for p in keep:
            engine.lib.tlsgpu_host_free(engine.handle, p)
        table.close()
