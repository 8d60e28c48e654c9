"""tlsgpu_gather_wire on the GPU against the rule's model (read_wire_model.py).

Wire bytes come from the engine's own write side: every record of a read stream
is one tlsgpu_seal_wire write stream (a record without content, which a write
never sends, is one tlsgpu_seal_batch record under a header written here), laid
back to back with continuing sequence numbers.  tlsgpu_open_wire opens them;
what it returned — descriptors, statuses, wire results, the opened buffer — is
the model's input, so every comparison is exact: the whole of d_app (pre-filled
with 0xA5), every result field, and d_wire before and after the gather.
"""
import numpy as np
import pytest

from read_wire_model import gather_model

pytestmark = pytest.mark.gpu

TLS12, TLS13 = 0x0303, 0x0304
FILL = 0xA5


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
    """(kind, session version, pad_block)"""
    return {"aes128gcm-tls12": (ta.AES_128_GCM, TLS12, 0),
            "chacha-tls12": (ta.CHACHA20_POLY1305, TLS12, 0),
            "aes256gcm-tls13-pad64": (ta.AES_256_GCM, TLS13, 64),
            "chacha-tls13": (ta.CHACHA20_POLY1305_TLS13, TLS13, 0)}


class Opened:
    """Read streams sealed by the engine and opened by tlsgpu_open_wire: the device
    buffers a gather reads and host copies of them."""

    def __init__(self, ta, engine, suite, spec, seed, max_records=None, tamper=None):
        kind, version, pad = suites(ta)[suite]
        t13 = version == TLS13
        eiv = 0 if t13 else ta.EXPLICIT_NONCE_LEN[kind]
        rng = np.random.default_rng(seed)
        self.ta, self.engine = ta, engine
        self.table = ta.SessionTable(engine, 1)
        self.table.install(0, [ta.SessionParams(kind, rng.bytes(ta.KEY_LEN[kind]),
                                                rng.bytes(12 if t13 else ta.FIXED_IV_LEN[kind]),
                                                version=version, pad_block=pad)])
        data, writes, empties, rstreams, pos = bytearray(b"\xC3"), [], [], [], 7
        self.contents, self.layout = [], []     # per stream: [content], [(wire offset, size)]
        for k, records in enumerate(spec):
            seq0, start = 1000 * k + 5, pos
            self.contents.append([])
            self.layout.append([])
            for j, (rtype, n) in enumerate(records):
                size = 5 + eiv + (ta.tls13_inner_len(n, pad) if t13 else n) + ta.TAG_LEN
                content = rng.bytes(n)
                if n:
                    assert ta.seal_wire_size(kind, n, 0, 0, version=version, pad_block=pad) == size
                    writes.append((len(data), pos, seq0 + j, n, 0, TLS12, rtype, 0, 0))
                    data += content
                else:
                    empties.append((pos, seq0 + j, rtype, size))
                self.contents[k].append(content)
                self.layout[k].append((pos, size))
                pos += size
            rstreams.append((start, pos - start, 0, seq0, TLS12, 0, 0))
            pos += 3
        self.wire_bytes = pos + 64
        nrec = sum(len(r) for r in spec)
        self.max_records = nrec if max_records is None else max_records
        # the write side
        wst = np.array(writes, dtype=ta.WRITE_STREAM_DTYPE)
        est = np.zeros(len(empties), dtype=ta.RECORD_DTYPE)
        for i, (o, seq, rtype, _) in enumerate(empties):
            est[i] = (0, o + 5, seq, 0, ta.len_type(0, rtype))
        B = lambda n: ta.DeviceBuffer(engine, n)  # noqa: E731
        d_data, d_wst, d_srecs, d_sst, d_sres, d_total, d_est = (
            B(len(data)), B(wst.nbytes), B(32 * len(wst)), B(4 * (len(wst) + len(est))),
            B(32 * len(wst)), B(4), B(est.nbytes))
        self.d_wire = B(self.wire_bytes)
        d_data.upload(bytes(data))
        self.d_wire.fill(0)
        if len(wst):
            d_wst.upload(wst.view(np.uint8))
            ta.seal_wire(self.table, d_wst.ptr, len(wst), d_data.ptr, len(data), self.d_wire.ptr,
                         self.wire_bytes, len(wst), d_srecs.ptr, d_sst.ptr, d_sres.ptr, d_total.ptr)
        if len(est):
            d_est.upload(est.view(np.uint8))
            ta.seal_batch(self.table, d_est.ptr, len(est), d_data.ptr, len(data), self.d_wire.ptr,
                          self.wire_bytes, d_sst.ptr + 4 * len(wst))
        engine.sync()
        assert (d_sst.download().view(np.int32)[:len(wst) + len(est)] > 0).all()
        sealed = self.d_wire.download()
        for o, _, rtype, size in empties:
            sealed[o:o + 5] = (23 if t13 else rtype, 3, 3, (size - 5) >> 8, (size - 5) & 0xFF)
        if tamper:
            tamper(sealed, self.layout)
        self.d_wire.upload(sealed)
        for b in (d_data, d_wst, d_srecs, d_sst, d_sres, d_total, d_est):
            b.free()
        # the read side
        self.streams = np.array(rstreams, dtype=ta.WIRE_STREAM_DTYPE)
        self.d_streams, self.d_recs, self.d_status, self.d_results, self.d_total = (
            B(self.streams.nbytes), B(32 * self.max_records), B(4 * self.max_records),
            B(32 * len(spec)), B(4))
        self.d_streams.upload(self.streams.view(np.uint8))
        ta.open_wire(self.table, self.d_streams.ptr, len(spec), self.d_wire.ptr, self.max_records,
                     self.d_recs.ptr, self.d_status.ptr, self.d_results.ptr, self.d_total.ptr)
        engine.sync()
        self.wire = self.d_wire.download()
        self.recs = self.d_recs.download().view(ta.RECORD_DTYPE)[:self.max_records].copy()
        self.status = self.d_status.download().view(np.int32)[:self.max_records].copy()
        self.results = self.d_results.download().view(ta.WIRE_RESULT_DTYPE).copy()

    def gather(self, reads, app, wire_bytes=None, max_records=None):
        """One tlsgpu_gather_wire over `app` (the buffer's contents before the
        call) compared with the model in full; returns (app after, results)."""
        ta, engine, n = self.ta, self.engine, len(self.streams)
        wire_bytes = self.wire_bytes if wire_bytes is None else wire_bytes
        max_records = self.max_records if max_records is None else max_records
        rd = np.zeros(n, dtype=ta.READ_STREAM_DTYPE)
        for i, row in enumerate(reads):
            rd[i] = row
        d_reads, d_app, d_out = (ta.DeviceBuffer(engine, b) for b in (rd.nbytes, len(app), 32 * n))
        d_reads.upload(rd.view(np.uint8))
        d_app.upload(app)
        d_out.fill(0xEE)
        ta.gather_wire(self.table, self.d_streams.ptr, self.d_results.ptr, n, self.d_recs.ptr,
                       self.d_status.ptr, max_records, self.d_wire.ptr, wire_bytes, d_reads.ptr,
                       d_app.ptr, len(app), d_out.ptr)
        engine.sync()
        got_app = d_app.download()
        got = d_out.download().view(ta.READ_RESULT_DTYPE).copy()
        assert np.array_equal(self.d_wire.download(), self.wire), "the gather wrote d_wire"
        want_app, want = gather_model(self.streams, self.results, self.recs, self.status, max_records,
                                      self.wire, wire_bytes, rd, app)
        for f in ta.READ_RESULT_DTYPE.names:
            assert np.array_equal(got[f], want[f]), (f, got[f], want[f])
        bad = np.flatnonzero(got_app != want_app)
        assert bad.size == 0, f"{bad.size} bytes of d_app differ, first at {bad[0]}"
        for b in (d_reads, d_app, d_out):
            b.free()
        return got_app, got

    def close(self):
        for b in (self.d_wire, self.d_streams, self.d_recs, self.d_status, self.d_results,
                  self.d_total):
            b.free()
        self.table.close()


def canvas(nbytes):
    return np.full(nbytes, FILL, dtype=np.uint8)


def res(r):
    return tuple(int(r[f]) for f in ("app_len", "records", "next", "stop", "stop_type", "stop_len"))


# content lengths around every boundary of the copy: the 16-byte block, the wave's
# 1 KiB step, the piece sizes compiled (2048, 4096, one wave per record) and the
# record limit; 33 makes a stream's total 1 modulo 16.  With these lengths the
# wire holds about 3.5 KiB per record slot: one wave per record
LENGTHS = [0, 1, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097,
           8191, 8192, 8193, 16383, 16384, 33]


@pytest.mark.parametrize("suite", ["aes128gcm-tls12", "chacha-tls12", "aes256gcm-tls13-pad64",
                                   "chacha-tls13"])
def test_alignment(ta, engine, suite):
    """One stream per app_off residue 0..15, packed: stream k + 1's region begins
    where stream k's ends, so a stray byte at either end of any piece lands in a
    neighbour or a canary."""
    assert sum(LENGTHS) % 16 == 1
    spec = [[(23, n) for n in LENGTHS[k:] + LENGTHS[:k]] for k in range(16)]
    o = Opened(ta, engine, suite, spec, seed=11)
    assert (o.results["delivered"] == len(LENGTHS)).all() and (o.results["alert"] == 0).all()
    total, lead = sum(LENGTHS), 32
    reads = [(lead + k * total, total, 0) for k in range(16)]
    assert sorted(r[0] % 16 for r in reads) == list(range(16))
    app, got = o.gather(reads, canvas(lead + 16 * total + 64))
    for k in range(16):
        assert res(got[k]) == (total, len(LENGTHS), len(LENGTHS), ta.READ_END, 0, 0)
        assert int(got[k]["consumed"]) == int(o.streams[k]["wire_len"])
        # and the bytes are the ones that were sealed, in order
        assert app[reads[k][0]:reads[k][0] + total].tobytes() == b"".join(o.contents[k])
    assert (app[:lead] == FILL).all() and (app[lead + 16 * total:] == FILL).all()
    o.close()


# long records only: more than 9 KiB of wire per record slot, so the copy splits
# each record into 2048-byte pieces, one wave each; the total is 1 modulo 16 again
LONG = [16384, 16383, 16381, 12289, 16384, 16372]


@pytest.mark.parametrize("suite", ["aes128gcm-tls12", "aes256gcm-tls13-pad64"])
def test_alignment_of_split_records(ta, engine, suite):
    """The same packing over long records, which take the copy's other path: a
    record in pieces, each piece with its own first and last partial block."""
    assert sum(LONG) % 16 == 1
    spec = [[(23, n) for n in LONG[k % 6:] + LONG[:k % 6]] for k in range(16)]
    o = Opened(ta, engine, suite, spec, seed=19)
    assert o.wire_bytes // o.max_records > 9216
    assert (o.results["delivered"] == len(LONG)).all()
    total, lead = sum(LONG), 48
    reads = [(lead + k * total, total, 0) for k in range(16)]
    assert sorted(r[0] % 16 for r in reads) == list(range(16))
    app, got = o.gather(reads, canvas(lead + 16 * total + 64))
    for k in range(16):
        assert res(got[k]) == (total, len(LONG), len(LONG), ta.READ_END, 0, 0)
        assert app[reads[k][0]:reads[k][0] + total].tobytes() == b"".join(o.contents[k])
    assert (app[:lead] == FILL).all() and (app[lead + 16 * total:] == FILL).all()
    o.close()


def test_scan_carry(ta, engine):
    """130 records (more than two 64-record steps) next to a stream without
    records and a stream of one."""
    lens = [1 + (7 * i) % 40 for i in range(130)]
    o = Opened(ta, engine, "aes128gcm-tls12", [[(23, n) for n in lens], [], [(23, 5)]], seed=12)
    total = sum(lens)
    app, got = o.gather([(3, total, 0), (3 + total, 0, 0), (3 + total, 5, 0)], canvas(total + 40))
    assert res(got[0]) == (total, 130, 130, ta.READ_END, 0, 0)
    assert res(got[1]) == (0, 0, 0, ta.READ_END, 0, 0) and int(got[1]["consumed"]) == 0
    assert res(got[2]) == (5, 1, 1, ta.READ_END, 0, 0)
    assert app[3:3 + total].tobytes() == b"".join(o.contents[0])
    # a stop in the third step, and a start in the second
    _, got = o.gather([(0, sum(lens[:129]), 0), (0, 0, 0), (0, 0, 0)], canvas(total))
    assert res(got[0]) == (sum(lens[:129]), 129, 129, ta.READ_FULL, 23, lens[129])
    assert res(got[2]) == (0, 0, 0, ta.READ_FULL, 23, 5)
    _, got = o.gather([(1, total, 70), (0, 0, 1), (0, 0, 2)], canvas(total))
    assert res(got[0]) == (sum(lens[70:]), 60, 130, ta.READ_END, 0, 0)
    assert got[1]["stop"] == ta.READ_OUT_OF_BOUNDS and got[2]["stop"] == ta.READ_OUT_OF_BOUNDS
    o.close()


@pytest.mark.parametrize("suite,other", [("aes128gcm-tls12", 21), ("aes256gcm-tls13-pad64", 22),
                                         ("chacha-tls13", 21)])
def test_stops_at_a_record_that_is_not_application_data(ta, engine, suite, other):
    """data, a warning alert (21) or a handshake record (22; under TLS 1.3 the
    type is the inner byte), data: the first gather stops there, a second one
    with start = next + 1 delivers the rest behind the first one's bytes."""
    o = Opened(ta, engine, suite, [[(23, 300), (23, 17), (other, 2), (23, 100), (23, 1)]], seed=13)
    assert int(o.results[0]["delivered"]) == 5
    app, got = o.gather([(5, 1000, 0)], canvas(500))
    assert res(got[0]) == (317, 2, 2, ta.READ_NOT_APP_DATA, other, 2)
    slot = int(o.results[0]["first"]) + 2    # the record lies at its descriptor's out_off
    at = int(o.recs[slot]["out_off"])
    assert o.wire[at:at + 2].tobytes() == o.contents[0][2]
    app, got = o.gather([(5 + 317, 1000, int(got[0]["next"]) + 1)], app)
    assert res(got[0]) == (101, 2, 5, ta.READ_END, 0, 0)
    assert int(got[0]["consumed"]) == int(o.streams[0]["wire_len"])
    assert app[5:5 + 418].tobytes() == b"".join(o.contents[0][i] for i in (0, 1, 3, 4))
    o.close()


def test_app_cap_exact_and_one_byte_short(ta, engine):
    lens = [4096, 1, 4097, 700]
    o = Opened(ta, engine, "chacha-tls12", [[(23, n) for n in lens]], seed=14)
    total = sum(lens)
    _, got = o.gather([(9, total, 0)], canvas(total + 32))
    assert res(got[0]) == (total, 4, 4, ta.READ_END, 0, 0)
    app, got = o.gather([(9, total - 1, 0)], canvas(total + 32))
    assert res(got[0]) == (total - 700, 3, 3, ta.READ_FULL, 23, 700)
    assert (app[9 + total - 700:] == FILL).all()
    # the same limit from the end of d_app
    _, got = o.gather([(9, total, 0)], canvas(9 + total - 1))
    assert res(got[0]) == (total - 700, 3, 3, ta.READ_FULL, 23, 700)
    o.close()


def test_failed_record_ends_what_is_gathered(ta, engine):
    """One flipped ciphertext bit in the middle record: delivered ends there; the
    zero-filled record and the skipped ones behind it are not gathered."""
    def flip(wire, layout):
        pos, size = layout[0][2]
        wire[pos + size // 2] ^= 0x04
    o = Opened(ta, engine, "aes128gcm-tls12",
               [[(23, 50), (23, 60), (23, 70), (23, 80), (23, 90)], [(23, 10)]], seed=15, tamper=flip)
    assert (int(o.results[0]["delivered"]), int(o.results[0]["alert"])) == (2, 20)
    assert list(o.status[:5]) == [50, 60, ta.REC_BAD_MAC, ta.REC_SKIPPED, ta.REC_SKIPPED]
    app, got = o.gather([(0, 1000, 0), (110, 10, 0)], canvas(160))
    assert res(got[0]) == (110, 2, 2, ta.READ_END, 0, 0)
    assert int(got[0]["consumed"]) == o.layout[0][2][0] - o.layout[0][0][0]
    assert res(got[1]) == (10, 1, 1, ta.READ_END, 0, 0) and (app[120:] == FILL).all()
    o.close()


def test_stream_truncated_by_max_records(ta, engine):
    """max_records smaller than the records present: the stream open_wire cut at
    a record boundary gathers what was framed."""
    o = Opened(ta, engine, "chacha-tls12", [[(23, 20), (23, 30), (23, 40), (23, 50), (23, 60)]],
               seed=16, max_records=3)
    assert (int(o.results[0]["records"]), int(o.results[0]["delivered"])) == (3, 3)
    app, got = o.gather([(2, 500, 0)], canvas(200))
    assert res(got[0]) == (90, 3, 3, ta.READ_END, 0, 0)
    assert int(got[0]["consumed"]) == int(o.results[0]["consumed"])
    assert app[2:92].tobytes() == b"".join(o.contents[0][:3])
    # told of fewer slots than the stream holds: nothing is gathered
    app, got = o.gather([(2, 500, 0)], canvas(200), max_records=2)
    assert res(got[0]) == (0, 0, 0, ta.READ_OUT_OF_BOUNDS, 0, 0) and (app == FILL).all()
    o.close()


def test_out_of_bounds_requests_write_nothing(ta, engine):
    o = Opened(ta, engine, "aes128gcm-tls12", [[(23, 40), (23, 40)], [(23, 40)], [(23, 40)]], seed=17)
    # start > delivered; app_off beyond app_bytes; a plaintext span that leaves wire_bytes
    end = int(o.recs[int(o.results[2]["first"])]["out_off"]) + 40
    app, got = o.gather([(0, 100, 3), (500, 100, 0), (0, 100, 0)], canvas(128), wire_bytes=end - 1)
    assert res(got[0]) == (0, 0, 3, ta.READ_OUT_OF_BOUNDS, 0, 0)
    assert res(got[1]) == (0, 0, 0, ta.READ_FULL, 23, 40)
    assert res(got[2]) == (0, 0, 0, ta.READ_OUT_OF_BOUNDS, 0, 0)
    assert (app == FILL).all()
    o.close()


def test_argument_errors_and_the_empty_call(ta, engine):
    o = Opened(ta, engine, "chacha-tls12", [[(23, 40)]], seed=18)
    d_reads, d_out = ta.DeviceBuffer(engine, 16), ta.DeviceBuffer(engine, 32)
    d_app = ta.DeviceBuffer(engine, 64)
    d_app.fill(FILL)
    lib, t = o.table.lib, o.table.handle

    def call(n_streams, d_wire, wire_bytes, app, app_bytes, reads=d_reads.ptr):
        return lib.tlsgpu_gather_wire(t, o.d_streams.ptr, o.d_results.ptr, n_streams, o.d_recs.ptr,
                                      o.d_status.ptr, o.max_records, d_wire, wire_bytes, reads, app,
                                      app_bytes, d_out.ptr, None)
    w = o.d_wire.ptr
    assert call(1, w, o.wire_bytes, w + o.wire_bytes - 1, 64) == -1     # d_app's first byte inside d_wire
    assert call(1, w, o.wire_bytes, w - 63, 64) == -1                   # its last byte
    assert b"overlaps" in lib.tlsgpu_last_error()
    assert call(1, w, o.wire_bytes, d_app.ptr, 64, reads=None) == -1
    assert call(0, w, o.wire_bytes, d_app.ptr, 64) == 0                 # the empty call
    assert lib.tlsgpu_gather_wire(t, None, None, 0, None, None, 0, None, 0, None, None, 0, None,
                                  None) == 0
    engine.sync()
    assert (d_app.download() == FILL).all()
    assert np.array_equal(o.d_wire.download(), o.wire)
    for b in (d_reads, d_out, d_app):
        b.free()
    o.close()
