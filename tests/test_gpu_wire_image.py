"""tlsgpu_seal_wire and tlsgpu_open_wire over hundreds of streams, whole images
(wire_image.py: layout, slot rule, models, checkers).

Seal: one population of 300 streams per session table, used by prefix at the
lane, wave and workgroup edges of wire_seal_frame_kernel (one stream per lane,
256 lanes), on a mixed table (check_record_bounds, two GCM passes, the staged
ChaCha kernel and the draft-suite kernel behind one wire call), on the two fused
setups and on an unhinted single-kind table; max_records cuts; and one
out-of-bounds or unknown-session condition per case among valid streams.
Open: test_wire.build_streams' twelve shapes cycled over a mixed TLS 1.2 table
at wire_frame_kernel's workgroup edges (4 streams per workgroup), cuts that fall
in later workgroups, and one tlsgpu_gather_wire over the largest open.
"""
import random
from dataclasses import replace

import numpy as np
import pytest

import pyoracle as po
import wire_image as wi
from read_wire_model import gather_model
from talos_amd import REC_OUT_OF_BOUNDS, REC_PUBLIC_INVALID
from test_wire import build_streams

pytestmark = pytest.mark.gpu

CAPACITY = 8        # sessions 0..5 installed, 6 and 7 as tlsgpu_sessions_create leaves them
A128, A256, CC, OLD = po.AES_128_GCM, po.AES_256_GCM, po.CHACHA20_POLY1305, po.CHACHA20_POLY1305_OLD
TABLES = {"mixed": ([A128, CC, A256, OLD, CC, A128], 0),
          "chacha": ([CC] * 6, 0),                  # fused_cc
          "aes128-runs": ([A128] * 6, 2),           # TLSGPU_HINT_SESSION_RUNS: fused_gcm
          "aes256": ([A256] * 6, 0)}
POP = 300
SPARE = 5           # record slots an uncut case has beyond the ones its streams take


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


def population(nsess, seed):
    """Stream i of the seal population (the same data under every table)."""
    rng = np.random.default_rng(seed)
    lens, frags, big = [0, 1, 15, 16, 17, 100, 1400, 2049], [0, 0, 512, 0, 4096, 20000, 1], \
        [16384, 16385, 40000]
    out = []
    for i in range(POP):
        n = big[(i // 37) % 3] if i % 37 == 36 else lens[i % 8]
        mf = frags[i % 7]
        if mf == 1 and n > 100:         # one-byte records on short streams only
            mf = 0
        rtype = 23 if i % 4 else (22, 21)[(i // 4) % 2]
        out.append(wi.WStream(rng.bytes(n), i % nsess, (1 << 63) + 1000 * i, rtype, mf))
    return out


class Case:
    """One session table with its oracle sessions, memo and seal population."""

    def __init__(self, ta, engine, oracle, kinds, hints, capacity=CAPACITY):
        self.sessions = wi.make_sessions(oracle, kinds, 4242)
        self.table = ta.SessionTable(engine, capacity)
        self.table.install(0, [s.params for s in self.sessions])
        if hints:
            self.table.hint(hints)
        self.memo = wi.Memo(oracle)
        self.pop = population(len(kinds), 99)


@pytest.fixture(scope="module")
def cases(ta, engine, oracle):
    made = {}

    def get(name):
        if name not in made:
            made[name] = Case(ta, engine, oracle, *TABLES[name])
        return made[name]
    yield get
    for c in made.values():
        c.table.close()


def seal(engine, c, streams, max_records=None, label=None, **kw):
    """Uncut (max_records None): SPARE slots more than the streams want, which must
    come back as unused slots on every route the batch behind the call takes."""
    lay = wi.layout_seal(streams, c.sessions)
    wanted = sum(wi.seal_wanted(lay, c.sessions, 1 << 30))
    got = wi.run_seal(engine, c.table, c.memo, c.sessions, lay,
                      wanted + SPARE if max_records is None else max_records, label, **kw)
    if max_records is None:
        assert (got["status"][wanted:] == REC_PUBLIC_INVALID).all()
        assert (got["recs"][wanted:].view(np.uint8) == 0xFF).all()
    print(label, "streams", len(streams), "records wanted", wanted, "slot order differs:",
          got["reordered"])
    return lay, got


def open_sealed(engine, c, streams, lay, got, label):
    """tlsgpu_open_wire over the wire a seal left: the whole image again, and every
    stream's plaintext is its data."""
    rs = [dict(wire=got["wire"][o:o + int(r["wire_len"])].tobytes(), seq=s.seq, version=wi.TLS12,
               first=False, rbuf=0, session=s.session)
          for s, (_, o), r in zip(streams, lay.laid, got["results"])]
    olay = wi.OpenLayout(rs, [o for _, o in lay.laid], got["wire"].copy(), lay.wire_bytes)
    back = wi.run_open(engine, c.table, c.memo, c.sessions, olay, int(got["total"]) + SPARE, label)
    assert back["total"] == got["total"]
    assert (back["status"][back["total"]:] == REC_PUBLIC_INVALID).all()
    for i, s in enumerate(streams):
        r = back["results"][i]
        assert int(r["alert"]) == 0 and int(r["delivered"]) == int(got["results"][i]["records"])
        f = int(r["first"])
        plain = b"".join(
            back["wire"][int(back["recs"][f + k]["out_off"]):
                         int(back["recs"][f + k]["out_off"]) + int(back["status"][f + k])].tobytes()
            for k in range(int(r["records"])))
        assert plain == s.data, (label, "stream", i)
    print(label, "slot order differs:", back["reordered"])


# -- seal ----------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 300])
def test_seal_mixed_table_at_lane_wave_and_workgroup_edges(engine, cases, n):
    """Prefixes of the population rotated to begin with stream 13 (100 one-byte
    records), so that the single active lane of N = 1 has records to frame; N = 300
    is the whole population all the same."""
    c = cases("mixed")
    streams = (c.pop[13:] + c.pop[:13])[:n]
    assert len(streams[0].data) == 100 and streams[0].mf == 1
    lay, got = seal(engine, c, streams, label=f"seal mixed N={n}")
    if n == POP:
        open_sealed(engine, c, streams, lay, got, "open of seal mixed N=300")


@pytest.mark.parametrize("name", ["chacha", "aes128-runs", "aes256"])
def test_seal_single_kind_tables(engine, cases, name):
    c = cases(name)
    lay, got = seal(engine, c, c.pop, label=f"seal {name} N=300")
    open_sealed(engine, c, c.pop, lay, got, f"open of seal {name} N=300")


@pytest.mark.parametrize("cut", ["W-1", "W//2", "1"])
def test_seal_max_records_cut(engine, cases, cut):
    c = cases("mixed")
    w = sum(wi.seal_wanted(wi.layout_seal(c.pop, c.sessions), c.sessions, 1 << 30))
    m = {"W-1": w - 1, "W//2": w // 2, "1": 1}[cut]
    _, got = seal(engine, c, c.pop, max_records=m, label=f"seal mixed N=300 max_records={cut}")
    assert int(got["results"]["records"].sum()) == m


def test_seal_without_record_slots(engine, cases):
    """max_records = 0 with null d_recs / d_status: no descriptor, no record, d_total 0
    and the wire untouched."""
    c = cases("mixed")
    lay, got = seal(engine, c, c.pop, max_records=0, label="seal mixed N=300 max_records=0",
                    null_recs=True)
    assert got["total"] == 0 and not got["results"]["records"].any()
    assert not got["results"]["wire_len"].any() and (got["wire"] == wi.WIRE_FILL).all()
    assert (got["results"]["next_seq"] == lay.desc["seq"]).all()


# Eight population streams, one wave: 1, 1, 17, 1, 1, 100, 1 and 3 records.  Stream 2
# (17 one-byte records) and stream 5 take the conditions in the middle, stream 7
# (512 + 512 + 376 bytes) those at the end of the buffers.
BOUNDS_BASE = [1, 2, 20, 5, 6, 13, 7, 30]


def last_record(lay, c, streams):
    """(wire offset of the header, wire bytes) of the last stream's last record."""
    s = streams[-1]
    nrec = -(-len(s.data) // wi.frag_of(s.mf))
    before, size = wi.stream_size(s, c.sessions, nrec - 1), wi.stream_size(s, c.sessions)
    return lay.laid[-1][1] + before, size - before


@pytest.mark.parametrize("case", ["a", "b", "c", "d", "e", "f", "g", "h"])
def test_seal_bounds_and_sessions(engine, cases, case):
    """One condition per case, the other streams valid and compared.  The device
    buffers keep the size of the whole layout whatever wire_bytes / data_bytes the
    call is told (wire_image.layout_seal), so every stream lies inside them."""
    c = cases("mixed")
    S = [replace(c.pop[i]) for i in BOUNDS_BASE]
    max_records, want = None, None
    if case == "c":         # wire_off above wire_bytes (the layout's own end is wire_bytes)
        S[2].wire_off = wi.layout_seal(S, c.sessions).wire_bytes + 1
        want = {2: [REC_OUT_OF_BOUNDS] * 17}
    elif case == "d":       # wire_off + 5 leaves 64 bits; so does the second record's position
        S[2].wire_off = (1 << 64) - 4
        want = {2: [REC_OUT_OF_BOUNDS] * 17}
    elif case == "f":
        S[2].data_off = (1 << 63) + 5
        want = {2: [REC_OUT_OF_BOUNDS] * 17}
    elif case == "g":       # data_len near 2^32: 64-bit record count, capped at max_records
        s = S[-1]           # (the buffer holds a third fragment; data_bytes does not)
        S[-1] = wi.WStream(np.random.default_rng(7).bytes(3 * 16384), s.session, s.seq, 23, 0,
                           data_len=0xFFFFFFFF,
                           region=3 * (5 + c.sessions[s.session].eiv + 16384 + 16))
    elif case == "h":       # session 8 >= capacity, session 7 never installed
        S[2].session, S[5].session = 8, 7
    lay = wi.layout_seal(S, c.sessions)
    if case == "g":
        lay.data_bytes = lay.laid[-1][0] + 2 * 16384 + 100
        max_records = sum(wi.seal_wanted(lay, c.sessions, 1 << 30)[:-1]) + 3
    hdr, size = last_record(lay, c, S) if case in "abe" else (0, 0)
    if case == "a":         # wire_bytes ends 1 byte before the last record ends
        lay.wire_bytes = hdr + size - 1
    elif case == "b":       # ... 3 bytes into its header
        lay.wire_bytes = hdr + 3
    elif case == "e":       # data_bytes ends 1 byte before the last stream's data ends
        lay.data_bytes -= 1
    if max_records is None:     # with unused slots behind the streams' (in (h): the only ones
        used = sum(wi.seal_wanted(lay, c.sessions, 1 << 30))    # streams 2 and 5 could have had)
        max_records = used + SPARE
    got = wi.run_seal(engine, c.table, c.memo, c.sessions, lay, max_records, f"seal bounds ({case})")
    res, st = got["results"], got["status"]
    if case != "g":
        assert st[used:].tolist() == [REC_PUBLIC_INVALID] * SPARE
        assert (got["recs"][used:].view(np.uint8) == 0xFF).all()
    last = res[-1]
    tail = st[int(last["first"]):int(last["first"]) + int(last["records"])].tolist()
    eiv = c.sessions[S[-1].session].eiv
    if case in "ab":        # the record does not fit the wire: not even its header is written
        assert tail == [eiv + 512 + 16] * 2 + [REC_OUT_OF_BOUNDS]
        assert (got["wire"][hdr:] == wi.WIRE_FILL).all()
        assert int(last["wire_len"]) == wi.stream_size(S[-1], c.sessions)
    elif case == "e":       # the header of the last record is written, the fragment not
        assert tail == [eiv + 512 + 16] * 2 + [REC_OUT_OF_BOUNDS]
        assert got["wire"][hdr:hdr + 5].tolist() == [S[-1].rtype, 3, 3, (size - 5) >> 8, (size - 5) & 255]
        assert (got["wire"][hdr + 5:] == wi.WIRE_FILL).all()
    elif case == "g":
        full16k = eiv + 16384 + 16
        assert tail == [full16k, full16k, REC_OUT_OF_BOUNDS]
        assert int(last["wire_len"]) == 3 * (5 + full16k) and int(last["next_seq"]) == S[-1].seq + 3
        assert got["total"] == sum(int(r) for r in res["records"][:-1]) + max_records
    elif case == "h":       # records 0, wire_len 0, next_seq == seq; the image has no byte of them
        for i in (2, 5):
            assert (int(res[i]["records"]), int(res[i]["wire_len"]), int(res[i]["first"])) == (0, 0, 0)
            assert int(res[i]["next_seq"]) == S[i].seq
    for i, sts in (want or {}).items():
        f = int(res[i]["first"])
        assert st[f:f + int(res[i]["records"])].tolist() == sts
        assert int(res[i]["wire_len"]) == wi.stream_size(S[i], c.sessions)
        assert int(res[i]["next_seq"]) == S[i].seq + len(sts)


# -- open ----------------------------------------------------------------------------

OPEN_KINDS = [A128, CC, A256, OLD]
OPEN_N = 257


class OpenCase:
    def __init__(self, ta, engine, oracle):
        self.sessions = wi.make_sessions(oracle, OPEN_KINDS, 777)
        self.table = ta.SessionTable(engine, len(OPEN_KINDS))   # session 7 is outside it
        self.table.install(0, [s.params for s in self.sessions])
        self.memo = wi.Memo(oracle)
        rnd = random.Random(2024)
        self.streams = []
        cycle = 0
        while len(self.streams) < OPEN_N:
            # every shape meets every session: the assignment shifts by one per cycle.  The
            # good 16 KiB record stays in the first cycle only; the two overflow shapes
            # need their long fragment and keep it for four cycles, one per session
            shapes = [build_streams(oracle, rnd, s.osess, session=sid, big=cycle == 0,
                                    overflow=cycle < len(OPEN_KINDS))
                      for sid, s in enumerate(self.sessions)]
            self.streams += [shapes[(j + cycle) % len(OPEN_KINDS)][j] for j in range(12)]
            cycle += 1
        del self.streams[OPEN_N:]
        self.framed = sum(wi.open_wanted(self.memo, self.sessions, wi.layout_open(self.streams)))


@pytest.fixture(scope="module")
def opens(ta, engine, oracle):
    c = OpenCase(ta, engine, oracle)
    yield c
    c.table.close()


def run_open(engine, c, n, max_records=None, label=None, after=None):
    lay = wi.layout_open(c.streams[:n])
    wanted = sum(wi.open_wanted(c.memo, c.sessions, lay))
    got = wi.run_open(engine, c.table, c.memo, c.sessions, lay,
                      wanted + SPARE if max_records is None else max_records, label, after)
    if max_records is None:     # the slots no stream took
        assert got["status"][wanted:].tolist() == [REC_PUBLIC_INVALID] * SPARE
        assert (got["recs"][wanted:].view(np.uint8) == 0xFF).all()
    print(label, "records framed", wanted, "slot order differs:", got["reordered"])
    return lay, got


@pytest.mark.parametrize("n", [3, 4, 5, 64])
def test_open_mixed_table_at_workgroup_edges(engine, opens, n):
    run_open(engine, opens, n, label=f"open N={n}")


def test_open_257_streams_and_gather(ta, engine, opens):
    """The uncut open of all 257 streams, then one tlsgpu_gather_wire over it: d_app
    whole against read_wire_model.py, d_wire byte-identical before and after."""
    c = opens

    def gather(got, dev):
        n = len(dev["descs"])
        reads = np.zeros(n, dtype=ta.READ_STREAM_DTYPE)
        pos = 5
        for i, d in enumerate(dev["descs"]):    # disjoint regions, packed; every third one is
            cap = int(d["wire_len"]) // (2 if i % 3 == 2 else 1) + i % 3    # too small: READ_FULL
            reads[i] = (pos, cap, 0)
            pos += cap
        app = np.full(pos + 64, wi.WIRE_FILL, dtype=np.uint8)
        d_reads, d_app, d_out = (ta.DeviceBuffer(engine, b) for b in (reads.nbytes, app.nbytes, 32 * n))
        d_reads.upload(reads.view(np.uint8))
        d_app.upload(app)
        d_out.fill(0xEE)
        wire_bytes = len(got["wire"])
        ta.gather_wire(c.table, dev["streams"].ptr, dev["results"].ptr, n, dev["recs"].ptr,
                       dev["status"].ptr, len(got["status"]), dev["wire"].ptr, wire_bytes,
                       d_reads.ptr, d_app.ptr, app.nbytes, d_out.ptr)
        engine.sync()
        assert np.array_equal(dev["wire"].download(), got["wire"]), "the gather wrote d_wire"
        want_app, want = gather_model(dev["descs"], got["results"], got["recs"], got["status"],
                                      len(got["status"]), got["wire"], wire_bytes, reads, app)
        out = d_out.download().view(ta.READ_RESULT_DTYPE)
        for f in ta.READ_RESULT_DTYPE.names:
            assert np.array_equal(out[f], want[f]), (f, np.flatnonzero(out[f] != want[f])[:4])
        bad = np.flatnonzero(d_app.download() != want_app)
        assert bad.size == 0, f"{bad.size} bytes of d_app differ, first at {bad[0]}"
        assert {ta.READ_END, ta.READ_FULL} <= set(want["stop"].tolist())
        for b in (d_reads, d_app, d_out):
            b.free()

    run_open(engine, c, OPEN_N, label="open N=257", after=gather)


@pytest.mark.parametrize("cut", ["W-1", "W//2", "1"])
def test_open_max_records_cut(engine, opens, cut):
    w = opens.framed
    m = {"W-1": w - 1, "W//2": w // 2, "1": 1}[cut]
    _, got = run_open(engine, opens, OPEN_N, max_records=m, label=f"open N=257 max_records={cut}")
    assert int(got["results"]["records"].sum()) == m and got["total"] == w

