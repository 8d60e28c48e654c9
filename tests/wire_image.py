"""Whole-image runs of tlsgpu_seal_wire / tlsgpu_open_wire over many streams: the
wire-path counterpart of batch_image.py.  The layout, the models of both calls
and the checkers live here; test_wire_image_model.py shows on the CPU that the
checkers can fail, test_gpu_wire_image.py drives the engine through them.

Conventions: d_wire is 0xA5 and d_data 0xC3 around every stream; stream regions
lie back to back with gaps of 0, 1, 2, 3 bytes in turn in both buffers (every
alignment modulo 16 occurs, some neighbours touch); both device buffers are
allocated 64 bytes beyond the wire_bytes / data_bytes the call is given, and that
slack must come back untouched; d_status starts from a sentinel; d_recs,
d_status and d_results are compared whole; every call runs twice on refilled
buffers and both runs must meet the model.

Record slots.  Slot bases come from atomics, so which range a stream gets is not
fixed once there is more than one wave (seal) or workgroup (open).  check_slots
validates the reported (first, records) of every stream without assuming an
order; the expected images are then built from the reported ranges.  Slots
outside all ranges hold all-ones descriptors and TLSGPU_REC_PUBLIC_INVALID.

The seal image, per stream and per record k at wire position pos with length
field L: the record fits the wire iff pos <= wire_bytes and 5 + L <= wire_bytes -
pos, it fits the data iff [data_off + k * frag, + len) lies in data_bytes; the
header is written iff it fits the wire, the fragment iff it fits both, otherwise
the status is TLSGPU_REC_OUT_OF_BOUNDS and no fragment byte changes; records,
wire_len and next_seq count such a record all the same.  Descriptor offsets
saturate at 2^64 - 1.

The open image is the input wire with, per framed record, the plaintext at
fragment + explicit nonce when the AEAD accepts (a plaintext above 16384 bytes
too), zeros there on a bad MAC, nothing for a publicly invalid record.  Records
behind a stream's first failure are TLSGPU_REC_SKIPPED: the open kernels run
before wire_finish_kernel, so their plaintext span may or may not have been
opened.  Exactly those spans are masked out of the comparison; their headers,
explicit nonces and tags are compared like every other byte.
"""
import bisect
from dataclasses import dataclass, field

import numpy as np

import pyoracle as po
import talos_amd as ta
from test_wire import model_stream

SENTINEL = 0x5A5A5A5A
SLACK = 64
WIRE_FILL, DATA_FILL = 0xA5, 0xC3
TLS12 = 0x0303
GCM = (po.AES_128_GCM, po.AES_256_GCM)
M64 = (1 << 64) - 1
TAG = 16


class Memo:
    """The oracle's TLS seal / open with every answer kept: the populations are
    used by prefix and under several cuts, each record is computed once."""

    def __init__(self, oracle):
        self.oracle, self.sealed, self.opened = oracle, {}, {}

    def tls_seal(self, sess, seq, rtype, pt):
        key = (id(sess), seq, rtype, pt)
        if key not in self.sealed:
            self.sealed[key] = self.oracle.tls_seal(sess, seq, rtype, pt)
        return self.sealed[key]

    def tls_open(self, sess, seq, rtype, frag):
        key = (id(sess), seq, rtype, frag)
        if key not in self.opened:
            self.opened[key] = self.oracle.tls_open(sess, seq, rtype, frag)
        return self.opened[key]


@dataclass
class Sess:
    kind: int
    params: object      # talos_amd.SessionParams
    osess: object       # the oracle's TLS session

    @property
    def eiv(self):
        return 8 if self.kind in GCM else 0


def make_sessions(oracle, kinds, seed):
    rng = np.random.default_rng(seed)
    out = []
    for k in kinds:
        key, fiv = rng.bytes(po.KEY_LEN[k]), rng.bytes(po.FIXED_IV_LEN[k])
        out.append(Sess(k, ta.SessionParams(k, key, fiv), oracle.tls_session(k, key, fiv)))
    return out


# -- the slot rule -----------------------------------------------------------------

def check_slots(wanted, results, max_records, total):
    """The reported (first, records) of every stream against the slot rule (module
    docstring).  wanted: per stream, the records it asks for (seal: already
    capped at max_records)."""
    first = [int(x) for x in results["first"]]
    records = [int(x) for x in results["records"]]
    assert len(wanted) == len(first)
    assert total == sum(wanted), ("total", total, "sum of wanted", sum(wanted))
    used = min(total, max_records)
    partial = []
    for i, (w, f, r) in enumerate(zip(wanted, first, records)):
        assert r <= w, ("stream", i, "records", r, "above wanted", w)
        if r == 0:
            assert f == 0, ("stream", i, "without records reports first", f)
            assert w == 0 or total > max_records, ("stream", i, "cut to nothing although all fit")
        elif r < w:
            partial.append(i)
    assert len(partial) <= 1, ("more than one partly cut stream", partial)
    for i in partial:
        assert first[i] + records[i] == max_records, (
            "stream", i, "partly cut, its range ends at", first[i] + records[i], "not at",
            max_records)
    at = 0
    for f, r, i in sorted((first[i], records[i], i) for i in range(len(first)) if records[i]):
        assert f >= at, ("stream", i, "range", (f, f + r), "overlaps the one before, which ends at", at)
        assert f == at, ("gap in the record slots", (at, f), "before stream", i)
        at = f + r
    assert at == used, ("the ranges end at", at, "not at", used)


def reordered(results):
    """Some stream with records got a lower range than a stream before it."""
    firsts = [int(f) for f, r in zip(results["first"], results["records"]) if r]
    return any(b < a for a, b in zip(firsts, firsts[1:]))


# -- what a call should leave ------------------------------------------------------

@dataclass
class Expected:
    wire: np.ndarray                    # wire_bytes + SLACK
    wire_bytes: int
    recs: np.ndarray                    # RECORD_DTYPE x max_records
    status: np.ndarray                  # int32 x max_records
    results: np.ndarray                 # one per stream
    wanted: list
    mask: np.ndarray = None             # wire bytes left out of the comparison
    spans: list = field(default_factory=list)    # (start, end, what) of the wire, sorted
    owner: dict = field(default_factory=dict)    # slot -> (stream, record)

    def where(self, at):
        if at >= self.wire_bytes:
            return "slack behind wire_bytes"
        k = bisect.bisect_right(self.spans, (at, 1 << 70, "")) - 1
        while k >= 0:                   # the innermost span that holds the byte
            lo, hi, what = self.spans[k]
            if lo <= at < hi:
                return f"{what} + {at - lo}"
            k -= 1
        return "outside every stream (gap or unwritten)"

    def slot(self, j):
        return "stream %d record %d" % self.owner[j] if j in self.owner else "unused slot"


def compare(exp, got, label=None):
    """got: dict(wire, recs, status, results, total) as downloaded, whole."""
    for f in exp.results.dtype.names:
        bad = np.flatnonzero((exp.results[f] != got["results"][f]).reshape(len(exp.results), -1)
                             .any(axis=1))
        assert bad.size == 0, (label, "result field", f, "stream", int(bad[0]), "got",
                               got["results"][f][bad[0]].tolist(), "expected",
                               exp.results[f][bad[0]].tolist())
    a, b = got["recs"].view(np.uint8).reshape(-1, 32), exp.recs.view(np.uint8).reshape(-1, 32)
    assert a.shape == b.shape, (label, "descriptor slots", a.shape, b.shape)
    bad = np.flatnonzero((a != b).any(axis=1))
    if bad.size:
        j = int(bad[0])
        raise AssertionError((label, "descriptor", j, exp.slot(j), "byte",
                              int(np.flatnonzero(a[j] != b[j])[0]), "got", got["recs"][j].tolist(),
                              "expected", exp.recs[j].tolist(), "differing slots", int(bad.size)))
    assert got["status"].shape == exp.status.shape
    bad = np.flatnonzero(got["status"] != exp.status)
    if bad.size:
        j = int(bad[0])
        raise AssertionError((label, "status", j, exp.slot(j), "got", int(got["status"][j]),
                              "expected", int(exp.status[j]), "differing", int(bad.size)))
    assert got["wire"].shape == exp.wire.shape
    diff = got["wire"] != exp.wire
    if exp.mask is not None:
        diff &= ~exp.mask
    bad = np.flatnonzero(diff)
    if bad.size:
        at = int(bad[0])
        raise AssertionError((label, "wire byte", at, exp.where(at), "got", int(got["wire"][at]),
                              "expected", int(exp.wire[at]), "differing bytes", int(bad.size)))


def same_but_slots(a, b, max_records, mask=None, label=None):
    """Two runs of one call differ in the slot assignment only: where nothing is cut
    (under a cut, which stream loses records may differ too), the wire outside the
    masked spans and every result field but `first` are the same."""
    if a["total"] != b["total"] or a["total"] > max_records:
        assert a["total"] == b["total"], (label, "totals differ", a["total"], b["total"])
        return
    diff = a["wire"] != b["wire"]
    if mask is not None:
        diff &= ~mask
    assert not diff.any(), (label, "the two runs' wires differ at", int(np.flatnonzero(diff)[0]))
    for f in a["results"].dtype.names:
        if f != "first":
            assert np.array_equal(a["results"][f], b["results"][f]), (label, "the two runs differ in", f)


def _unused(max_records):
    recs = np.frombuffer(b"\xFF" * (32 * max_records), dtype=ta.RECORD_DTYPE).copy()
    return recs, np.full(max_records, ta.REC_PUBLIC_INVALID, dtype=np.int32)


# -- tlsgpu_seal_wire --------------------------------------------------------------

@dataclass
class WStream:
    data: bytes
    session: int
    seq: int
    rtype: int
    mf: int                     # max_fragment as the descriptor has it
    data_len: int = None        # what the descriptor says (default: len(data))
    data_off: int = None        # in place of the layout's offsets
    wire_off: int = None
    region: int = None          # wire bytes the layout keeps for it (default: all it writes)


def frag_of(mf):
    return 16384 if mf == 0 or mf > 16384 else mf


def stream_size(s, sessions, n=None):
    """Wire bytes of the stream's first n records (default: all)."""
    frag = frag_of(s.mf)
    eiv = sessions[s.session].eiv if s.session < len(sessions) else 8
    total = len(s.data) if s.data_len is None else s.data_len
    nrec = -(-total // frag)
    n = nrec if n is None else min(n, nrec)
    return sum(5 + eiv + min(frag, total - k * frag) + TAG for k in range(n))


@dataclass
class SealLayout:
    desc: np.ndarray            # WRITE_STREAM_DTYPE
    data: np.ndarray            # data_bytes + SLACK
    data_bytes: int
    wire_bytes: int
    laid: list                  # (data offset, wire offset) the layout gave each stream
    wire_alloc: int = 0         # bytes of the device wire buffer: the layout's end + SLACK, kept
                                # when a test lowers wire_bytes (the data buffer: data.nbytes)


def layout_seal(streams, sessions):
    desc = np.zeros(len(streams), dtype=ta.WRITE_STREAM_DTYPE)
    laid, dpos, wpos, chunks = [], 0, 0, []
    for i, s in enumerate(streams):
        dpos += i % 4
        wpos += i % 4
        laid.append((dpos, wpos))
        desc[i] = (dpos if s.data_off is None else s.data_off,
                   wpos if s.wire_off is None else s.wire_off, s.seq,
                   len(s.data) if s.data_len is None else s.data_len, s.session, TLS12, s.rtype, 0,
                   s.mf)
        chunks.append((dpos, s.data))
        dpos += len(s.data)
        wpos += stream_size(s, sessions) if s.region is None else s.region
    data = np.full(dpos + SLACK, DATA_FILL, dtype=np.uint8)
    for o, d in chunks:
        data[o:o + len(d)] = np.frombuffer(d, dtype=np.uint8)
    return SealLayout(desc, data, dpos, wpos, laid, wpos + SLACK)


def seal_wanted(lay, sessions, max_records):
    out = []
    for d in lay.desc:
        known = int(d["session"]) < len(sessions)
        n = -(-int(d["data_len"]) // frag_of(int(d["max_fragment"]))) if known else 0
        out.append(min(n, max_records))
    return out


def seal_expect(memo, sessions, lay, max_records, results):
    """The image of a tlsgpu_seal_wire over `lay`, with every stream's slots where
    `results` reports them (check_slots has validated those)."""
    wb, db = lay.wire_bytes, lay.data_bytes
    wire = np.full(lay.wire_alloc, WIRE_FILL, dtype=np.uint8)
    recs, status = _unused(max_records)
    res = np.zeros(len(lay.desc), dtype=ta.WRITE_RESULT_DTYPE)
    exp = Expected(wire, wb, recs, status, res, seal_wanted(lay, sessions, max_records))
    for i, d in enumerate(lay.desc):
        first, n = int(results[i]["first"]), int(results[i]["records"])
        doff, pos, seq, dlen, sid, rtype, frag = (
            int(d["data_off"]), int(d["wire_off"]), int(d["seq"]), int(d["data_len"]),
            int(d["session"]), int(d["type"]), frag_of(int(d["max_fragment"])))
        ver = int(d["version"])
        for k in range(n):
            s = sessions[sid]
            ln = min(frag, dlen - k * frag)
            L = s.eiv + ln + TAG
            in_off = doff + k * frag
            fits_wire = pos <= wb and 5 + L <= wb - pos
            fits_data = in_off <= db and ln <= db - in_off
            if fits_wire:
                wire[pos:pos + 5] = (rtype, ver >> 8, ver & 0xFF, L >> 8, L & 0xFF)
                exp.spans.append((pos, pos + 5, f"stream {i} record {k} header"))
                exp.spans.append((pos + 5, pos + 5 + L, f"stream {i} record {k} fragment"))
            if fits_wire and fits_data:
                body = memo.tls_seal(s.osess, (seq + k) & M64, rtype,
                                     lay.data[in_off:in_off + ln].tobytes())
                assert len(body) == L
                wire[pos + 5:pos + 5 + L] = np.frombuffer(body, dtype=np.uint8)
                status[first + k] = L
            else:
                status[first + k] = ta.REC_OUT_OF_BOUNDS
            recs[first + k] = (min(in_off, M64), min(pos + 5, M64), (seq + k) & M64, sid,
                               ta.len_type(ln, rtype))
            exp.owner[first + k] = (i, k)
            pos += 5 + L
        res[i] = (first, n, (pos - int(d["wire_off"])) & M64, (seq + n) & M64, 0)
    exp.spans.sort()
    return exp


def run_seal(engine, table, memo, sessions, lay, max_records, label=None, null_recs=False,
             after=None):
    """tlsgpu_seal_wire over `lay`, twice, everything compared (module docstring).
    null_recs: d_recs / d_status are null (max_records must be 0).  after(got): called
    with the second run's downloads.  Returns them, with `reordered` (either run)."""
    n = len(lay.desc)
    assert n and not (null_recs and max_records)
    B = lambda nbytes: ta.DeviceBuffer(engine, nbytes)  # noqa: E731
    d_data, d_wire, d_streams, d_results, d_total = (
        B(lay.data.nbytes), B(lay.wire_alloc), B(lay.desc.nbytes), B(32 * n), B(4))
    d_recs, d_status = (None, None) if null_recs else (B(32 * max_records), B(4 * max_records))
    d_streams.upload(lay.desc.view(np.uint8))
    wanted = seal_wanted(lay, sessions, max_records)
    seen, got, before = False, None, None
    try:
        for run in range(2):
            before = got
            d_data.upload(lay.data)
            d_wire.fill(WIRE_FILL)
            d_results.fill(0xEE)
            d_total.fill(0xEE)
            if max_records:
                d_recs.fill(0x11)
                d_status.upload(np.full(max_records, SENTINEL, dtype=np.uint32).view(np.uint8))
            ta.seal_wire(table, d_streams.ptr, n, d_data.ptr, lay.data_bytes, d_wire.ptr,
                         lay.wire_bytes, max_records, d_recs.ptr if d_recs else None,
                         d_status.ptr if d_status else None, d_results.ptr, d_total.ptr)
            engine.sync()
            got = dict(
                wire=d_wire.download(),
                recs=(d_recs.download().view(ta.RECORD_DTYPE)[:max_records].copy() if max_records
                      else np.zeros(0, dtype=ta.RECORD_DTYPE)),
                status=(d_status.download().view(np.int32)[:max_records].copy() if max_records
                        else np.zeros(0, dtype=np.int32)),
                results=d_results.download().view(ta.WRITE_RESULT_DTYPE).copy(),
                total=int(d_total.download().view(np.uint32)[0]))
            check_slots(wanted, got["results"], max_records, got["total"])
            compare(seal_expect(memo, sessions, lay, max_records, got["results"]), got,
                    (label, "run", run))
            assert np.array_equal(d_data.download(), lay.data), (label, "d_data changed")
            seen = seen or reordered(got["results"])
        same_but_slots(before, got, max_records, None, label)
        if after:
            after(got)
    finally:
        for b in (d_data, d_wire, d_streams, d_results, d_total, d_recs, d_status):
            if b:
                b.free()
    got["reordered"] = seen
    return got


# -- tlsgpu_open_wire --------------------------------------------------------------

@dataclass
class OpenLayout:
    streams: list               # test_wire.build_streams' dicts
    offs: list                  # each stream's wire_off
    wire: np.ndarray            # the input image, wire_bytes + SLACK
    wire_bytes: int


def layout_open(streams):
    offs, pos = [], 0
    for i, s in enumerate(streams):
        pos += i % 4
        offs.append(pos)
        pos += len(s["wire"])
    wire = np.full(pos + SLACK, WIRE_FILL, dtype=np.uint8)
    for o, s in zip(offs, streams):
        wire[o:o + len(s["wire"])] = np.frombuffer(s["wire"], dtype=np.uint8)
    return OpenLayout(streams, offs, wire, pos)


def open_descs(lay):
    descs = np.zeros(len(lay.streams), dtype=ta.WIRE_STREAM_DTYPE)
    for i, (o, s) in enumerate(zip(lay.offs, lay.streams)):
        descs[i] = (o, len(s["wire"]), s["session"], s["seq"], s["version"],
                    ta.WIRE_FIRST_PACKET if s["first"] else 0, s["rbuf"])
    return descs


def _model(memo, sessions, s, wire):
    known = s["session"] < len(sessions)
    return model_stream(memo, sessions[s["session"]].osess if known else None,
                        sessions[s["session"]].kind if known else 0, wire, s["version"],
                        s["first"], s["rbuf"], s["seq"])


def frames(wire, n):
    """(offset, type, length) of the first n records of a stream."""
    out, pos = [], 0
    for _ in range(n):
        ln = (wire[pos + 3] << 8) | wire[pos + 4]
        out.append((pos, wire[pos], ln))
        pos += 5 + ln
    return out, pos


def open_wanted(memo, sessions, lay):
    return [len(_model(memo, sessions, s, s["wire"])[0]) for s in lay.streams]


def open_expect(memo, sessions, lay, max_records, results):
    """The image of a tlsgpu_open_wire over `lay` from the reported slots.  A stream
    cut to fewer records than it frames is the model of exactly those records'
    bytes: no header alert is reached, delivered / alert / alert_record come from
    those records only, consumed is their bytes."""
    wire = lay.wire.copy()
    mask = np.zeros(len(wire), dtype=bool)
    recs, status = _unused(max_records)
    res = np.zeros(len(lay.streams), dtype=ta.WIRE_RESULT_DTYPE)
    exp = Expected(wire, lay.wire_bytes, recs, status, res, open_wanted(memo, sessions, lay), mask)
    for i, (off, s) in enumerate(zip(lay.offs, lay.streams)):
        first, n = int(results[i]["first"]), int(results[i]["records"])
        exp.spans.append((off, off + len(s["wire"]), f"stream {i} (behind its framed records)"))
        sw = s["wire"]
        if n < exp.wanted[i]:
            sw = sw[:frames(sw, n)[1]]
        out, consumed, alert, alert_rec, delivered = _model(memo, sessions, s, sw)
        assert len(out) == n
        known = s["session"] < len(sessions)
        eiv = sessions[s["session"]].eiv if known else 0
        for k, ((st, _), (p, rtype, ln)) in enumerate(zip(out, frames(sw, n)[0])):
            fo = off + p + 5
            npt = max(ln - eiv - TAG, 0)
            exp.spans += [(off + p, fo, f"stream {i} record {k} header"),
                          (fo, fo + ln, f"stream {i} record {k} fragment")]
            if st == ta.REC_SKIPPED:
                mask[fo + eiv:fo + eiv + npt] = True
            elif st == ta.REC_BAD_MAC:
                wire[fo + eiv:fo + eiv + npt] = 0
            elif st != ta.REC_PUBLIC_INVALID:       # delivered, or opened and then too long
                r, pt = memo.tls_open(sessions[s["session"]].osess, s["seq"] + k, rtype,
                                      bytes(sw[p + 5:p + 5 + ln]))
                assert r == 1 and len(pt) == npt and (st == npt or st == ta.REC_OVERFLOW)
                wire[fo + eiv:fo + eiv + npt] = np.frombuffer(pt, dtype=np.uint8)
            status[first + k] = st
            recs[first + k] = (fo, fo + eiv, (s["seq"] + k) & M64, s["session"], (rtype << 24) | ln)
            exp.owner[first + k] = (i, k)
        res[i] = (first, n, delivered, consumed, alert, alert_rec, (0, 0))
    exp.spans.sort()
    return exp


def run_open(engine, table, memo, sessions, lay, max_records, label=None, after=None):
    """tlsgpu_open_wire over `lay`, twice, everything compared.  after(got, dev): called
    after the second run with its downloads and the live device buffers (dict)."""
    n = len(lay.streams)
    assert n and max_records
    descs = open_descs(lay)
    B = lambda nbytes: ta.DeviceBuffer(engine, nbytes)  # noqa: E731
    d_wire, d_streams, d_recs, d_status, d_results, d_total = (
        B(lay.wire.nbytes), B(descs.nbytes), B(32 * max_records), B(4 * max_records), B(32 * n), B(4))
    d_streams.upload(descs.view(np.uint8))
    wanted = open_wanted(memo, sessions, lay)
    seen, got, before, exp = False, None, None, None
    try:
        for run in range(2):
            before = got
            d_wire.upload(lay.wire)
            d_recs.fill(0x11)
            d_status.upload(np.full(max_records, SENTINEL, dtype=np.uint32).view(np.uint8))
            d_results.fill(0xEE)
            d_total.fill(0xEE)
            ta.open_wire(table, d_streams.ptr, n, d_wire.ptr, max_records, d_recs.ptr,
                         d_status.ptr, d_results.ptr, d_total.ptr)
            engine.sync()
            got = dict(wire=d_wire.download(),
                       recs=d_recs.download().view(ta.RECORD_DTYPE)[:max_records].copy(),
                       status=d_status.download().view(np.int32)[:max_records].copy(),
                       results=d_results.download().view(ta.WIRE_RESULT_DTYPE).copy(),
                       total=int(d_total.download().view(np.uint32)[0]))
            check_slots(wanted, got["results"], max_records, got["total"])
            exp = open_expect(memo, sessions, lay, max_records, got["results"])
            compare(exp, got, (label, "run", run))
            seen = seen or reordered(got["results"])
        same_but_slots(before, got, max_records, exp.mask, label)
        if after:
            after(got, dict(wire=d_wire, streams=d_streams, recs=d_recs, status=d_status,
                            results=d_results, descs=descs))
    finally:
        for b in (d_wire, d_streams, d_recs, d_status, d_results, d_total):
            b.free()
    got["reordered"] = seen
    return got
