"""The rule of tlsgpu_read_wire (include/tlsgpu.h "One-call wire read path"),
restated over host arrays: the streams and reads of a call, the input wire, and
per record the AEAD's verdict and plaintext.  Nothing here decrypts, so every
comparison with the device is exact.

Framing is test_wire.model_stream's header walk (ssl3_get_record); the same
function, driven by the verdict table instead of the oracle, is the open and the
finish over the records the plan kept.  Between the two stands the plan, which
is the new part: see read_model.

Record slots come from an atomic per workgroup, so which range a stream gets is
not fixed once a call has more than four streams.  check_read_slots validates
the reported ranges without assuming an order; the expected images are then built
from them, as wire_image.py does.
"""
from dataclasses import dataclass

import numpy as np

import talos_amd as ta
from test_wire import model_stream
from wire_image import check_slots, frames

APP_DATA = 23
OK, BAD_MAC = 1, -1
GCM = (ta.AES_128_GCM, ta.AES_256_GCM)
M64 = (1 << 64) - 1


def overhead(kind, tag_len=16):
    """(explicit nonce, tag) bytes of a session of `kind`.  (A stream of an unknown
    session has None in their place: the plan counts no overhead for it.)"""
    return (8 if kind in GCM else 0), tag_len


class Verdicts:
    """model_stream's `oracle` without a cipher: tls_open answers from a table
    {(stream, record): (OK, plaintext) | (BAD_MAC, None)}.  A fragment shorter
    than explicit nonce + tag is publicly invalid whatever the table says."""

    def __init__(self, table, over):
        self.table, self.over = table, over

    def tls_open(self, key, seq, rtype, frag):
        s, seq0 = key
        if len(frag) < sum(self.over[s]):
            return 0, b""
        est, pt = self.table[(s, (seq - seq0) & M64)]
        return (1, pt) if est == OK else (-1, b"")


class _Accept:
    """Every record verifies: model_stream is then the header walk alone."""

    @staticmethod
    def tls_open(key, seq, rtype, frag):
        return 1, b""


def stream_bytes(wire, st):
    off, n = int(st["wire_off"]), int(st["wire_len"])
    return wire[off:off + n].tobytes()


def walk(wire, st):
    """Framing of one stream: ([(offset, type, length)], consumed, header alert)."""
    sw = stream_bytes(wire, st)
    out, consumed, alert, _, _ = model_stream(_Accept, (0, 0), 0, sw, int(st["version"]),
                                              bool(int(st["flags"]) & ta.WIRE_FIRST_PACKET),
                                              int(st["rbuf_len"]), 0)
    return frames(sw, len(out))[0], consumed, alert


def wanted_records(wire, streams):
    return [len(walk(wire, st)[0]) for st in streams]


def check_read_slots(wanted, results, max_records, total):
    """The reported `first` of every stream against the slot rule; returns the
    records framing kept per stream.  All records fit (total <= max_records): a
    stream's reserved range is (first, wanted) even where the plan cut it, to
    nothing too, and the ranges of the streams that framed records tile [0, total)
    in some order.  Otherwise the caller guarantees that the plan cut nothing, so
    `records` is framing's and wire_image.check_slots applies as it stands."""
    assert total == sum(wanted), ("total", total, "sum of wanted", sum(wanted))
    if total > max_records:
        check_slots(wanted, results, max_records, total)
        return [int(r) for r in results["records"]]
    at = 0
    for f, w, i in sorted((int(results[i]["first"]), w, i) for i, w in enumerate(wanted) if w):
        assert f == at, ("stream", i, "range starts at", f, "not at", at)
        at = f + w
    assert at == total
    for i, w in enumerate(wanted):
        assert w or int(results[i]["first"]) == 0, ("stream", i, "without records reports first")
        assert int(results[i]["records"]) <= w
    return list(wanted)


def slots_in_order(wanted, max_records):
    """(first, kept) per stream when the ranges are handed out in stream order."""
    out, at = [], 0
    for w in wanted:
        k = max(0, min(w, max_records - at))
        out.append((at if k else 0, k))
        at += w
    return out


@dataclass
class ReadExpected:
    recs: np.ndarray            # RECORD_DTYPE x max_records
    status: np.ndarray          # int32 x max_records
    results: np.ndarray         # WIRE_RESULT_DTYPE per stream
    reads: np.ndarray           # READ_RESULT_DTYPE per stream
    app: np.ndarray             # the whole application buffer after the call
    mask: np.ndarray            # bool per byte of app: the unspecified ranges, and no more
    total: int
    placed: list                # per stream, T: the plaintext bytes the plan placed


def read_model(streams, reads, wire, wire_bytes, over, verdicts, slots, max_records, app, app_bytes):
    """streams / reads: WIRE_STREAM_DTYPE / READ_STREAM_DTYPE arrays; wire: the input
    wire as allocated (uint8), wire_bytes what the call is told; over: per stream
    (explicit nonce, tag) as overhead() gives it, None for an unknown session; verdicts: the Verdicts table;
    slots: per stream (first, records framing kept); app: the application buffer as
    allocated before the call, app_bytes what the call is told."""
    app = np.array(app, dtype=np.uint8, copy=True)
    mask = np.zeros(len(app), dtype=bool)
    recs = np.frombuffer(b"\xFF" * (32 * max_records), dtype=ta.RECORD_DTYPE).copy()
    status = np.full(max_records, ta.REC_PUBLIC_INVALID, dtype=np.int32)
    res = np.zeros(len(streams), dtype=ta.WIRE_RESULT_DTYPE)
    out = np.zeros(len(streams), dtype=ta.READ_RESULT_DTYPE)
    oracle = Verdicts(verdicts, over)
    total, placed = 0, []
    for s, (st, rd) in enumerate(zip(streams, reads)):
        woff, seq0, sid = int(st["wire_off"]), int(st["seq"]), int(st["session"])
        app_off, cap, start = (int(rd[f]) for f in ("app_off", "app_cap", "start"))
        eiv, tag = over[s] or (0, 0)
        first, kept = slots[s]
        walked = walk(wire, st)[0]
        total += len(walked)
        framed = walked[:kept]          # max_records truncates at a record boundary
        # -- the plan
        room = 0 if app_off > app_bytes else min(cap, app_bytes - app_off)
        T, cut, stop, stop_type, stop_len, offs = 0, None, ta.READ_END, 0, 0, []
        if start != 0:
            cut, stop = 0, ta.READ_OUT_OF_BOUNDS
        else:
            for i, (p, rtype, ln) in enumerate(framed):
                in_off, pi = woff + p + 5, max(0, ln - eiv - tag)
                if in_off > wire_bytes or ln > wire_bytes - in_off:
                    cut, stop = i, ta.READ_OUT_OF_BOUNDS
                elif rtype != APP_DATA:
                    cut, stop, stop_type, stop_len = i, ta.READ_NOT_APP_DATA, rtype, pi
                elif T + pi > room:
                    cut, stop, stop_type, stop_len = i, ta.READ_FULL, APP_DATA, pi
                if cut is not None:
                    break
                offs.append(min(app_off, app_bytes) + T)    # (past the end: empty records only)
                T += pi
        if cut is not None:             # wire_peek.hip's cut
            framed = framed[:cut]
        placed.append(T)
        n = len(framed)
        # -- the open and the finish: ssl3_get_record over the records kept.  A stream
        # cut short, by max_records or by the plan, is the model of exactly those
        # records' bytes: no header alert is reached, consumed is their bytes
        sw = stream_bytes(wire, st)
        if n < len(walked):
            sw = sw[:framed[-1][0] + 5 + framed[-1][2]] if n else b""
        opened, consumed, alert, alert_rec, delivered = model_stream(
            oracle, (s, seq0) if over[s] is not None else None, 0, sw, int(st["version"]),
            bool(int(st["flags"]) & ta.WIRE_FIRST_PACKET), int(st["rbuf_len"]), seq0)
        assert len(opened) == n, (s, len(opened), n)
        app_len = 0
        for k, ((stt, pt), (p, rtype, ln)) in enumerate(zip(opened, framed)):
            pk = max(0, ln - eiv - tag)
            if stt == ta.REC_BAD_MAC:
                app[offs[k]:offs[k] + pk] = 0
            elif stt not in (ta.REC_SKIPPED, ta.REC_PUBLIC_INVALID):
                if stt == ta.REC_OVERFLOW:      # opened, and then too long
                    pt = verdicts[(s, k)][1]
                assert len(pt) == pk, (s, k, len(pt), pk)
                app[offs[k]:offs[k] + pk] = np.frombuffer(pt, dtype=np.uint8)
            if k < delivered:
                app_len += stt
            status[first + k] = stt
            recs[first + k] = (woff + p + 5, offs[k], (seq0 + k) & M64, sid, (rtype << 24) | ln)
        mask[app_off + app_len:app_off + T] = True
        res[s] = (first, n, delivered, consumed, alert, alert_rec, (0, 0))
        # -- the read result
        r = out[s]
        r["app_len"], r["records"], r["next"] = app_len, delivered, delivered
        if delivered:
            p, _, ln = framed[delivered - 1]
            r["consumed"] = p + 5 + ln
        if delivered == n:
            r["stop"], r["stop_type"], r["stop_len"] = stop, stop_type, stop_len
    return ReadExpected(recs, status, res, out, app, mask, total, placed)


def compare_read(exp, got, label=None):
    """got: dict(recs, status, results, reads, app, total) as downloaded, whole.  Every
    field and every byte, but the bytes of d_app under exp.mask."""
    assert got["total"] == exp.total, (label, "d_total", got["total"], exp.total)
    for name, want in (("results", exp.results), ("reads", exp.reads)):
        for f in want.dtype.names:
            a, b = got[name][f].reshape(len(want), -1), want[f].reshape(len(want), -1)
            bad = np.flatnonzero((a != b).any(axis=1))
            assert bad.size == 0, (label, name, f, "stream", int(bad[0]), "got", a[bad[0]].tolist(),
                                   "expected", b[bad[0]].tolist())
    a, b = got["recs"].view(np.uint8).reshape(-1, 32), exp.recs.view(np.uint8).reshape(-1, 32)
    assert a.shape == b.shape, (label, "descriptor slots", a.shape, b.shape)
    bad = np.flatnonzero((a != b).any(axis=1))
    assert bad.size == 0, (label, "descriptor", int(bad[0]), "got", got["recs"][bad[0]].tolist(),
                           "expected", exp.recs[bad[0]].tolist(), "differing", int(bad.size))
    assert got["status"].shape == exp.status.shape
    bad = np.flatnonzero(got["status"] != exp.status)
    assert bad.size == 0, (label, "status", int(bad[0]), "got", int(got["status"][bad[0]]),
                           "expected", int(exp.status[bad[0]]), "differing", int(bad.size))
    assert got["app"].shape == exp.app.shape
    bad = np.flatnonzero((got["app"] != exp.app) & ~exp.mask)
    assert bad.size == 0, (label, "d_app byte", int(bad[0]), "got", int(got["app"][bad[0]]),
                           "expected", int(exp.app[bad[0]]), "differing bytes", int(bad.size))
