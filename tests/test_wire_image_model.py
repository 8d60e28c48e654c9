"""wire_image.py's checkers on the CPU: they accept what the rules allow and they
fail, naming the place, on each corruption a wrong kernel could leave.  (The GPU
tests in test_gpu_wire_image.py would show nothing if these could not fail.)
"""
import itertools
import random

import numpy as np
import pytest

import pyoracle as po
import talos_amd as ta
import wire_image as wi
from test_seal_wire import model_write
from test_wire import build_streams


def results_of(pairs, dtype=ta.WRITE_RESULT_DTYPE):
    r = np.zeros(len(pairs), dtype=dtype)
    for i, (f, n) in enumerate(pairs):
        r[i]["first"], r[i]["records"] = f, n
    return r


def in_order(wanted, order, max_records):
    """(first, records) per stream when the streams reserve their slots in `order`."""
    out, at = [None] * len(wanted), 0
    for i in order:
        n = max(min(wanted[i], max_records - at), 0) if at < max_records else 0
        out[i] = (at if n else 0, n)
        at += wanted[i]
    return out


# -- check_slots ---------------------------------------------------------------------

@pytest.mark.parametrize("wanted", [[3, 0, 2, 5], [1, 1, 1], [4, 4, 0, 0, 1]])
def test_check_slots_accepts_every_reservation_order(wanted):
    total = sum(wanted)
    for m in {total + 3, total, total - 1, total // 2, 1}:
        for order in itertools.permutations(range(len(wanted))):
            wi.check_slots(wanted, results_of(in_order(wanted, order, m)), m, total)


def rejects(wanted, pairs, max_records, total, word):
    with pytest.raises(AssertionError) as e:
        wi.check_slots(wanted, results_of(pairs), max_records, total)
    assert word in str(e.value), str(e.value)


def test_check_slots_rejects():
    w = [3, 2, 4]
    wi.check_slots(w, results_of([(0, 3), (3, 2), (5, 4)]), 16, 9)
    rejects(w, [(0, 3), (2, 2), (5, 4)], 16, 9, "overlaps")
    rejects(w, [(0, 3), (4, 2), (6, 4)], 16, 9, "gap")
    rejects(w, [(0, 3), (3, 2), (5, 4)], 16, 8, "total")
    rejects(w, [(0, 3), (3, 2), (5, 5)], 16, 9, "above wanted")
    # cut at 7: the last stream keeps 2 of its 4 records
    wi.check_slots(w, results_of([(0, 3), (3, 2), (5, 2)]), 7, 9)
    rejects(w, [(0, 3), (3, 2), (5, 1)], 7, 9, "partly cut")            # ends at 6, not at 7
    rejects(w, [(0, 2), (2, 2), (4, 3)], 7, 9, "more than one partly cut")
    rejects(w, [(0, 3), (3, 2), (5, 4)], 7, 9, "not at")                # runs past max_records
    # a stream cut to nothing reports first == 0, and only under a cut
    wi.check_slots(w, results_of([(0, 3), (3, 2), (0, 0)]), 5, 9)
    rejects(w, [(0, 3), (3, 2), (5, 0)], 5, 9, "without records reports first")
    rejects(w, [(0, 3), (3, 2), (0, 0)], 16, 9, "cut to nothing")


# -- the seal image ------------------------------------------------------------------

KINDS = [po.AES_128_GCM, po.CHACHA20_POLY1305, po.AES_256_GCM, po.CHACHA20_POLY1305_OLD]


@pytest.fixture(scope="module")
def seal_case(oracle):
    sessions = wi.make_sessions(oracle, KINDS, 5)
    rng = np.random.default_rng(6)
    sizes, frags = [0, 1, 100, 1400, 40, 16385, 3], [0, 0, 7, 512, 1, 0, 20000]
    streams = [wi.WStream(rng.bytes(n), i % 4, (1 << 63) + 1000 * i, 23 if i % 4 else 22, mf)
               for i, (n, mf) in enumerate(zip(sizes, frags))]
    lay = wi.layout_seal(streams, sessions)
    wanted = wi.seal_wanted(lay, sessions, 1 << 30)
    return sessions, streams, lay, wanted, wi.Memo(oracle)


def fake(exp, total):
    return dict(wire=exp.wire.copy(), recs=exp.recs.copy(), status=exp.status.copy(),
                results=exp.results.copy(), total=total)


def test_seal_image_is_model_write_at_the_stream_offsets(oracle, seal_case):
    sessions, streams, lay, wanted, memo = seal_case
    assert [o % 4 for _, o in lay.laid[:4]] != [0] * 4 and lay.laid[0] == (0, 0)
    res = results_of(in_order(wanted, range(len(wanted)), sum(wanted)))
    exp = wi.seal_expect(memo, sessions, lay, sum(wanted) + 2, res)
    image = np.full(lay.wire_bytes + wi.SLACK, wi.WIRE_FILL, dtype=np.uint8)
    for s, (_, woff), r in zip(streams, lay.laid, exp.results):
        out, k = model_write(oracle, sessions[s.session].osess, s.data, s.seq, s.rtype, wi.TLS12,
                             0 if s.mf > 16384 else s.mf)
        image[woff:woff + len(out)] = np.frombuffer(out, dtype=np.uint8)
        assert (int(r["records"]), int(r["wire_len"]), int(r["next_seq"])) == (k, len(out), s.seq + k)
        assert len(out) == wi.stream_size(s, sessions)
    assert np.array_equal(exp.wire, image)
    assert (exp.status[:sum(wanted)] > 0).all() and (exp.status[sum(wanted):] == ta.REC_PUBLIC_INVALID).all()
    assert (exp.recs[sum(wanted):].view(np.uint8) == 0xFF).all()
    wi.compare(exp, fake(exp, sum(wanted)))


def test_seal_image_comparison_names_the_place(seal_case):
    sessions, streams, lay, wanted, memo = seal_case
    n = sum(wanted)
    # the slots in another order than the streams: the image follows the reported ranges
    res = results_of(in_order(wanted, reversed(range(len(wanted))), n))
    exp = wi.seal_expect(memo, sessions, lay, n + 2, res)

    def fails(change, *words):
        got = fake(exp, n)
        change(got)
        with pytest.raises(AssertionError) as e:
            wi.compare(exp, got)
        for w in words:
            assert w in str(e.value), str(e.value)

    def poke(name, at):
        def change(got):
            a = got[name].view(np.uint8)
            a[at] ^= 0x40
        return change

    gap = lay.laid[2][1] - 1            # one of the two bytes between stream 1 and stream 2
    assert lay.laid[1][1] + wi.stream_size(streams[1], sessions) == gap - 1
    fails(poke("wire", gap), "wire byte", "outside every stream")
    fails(poke("wire", lay.wire_bytes + 5), "slack")
    fails(poke("wire", lay.laid[3][1] + 3), "stream 3 record 0 header + 3")
    fails(poke("wire", lay.laid[3][1] + 5 + 512 + 16 + 5 + 9), "stream 3 record 1 fragment + 9")
    fails(poke("recs", 32 * n + 17), "descriptor", "unused slot")
    fails(poke("recs", 32 * int(res[5]["first"]) + 8), "descriptor", "stream 5 record 0")
    fails(poke("status", 4 * (n + 1)), "status", "unused slot")
    fails(poke("status", 4 * int(res[2]["first"])), "status", "stream 2 record 0")
    fails(poke("results", 32 * 4 + 8), "result field", "wire_len", "'stream', 4")


def test_two_runs_may_differ_in_slots_only(seal_case):
    sessions, streams, lay, wanted, memo = seal_case
    n = sum(wanted)
    runs = [fake(wi.seal_expect(memo, sessions, lay, n, results_of(in_order(wanted, order, n))), n)
            for order in (range(len(wanted)), reversed(range(len(wanted))))]
    assert not np.array_equal(runs[0]["results"]["first"], runs[1]["results"]["first"])
    wi.same_but_slots(runs[0], runs[1], n)
    runs[1]["wire"][lay.laid[3][1] + 40] ^= 1
    with pytest.raises(AssertionError):
        wi.same_but_slots(runs[0], runs[1], n)
    mask = np.zeros(len(runs[1]["wire"]), dtype=bool)
    mask[lay.laid[3][1] + 40] = True
    wi.same_but_slots(runs[0], runs[1], n, mask)
    runs[1]["results"][2]["next_seq"] += 1
    with pytest.raises(AssertionError):
        wi.same_but_slots(runs[0], runs[1], n, mask)


def test_seal_image_out_of_bounds_rules(seal_case):
    """The header iff the record fits the wire, the fragment iff it fits both; the
    results count the record anyway; offsets saturate."""
    sessions, streams, lay, wanted, memo = seal_case
    import copy
    n = sum(wanted)
    res = results_of(in_order(wanted, range(len(wanted)), n))
    whole = wi.seal_expect(memo, sessions, lay, n, res)
    cut = copy.copy(lay)
    cut.data_bytes -= 1                 # the last stream (3 bytes, one record) loses a byte
    exp = wi.seal_expect(memo, sessions, cut, n, res)
    last = lay.laid[-1][1]
    assert np.array_equal(exp.wire[:last + 5], whole.wire[:last + 5])
    assert (exp.wire[last + 5:] == wi.WIRE_FILL).all() and exp.status[n - 1] == ta.REC_OUT_OF_BOUNDS
    assert np.array_equal(exp.results, whole.results)
    cut = copy.copy(lay)
    cut.wire_bytes -= 1
    exp = wi.seal_expect(memo, sessions, cut, n, res)
    assert (exp.wire[last:] == wi.WIRE_FILL).all() and exp.status[n - 1] == ta.REC_OUT_OF_BOUNDS
    assert np.array_equal(exp.results, whole.results)
    far = copy.copy(lay)
    far.desc = lay.desc.copy()
    far.desc[4]["wire_off"] = (1 << 64) - 4          # 40 one-byte records
    exp = wi.seal_expect(memo, sessions, far, n, res)
    f = int(res[4]["first"])
    assert (exp.status[f:f + 40] == ta.REC_OUT_OF_BOUNDS).all()
    assert (exp.recs[f:f + 40]["out_off"] == wi.M64).all()
    assert int(exp.results[4]["wire_len"]) == int(whole.results[4]["wire_len"])
    o = lay.laid[4][1]
    assert (exp.wire[o:o + int(whole.results[4]["wire_len"])] == wi.WIRE_FILL).all()


# -- the open image ------------------------------------------------------------------

def test_open_image_masks_only_the_plaintext_of_skipped_records(oracle):
    sessions = wi.make_sessions(oracle, [po.AES_128_GCM], 8)
    memo = wi.Memo(oracle)
    streams = build_streams(oracle, random.Random(3), sessions[0].osess, big=False)
    lay = wi.layout_open(streams)
    wanted = wi.open_wanted(memo, sessions, lay)
    n = sum(wanted)
    res = results_of(in_order(wanted, range(len(wanted)), n), ta.WIRE_RESULT_DTYPE)
    exp = wi.open_expect(memo, sessions, lay, n + 1, res)
    wi.compare(exp, fake(exp, n))
    # stream 1: six records, the fourth tampered -> bad_record_mac, records 4 and 5 skipped
    r = exp.results[1]
    assert (int(r["records"]), int(r["delivered"]), int(r["alert"])) == (6, 3, 20)
    f = int(r["first"])
    assert exp.status[f + 3:f + 6].tolist() == [ta.REC_BAD_MAC, ta.REC_SKIPPED, ta.REC_SKIPPED]
    assert exp.status[n] == ta.REC_PUBLIC_INVALID
    good, skipped = exp.recs[f + 1], exp.recs[f + 4]

    def outcome(at):
        got = fake(exp, n)
        got["wire"][at] ^= 1
        try:
            wi.compare(exp, got)
        except AssertionError as e:
            return str(e)
        return None

    ln = int(good["len_type"]) & 0xFFFFFF
    assert "stream 1 record 1 fragment" in outcome(int(good["in_off"]) + ln - 1)     # a tag byte
    assert "stream 1 record 1 fragment" in outcome(int(good["out_off"]))            # plaintext
    ln = int(skipped["len_type"]) & 0xFFFFFF
    assert "stream 1 record 4 header" in outcome(int(skipped["in_off"]) - 2)
    assert "stream 1 record 4 fragment + 0" in outcome(int(skipped["in_off"]))       # explicit nonce
    assert "stream 1 record 4 fragment" in outcome(int(skipped["in_off"]) + ln - 16)  # its tag
    assert outcome(int(skipped["out_off"])) is None                 # the plaintext span: masked
    assert outcome(int(skipped["in_off"]) + ln - 17) is None
    assert exp.mask.sum() == sum((int(d["len_type"]) & 0xFFFFFF) - 24 for d in exp.recs[f + 4:f + 6])
    # the incomplete tail behind stream 0's records and the gap before stream 1
    assert "stream 0 (behind" in outcome(lay.offs[0] + len(streams[0]["wire"]) - 1)
    assert "outside every stream" in outcome(lay.offs[1] - 1)


def test_open_image_of_a_cut_stream(oracle):
    """records < framed: consumed is exactly those records' bytes, no header alert is
    reached, and an AEAD failure counts only inside them."""
    sessions = wi.make_sessions(oracle, [po.AES_128_GCM], 8)
    memo = wi.Memo(oracle)
    streams = build_streams(oracle, random.Random(3), sessions[0].osess, big=False)[1:3]
    lay = wi.layout_open(streams)
    assert wi.open_wanted(memo, sessions, lay) == [6, 2]    # tampered 4th; wrong version on the 3rd
    for keep, alert, delivered in ((3, 0, 3), (4, 20, 3), (6, 20, 3)):
        res = results_of([(0, keep), (0, 0)], ta.WIRE_RESULT_DTYPE)
        wi.check_slots([6, 2], res, keep, 8)
        r = wi.open_expect(memo, sessions, lay, keep, res).results
        assert (int(r[0]["alert"]), int(r[0]["delivered"]), int(r[0]["alert_record"])) == \
            (alert, delivered, 3 if alert else keep)
        assert int(r[0]["consumed"]) == wi.frames(streams[0]["wire"], keep)[1]
        assert (int(r[1]["alert"]), int(r[1]["consumed"]), int(r[1]["records"])) == (0, 0, 0)
    res = results_of([(0, 6), (6, 2)], ta.WIRE_RESULT_DTYPE)
    r = wi.open_expect(memo, sessions, lay, 8, res).results
    assert int(r[1]["alert"]) == 70 and int(r[1]["delivered"]) == 2
