"""The KeyUpdate cut of tlsgpu_open_wire without a GPU: the rule's model
(wire_key_update_model.py) on hand-written streams, one for every key_update
value, and the parts of the ABI that need no device: the tlsgpu_wire_result
layout, the constants and the switch's argument check."""
import numpy as np
import pytest

import talos_amd as ta
import tls13_helper as t13
import wire_key_update_model as ku

@pytest.fixture(scope="module", params=sorted(ku.SUITES))
def gen(oracle, request):
    hashlen = 48 if request.param == "aes256" else 32
    return ku.Generation(oracle, request.param, bytes(range(7, 7 + hashlen)))


def fields(m):
    return tuple(m[f] for f in ("records", "delivered", "consumed", "alert", "alert_record",
                                "key_update"))


def test_predicate():
    ok = ku.looks_like_key_update
    assert ok(bytes.fromhex("180000010016")) and ok(bytes.fromhex("180000010116"))
    assert ok(bytes.fromhex("180000010016") + bytes(10))
    assert not ok(bytes.fromhex("180000010216"))            # request_update 2
    assert not ok(bytes.fromhex("180000010017"))            # byte 5 is not the handshake type
    assert not ok(bytes.fromhex("1800000100"))              # inner length 5
    assert not ok(bytes.fromhex("180000020016"))            # another length
    assert not ok(bytes.fromhex("190000010016"))            # another message
    assert not ok(bytes.fromhex("180000010016") + bytes(9) + b"\x01")   # byte 15
    assert not ok(bytes.fromhex("18000001001601"))          # byte 6


def test_keystream_is_the_first_cipher_block(oracle, gen):
    """Sealing zeros gives the keystream: XORed on any record's first 16 bytes it
    is that record's plaintext, whatever the record's length (the additional
    data does not enter a counter-mode keystream)."""
    for seq, n in ((0, 16), (5, 17), ((1 << 32) + 5, 600)):
        content = bytes((3 * i + seq) & 0xFF for i in range(n))
        w = gen.rec(seq, content)
        ks = ku.keystream16(oracle, gen.ctx, gen.iv, seq)
        assert bytes(a ^ b for a, b in zip(w[5:21], ks)) == (content + b"\x17")[:16]


def test_no_key_update_no_cut(gen):
    wire = b"".join(gen.rec(i, bytes(20 + i)) for i in range(4))
    on, off = gen.model(wire, 0, True), gen.model(wire, 0, False)
    assert fields(on) == fields(off) == (4, 4, len(wire), 0, 4, ku.KU_NONE)


@pytest.mark.parametrize("rr,pad", [(0, 0), (1, 0), (0, 9), (1, 10), (0, 11), (1, 506)])
def test_update_and_update_requested(gen, rr, pad):
    """data, data, KeyUpdate, then records under the next keys from seq 0."""
    nxt = gen.next()
    head = [gen.rec(7, b"a" * 30), gen.rec(8, b"b" * 3), gen.rec(9, ku.key_update_message(rr), 22, pad)]
    tail = [nxt.rec(0, b"c" * 40), nxt.rec(1, b"d" * 50)]
    wire = b"".join(head + tail)
    cut = sum(map(len, head))
    m = gen.model(wire, 7, True)
    assert fields(m) == (3, 3, cut, 0, 3, ku.KU_UPDATE + rr)
    assert m["walked"] == 5                      # d_total still counts the records behind the cut
    st, region, itype = m["recs"][2]
    assert (st, itype, region[:5]) == (5, 22, ku.key_update_message(rr))
    # the rest opens under the next generation, from sequence number 0
    m2 = nxt.model(wire[cut:], 0, True)
    assert fields(m2) == (2, 2, len(wire) - cut, 0, 2, ku.KU_NONE)
    assert [r[0] for r in m2["recs"]] == [40, 50]
    # switch off: today's outcome, bad_record_mac at the record behind the KeyUpdate
    assert fields(gen.model(wire, 7, False)) == (5, 3, len(wire), 20, 3, ku.KU_NONE)


def test_held_look_alike_application_data(gen):
    """Application data that begins like a KeyUpdate: a shorter batch, nothing
    else; the next call goes on under the same keys with seq + records."""
    look = bytes.fromhex("180000010016") + bytes(30)
    recs = [gen.rec(0, b"x" * 9), gen.rec(1, look), gen.rec(2, b"y" * 9), gen.rec(3, b"z" * 9)]
    wire = b"".join(recs)
    cut = len(recs[0]) + len(recs[1])
    m = gen.model(wire, 0, True)
    assert fields(m) == (2, 2, cut, 0, 2, ku.KU_HELD)
    assert m["recs"][1][0] == len(look) and m["recs"][1][2] == 23
    m2 = gen.model(wire[cut:], 0 + m["records"], True)
    assert fields(m2) == (2, 2, len(wire) - cut, 0, 2, ku.KU_NONE)


def test_held_forged_key_update(gen):
    """A true KeyUpdate with one tag bit flipped: alert 20 as usual, HELD."""
    k = bytearray(gen.rec(1, ku.key_update_message(0), 22))
    k[-1] ^= 0x10
    wire = gen.rec(0, b"x" * 9) + bytes(k) + gen.next().rec(0, b"y" * 9)
    m = gen.model(wire, 0, True)
    assert fields(m) == (2, 1, len(wire) - len(gen.rec(0, b"y" * 9)), 20, 1, ku.KU_HELD)


def test_held_handshake_record_with_more_content(gen):
    """18 00 00 01 00 16, ten zero bytes and four more content bytes in a type-22
    record: authentic, cut, but its content is not the 5-byte message."""
    content = bytes.fromhex("180000010016") + bytes(10) + b"\x01\x02\x03\x04"
    wire = gen.rec(0, content, 22) + gen.rec(1, b"y" * 9)
    m = gen.model(wire, 0, True)
    assert fields(m) == (1, 1, len(wire) - len(gen.rec(1, b"y" * 9)), 0, 1, ku.KU_HELD)
    assert m["recs"][0][0] == 20 and m["recs"][0][2] == 22


@pytest.mark.parametrize("inner", ["180000010216", "180000010017", "1800000116",
                                   "180000010016" + "00" * 9 + "17"])
def test_not_candidates(gen, inner):
    """request_update 2, byte 5 not 0x16, an inner plaintext of 5 bytes, a
    non-zero byte 15: the stream is not cut."""
    wire = gen.rec(0, b"x" * 9) + gen.rec(1, None, inner=bytes.fromhex(inner)) + gen.rec(2, b"y" * 9)
    on, off = gen.model(wire, 0, True), gen.model(wire, 0, False)
    assert fields(on) == fields(off) and on["key_update"] == ku.KU_NONE and on["records"] == 3


def test_header_alert_behind_the_cut_is_dropped(gen):
    bad = bytearray(gen.rec(2, b"y" * 9))
    bad[0] = 22                                   # a non-23 outer type: unexpected_message
    wire = gen.rec(0, b"x" * 9) + gen.rec(1, ku.key_update_message(1), 22) + bytes(bad)
    off = gen.model(wire, 0, False)
    assert (off["records"], off["alert"], off["alert_record"]) == (2, 10, 2)
    on = gen.model(wire, 0, True)
    assert fields(on) == (2, 2, len(wire) - len(bad), 0, 2, ku.KU_UPDATE_REQUESTED)


def test_truncation_by_slots(gen):
    """max_records in front of, at and behind the candidate."""
    recs = [gen.rec(0, b"x" * 9), gen.rec(1, ku.key_update_message(0), 22), gen.next().rec(0, b"y" * 9)]
    wire = b"".join(recs)
    assert fields(gen.model(wire, 0, True, slots=1)) == (1, 1, len(recs[0]), 0, 1, ku.KU_NONE)
    at = (2, 2, len(recs[0]) + len(recs[1]), 0, 2, ku.KU_UPDATE)
    assert fields(gen.model(wire, 0, True, slots=2)) == at
    assert fields(gen.model(wire, 0, True, slots=3)) == at


def test_confirm_needs_every_condition():
    msg = ku.key_update_message(1)
    assert ku.confirm(ku.KU_HELD, 3, 3, 22, 5, msg) == ku.KU_UPDATE_REQUESTED
    assert ku.confirm(ku.KU_NONE, 3, 3, 22, 5, msg) == ku.KU_NONE
    assert ku.confirm(ku.KU_HELD, 2, 3, 22, 5, msg) == ku.KU_HELD          # something failed
    assert ku.confirm(ku.KU_HELD, 3, 3, 23, 5, msg) == ku.KU_HELD          # application data
    assert ku.confirm(ku.KU_HELD, 3, 3, 22, 6, msg + b"\0") == ku.KU_HELD  # longer content
    assert ku.confirm(ku.KU_HELD, 3, 3, 22, 5, bytes([0x18, 0, 0, 1, 2])) == ku.KU_HELD


def test_wire_result_layout_is_unchanged():
    assert ta.WIRE_RESULT_DTYPE.itemsize == ta.WIRE_RESULT_KU_DTYPE.itemsize == 32
    f = ta.WIRE_RESULT_KU_DTYPE.fields
    assert [f[n][1] for n in ("first", "records", "delivered", "consumed", "alert", "alert_record",
                              "key_update", "reserved")] == list(range(0, 32, 4))
    assert ta.WIRE_RESULT_DTYPE.fields["reserved"][1] == 24
    r = np.zeros(1, dtype=ta.WIRE_RESULT_DTYPE)
    r["reserved"][0] = (3, 0)
    assert int(r.view(ta.WIRE_RESULT_KU_DTYPE)["key_update"][0]) == ta.WIRE_KU_HELD
    assert (ta.WIRE_KU_NONE, ta.WIRE_KU_UPDATE, ta.WIRE_KU_UPDATE_REQUESTED, ta.WIRE_KU_HELD) == \
        (ku.KU_NONE, ku.KU_UPDATE, ku.KU_UPDATE_REQUESTED, ku.KU_HELD) == (0, 1, 2, 3)
    src = open(ta.INCLUDE + "/tlsgpu.h").read()
    for name, value in (("NONE", 0), ("UPDATE", 1), ("UPDATE_REQUESTED", 2), ("HELD", 3)):
        assert f"#define TLSGPU_WIRE_KU_{name} {value}" in src
    assert "#define TLSGPU_ABI_VERSION 2" in src
    assert "uint32_t key_update;" in src


def test_switch_null_table_is_einval_without_a_device():
    lib = ta.load_library()
    assert lib.tlsgpu_sessions_wire_key_update(None, 1) == -1
    assert b"bad arguments" in lib.tlsgpu_last_error()
