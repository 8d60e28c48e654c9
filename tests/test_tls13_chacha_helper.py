"""CPU checks for TLS 1.3 ChaCha20-Poly1305 (TLS_CHACHA20_POLY1305_SHA256):
the expected-value helper (tests/tls13_helper.py) over the oracle's RFC 7905
AEAD against records captured from an OpenSSL connection, and the engine's
wire-size arithmetic for TLSGPU_CHACHA20_POLY1305_TLS13.

tests/golden/tls13_wire_chacha.json is tests/golden/tls13_wire.json again with
that suite negotiated (tools/make_tls13_fixture.py --suite): same writes, same
format.  RFC 7905's nonce is RFC 8446's, so the helper needs nothing new: the
oracle's kind 3 under the helper's nonce, additional data and inner plaintext
must open every captured record and re-seal it to the identical wire bytes.
The GPU tests (test_gpu_tls13_chacha.py) then take their expected values from
exactly this pairing.
"""
import os

import pytest

import pyoracle as po
import tls13_helper as t13

GOLDEN = os.path.join(os.path.dirname(t13.GOLDEN), "tls13_wire_chacha.json")
SUITE = "TLS_CHACHA20_POLY1305_SHA256"


@pytest.fixture(scope="module")
def fixture():
    return t13.load_fixture(GOLDEN)


def test_fixture_shape(fixture):
    assert fixture["suite"] == SUITE
    assert [d["name"] for d in fixture["directions"]] == ["client", "server"]
    for d in fixture["directions"]:
        assert len(d["key"]) == 32 and len(d["iv"]) == 12
        assert [r["seq"] for r in d["records"]] == list(range(len(d["records"])))
        app = b"".join(r["content"] for r in d["records"] if r["inner_type"] == 23)
        assert len(app) == sum(d["writes"])
    assert any(w > 16384 for d in fixture["directions"] for w in d["writes"])
    assert {r["inner_type"] for d in fixture["directions"] for r in d["records"]} >= {22, 23}


def test_helper_opens_and_reseals_every_captured_record(oracle, fixture):
    for d in fixture["directions"]:
        ctx = oracle.aead(po.CHACHA20_POLY1305, d["key"])
        for r in d["records"]:
            (hdr, frag), = t13.split_records(r["wire"])
            assert hdr == t13.header(len(frag))
            st, inner = t13.open_fragment(oracle, ctx, d["iv"], r["seq"], frag)
            assert st == len(r["content"]) and inner[:st] == r["content"], (d["name"], r["seq"])
            assert inner[st] == r["inner_type"]
            pad = len(inner) - st - 1
            again = t13.seal(oracle, ctx, d["iv"], r["seq"], r["inner_type"], r["content"], pad)
            assert hdr + again == r["wire"], (d["name"], r["seq"])
            # a wrong sequence number or a flipped bit does not open
            assert t13.open_fragment(oracle, ctx, d["iv"], r["seq"] + 1, frag)[0] == t13.BAD_MAC
            bad = bytearray(frag)
            bad[len(bad) // 2] ^= 4
            assert t13.open_fragment(oracle, ctx, d["iv"], r["seq"], bytes(bad))[0] == t13.BAD_MAC


def test_helper_seal_wire_reproduces_every_write(oracle, fixture):
    """The helper's framing of each write, the one above 16 KiB included, equals
    the captured records of that write."""
    for d in fixture["directions"]:
        ctx = oracle.aead(po.CHACHA20_POLY1305, d["key"])
        app = [r for r in d["records"] if r["inner_type"] == 23]
        k = 0
        for w in d["writes"]:
            n = len(t13.frame(bytes(w)))
            recs = app[k:k + n]
            k += n
            data = b"".join(r["content"] for r in recs)
            assert len(data) == w
            wire = t13.seal_wire(oracle, ctx, d["iv"], recs[0]["seq"], 23, data)
            assert wire == b"".join(r["wire"] for r in recs)
            assert len(wire) == t13.seal_wire_size(w)


def test_seal_wire_size_kind5():
    """Kind 5 exists in TLS 1.3 only: tlsgpu_seal_wire_size and _size_v give the
    TLS 1.3 framing whatever version is passed (host arithmetic, no GPU), over
    the grid of test_tls13_helper.py::test_seal_wire_size_v."""
    import talos_amd as ta
    ta.load_library()
    kind = ta.CHACHA20_POLY1305_TLS13
    assert kind == 5 and ta.KEY_LEN[kind] == 32 and ta.FIXED_IV_LEN[kind] == 12
    assert ta.EXPLICIT_NONCE_LEN[kind] == 0
    for n in (0, 1, 16383, 16384, 16385, 32768, 32769, 100000):
        for mf in (0, 1, 100, 16384, 20000):
            if mf == 1 and n > 20000:
                continue
            want = t13.seal_wire_size(n, mf)
            assert ta.seal_wire_size(kind, n, mf) == want, (n, mf)
            for version in (t13.VERSION, 0x0303, 0):
                assert ta.seal_wire_size(kind, n, mf, version=version) == want, (n, mf, version)
            assert ta.seal_wire_size(kind, n, mf, tag_len=12) == want   # the tag is 16 bytes
    assert ta.seal_wire_size(kind, 1) == 5 + 1 + 1 + 16
    assert ta.seal_wire_size(kind, 5, 1) == 5 * (5 + 1 + 1 + 16)
