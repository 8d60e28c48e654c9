"""CPU checks of the TLS 1.3 expected-value helper (tests/tls13_helper.py)
and of tlsgpu_seal_wire_size_v.

tests/golden/tls13_wire.json holds records an OpenSSL TLS 1.3 connection put
on the wire (tools/make_tls13_fixture.py), with each direction's traffic key
and IV.  The helper must open every one of them to the captured content and
inner type and re-seal that content to the identical wire bytes: nonce,
additional data, inner plaintext and framing then agree with an implementation
that shares nothing with this repository.  OpenSSL negotiates
TLS_AES_256_GCM_SHA384 here, so AES-128 rests on the helper being the same
code for both key sizes.
"""
import pytest

import pyoracle as po
import tls13_helper as t13


@pytest.fixture(scope="module")
def fixture():
    return t13.load_fixture()


def test_fixture_shape(fixture):
    assert fixture["suite"] in t13.SUITES
    names = [d["name"] for d in fixture["directions"]]
    assert names == ["client", "server"]
    for d in fixture["directions"]:
        assert [r["seq"] for r in d["records"]] == list(range(len(d["records"])))
        app = b"".join(r["content"] for r in d["records"] if r["inner_type"] == 23)
        assert len(app) == sum(d["writes"])
    # one write above 16 KiB went out as several records
    assert any(w > 16384 for d in fixture["directions"] for w in d["writes"])
    assert {r["inner_type"] for d in fixture["directions"] for r in d["records"]} >= {22, 23}


def test_helper_opens_and_reseals_every_captured_record(oracle, fixture):
    kind = t13.SUITES[fixture["suite"]][0]
    for d in fixture["directions"]:
        ctx = oracle.aead(kind, d["key"])
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


def test_helper_seal_wire_reproduces_the_multi_record_write(oracle, fixture):
    """The helper's framing of one write of more than 16 KiB equals the
    captured records of that write (OpenSSL fragments at 16384 too)."""
    kind = t13.SUITES[fixture["suite"]][0]
    d = fixture["directions"][1]
    app = [r for r in d["records"] if r["inner_type"] == 23]
    k = 0
    for w in d["writes"]:
        n = len(t13.frame(bytes(w)))
        recs = app[k:k + n]
        k += n
        if w <= 16384:
            continue
        data = b"".join(r["content"] for r in recs)
        assert len(data) == w
        ctx = oracle.aead(kind, d["key"])
        wire = t13.seal_wire(oracle, ctx, d["iv"], recs[0]["seq"], 23, data)
        assert wire == b"".join(r["wire"] for r in recs)
        assert len(wire) == t13.seal_wire_size(w)


def test_helper_statuses(oracle):
    key, iv = bytes(range(32)), bytes(range(100, 112))
    ctx = oracle.aead(po.AES_256_GCM, key)
    for inner, want in ((b"", t13.NO_CONTENT_TYPE), (bytes(40), t13.NO_CONTENT_TYPE),
                        (b"\x17", 0), (b"ab\0\0\x15\0\0\0", 4)):
        frag = t13.seal_inner(oracle, ctx, iv, 7, inner)
        st, out = t13.open_fragment(oracle, ctx, iv, 7, frag)
        assert st == want and out == inner
    assert t13.open_fragment(oracle, ctx, iv, 7, bytes(15)) == (t13.PUBLIC_INVALID, b"")


def test_seal_wire_size_v():
    """tlsgpu_seal_wire_size_v is host arithmetic (no GPU): the helper's framing
    for TLS 1.3 AES-GCM, tlsgpu_seal_wire_size for everything else."""
    import talos_amd as ta
    ta.load_library()
    for n in (0, 1, 16383, 16384, 16385, 32768, 32769, 100000):
        for mf in (0, 1, 100, 16384, 20000):
            if mf == 1 and n > 20000:
                continue
            want = sum(5 + len(p) + 1 + 16 for p in t13.frame(bytes(n), mf))
            assert want == t13.seal_wire_size(n, mf)
            for kind in (ta.AES_128_GCM, ta.AES_256_GCM):
                assert ta.seal_wire_size(kind, n, mf, version=t13.VERSION) == want, (n, mf)
                assert ta.seal_wire_size(kind, n, mf, version=0x0303) == \
                    ta.seal_wire_size(kind, n, mf)
            # 0x0304 with a ChaCha kind is no TLS 1.3 session of this engine
            assert ta.seal_wire_size(ta.CHACHA20_POLY1305, n, mf, version=t13.VERSION) == \
                ta.seal_wire_size(ta.CHACHA20_POLY1305, n, mf)
    assert ta.seal_wire_size(ta.AES_128_GCM, 1, 0, version=t13.VERSION) == 5 + 1 + 1 + 16
    assert ta.seal_wire_size(ta.AES_128_GCM, 5, 1, version=t13.VERSION) == 5 * (5 + 1 + 1 + 16)
    assert ta.REC_NO_CONTENT_TYPE == -6
