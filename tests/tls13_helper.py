"""TLS 1.3 record protection (RFC 8446 5.2-5.4) over any AEAD object, for the
tests' expected values.

The reference has no TLS 1.3, so nothing here comes from it: the AEAD itself
is ``pyoracle.Oracle()`` (or ``pyoracle.Reference()`` where oracle/_ref is
built), and this module adds the RFC's nonce, additional data, inner plaintext
and framing in Python.  tests/golden/tls13_wire.json (records captured from an
OpenSSL TLS 1.3 connection by tools/make_tls13_fixture.py) checks it against an
independent implementation: test_tls13_helper.py opens every captured record
with it and re-seals it to the identical wire bytes.

Statuses follow include/tlsgpu.h: an open returns the content length and the
inner plaintext as decrypted, NO_CONTENT_TYPE (-6) for an empty or all-zero
inner plaintext, BAD_MAC (-1) with zeros, PUBLIC_INVALID (-2) below a tag.
"""
import base64
import hashlib
import hmac
import json
import os

import pyoracle as po

TAG = 16
APPLICATION_DATA = 23
MAX_PLAIN = 16384
MAX_FRAGMENT = 16384 + 256          # ciphertext bound, RFC 8446 5.2
BAD_MAC, PUBLIC_INVALID, SKIPPED, OVERFLOW, OUT_OF_BOUNDS, NO_CONTENT_TYPE = -1, -2, -3, -4, -5, -6
VERSION = 0x0304
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tls13_wire.json")
SUITES = {"TLS_AES_128_GCM_SHA256": (po.AES_128_GCM, "sha256"),
          "TLS_AES_256_GCM_SHA384": (po.AES_256_GCM, "sha384")}


def nonce(iv: bytes, seq: int) -> bytes:
    """write_iv XOR (0^32 || BE64(seq)), RFC 8446 5.3."""
    assert len(iv) == 12
    return bytes(a ^ b for a, b in zip(iv, bytes(4) + seq.to_bytes(8, "big")))


def header(fragment_len: int) -> bytes:
    """The record header, which is also the additional data (RFC 8446 5.2)."""
    return bytes([APPLICATION_DATA, 3, 3, fragment_len >> 8, fragment_len & 0xFF])


def inner_plaintext(content: bytes, inner_type: int, pad: int = 0) -> bytes:
    return content + bytes([inner_type]) + bytes(pad)


def seal_inner(impl, ctx, iv: bytes, seq: int, inner: bytes) -> bytes:
    """ciphertext || tag of a given TLSInnerPlaintext (any bytes, so tests can
    make all-zero and empty ones)."""
    ok, out = impl.seal(ctx, nonce(iv, seq), inner, header(len(inner) + TAG))
    if not ok:
        raise RuntimeError("seal failed")
    return out


def seal(impl, ctx, iv: bytes, seq: int, inner_type: int, content: bytes, pad: int = 0) -> bytes:
    """The fragment tlsgpu_seal_batch writes for a TLS 1.3 session (pad = 0)."""
    return seal_inner(impl, ctx, iv, seq, inner_plaintext(content, inner_type, pad))


def content_length(inner: bytes):
    """Index of the last non-zero byte (the inner type), None if there is none."""
    n = len(inner.rstrip(b"\0"))
    return n - 1 if n else None


def open_fragment(impl, ctx, iv: bytes, seq: int, fragment: bytes):
    """(status, output region) as tlsgpu_open_batch gives them: the region is
    the whole inner plaintext as decrypted, or zeros for BAD_MAC."""
    if len(fragment) < TAG:
        return PUBLIC_INVALID, b""
    n = len(fragment) - TAG
    ok, out = impl.open(ctx, nonce(iv, seq), fragment, header(len(fragment)), max_out=n)
    if not ok:
        return BAD_MAC, bytes(n)
    cl = content_length(out)
    return (NO_CONTENT_TYPE if cl is None else cl), out


def frame(data: bytes, max_fragment: int = 0):
    """The fragments tlsgpu_seal_wire makes of one write."""
    frag = MAX_PLAIN if max_fragment == 0 or max_fragment > MAX_PLAIN else max_fragment
    return [data[i:i + frag] for i in range(0, len(data), frag)]


def seal_wire(impl, ctx, iv: bytes, seq: int, inner_type: int, data: bytes,
              max_fragment: int = 0) -> bytes:
    """The wire bytes of one tlsgpu_seal_wire stream of a TLS 1.3 session."""
    out = b""
    for k, piece in enumerate(frame(data, max_fragment)):
        f = seal(impl, ctx, iv, seq + k, inner_type, piece)
        out += header(len(f)) + f
    return out


def seal_wire_size(data_len: int, max_fragment: int = 0) -> int:
    frag = MAX_PLAIN if max_fragment == 0 or max_fragment > MAX_PLAIN else max_fragment
    return data_len + ((data_len + frag - 1) // frag) * (5 + 1 + TAG)


def split_records(wire: bytes):
    """[(header, fragment)] of complete records."""
    out, p = [], 0
    while p + 5 <= len(wire):
        n = (wire[p + 3] << 8) | wire[p + 4]
        if p + 5 + n > len(wire):
            break
        out.append((wire[p:p + 5], wire[p + 5:p + 5 + n]))
        p += 5 + n
    return out


# -- key schedule (RFC 8446 7.1, 7.3): traffic secret -> write key and IV ------

def hkdf_expand(prk: bytes, info: bytes, length: int, hashname: str) -> bytes:
    out, t, i = b"", b"", 1
    while len(out) < length:
        t = hmac.new(prk, t + info + bytes([i]), getattr(hashlib, hashname)).digest()
        out += t
        i += 1
    return out[:length]


def hkdf_expand_label(secret: bytes, label: str, length: int, hashname: str) -> bytes:
    full = b"tls13 " + label.encode()
    info = length.to_bytes(2, "big") + bytes([len(full)]) + full + b"\0"   # empty context
    return hkdf_expand(secret, info, length, hashname)


def traffic_keys(secret: bytes, suite: str):
    """(AEAD kind, write key, write IV) of a traffic secret."""
    kind, hashname = SUITES[suite]
    return (kind, hkdf_expand_label(secret, "key", po.KEY_LEN[kind], hashname),
            hkdf_expand_label(secret, "iv", 12, hashname))


def load_fixture(path: str = GOLDEN):
    """The captured connection: {"suite", "directions": [{"name", "key", "iv",
    "records": [{"seq", "wire", "inner_type", "content"}], "writes": [...]}]},
    keys in hex, record bytes in base64, decoded."""
    fx = json.load(open(path))
    for d in fx["directions"]:
        d["key"] = bytes.fromhex(d["key"])
        d["iv"] = bytes.fromhex(d["iv"])
        for r in d["records"]:
            r["wire"] = base64.b64decode(r["wire"])
            r["content"] = base64.b64decode(r["content"])
    return fx
