"""The TLS 1.3 block padding rule of a session (include/tlsgpu.h, pad_block;
RFC 8446 5.4; OpenSSL's SSL_CTX_set_block_padding / RecordPadding) over
tests/tls13_helper.py, for the tests' expected values.

    inner = len + 1                    pad_block <= 1 or len >= 16384
    inner = roundup(len + 1, pad_block) otherwise

The fragment is ciphertext(content || type || zeros) || tag, the additional
data 17 03 03 BE16(inner + 16), the status inner + 16.  Nothing here comes from
the engine: tests/golden/tls13_wire_padded.json and
tls13_wire_chacha_padded.json (an OpenSSL connection under RecordPadding = 512,
tools/make_tls13_fixture.py --record-padding 512) check the rule and the
framing against an independent implementation in test_tls13_padding.py.
"""
import os

import tls13_helper as t13

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN_PADDED = os.path.join(HERE, "golden", "tls13_wire_padded.json")
GOLDEN_CHACHA_PADDED = os.path.join(HERE, "golden", "tls13_wire_chacha_padded.json")


def inner_len(n: int, block: int) -> int:
    """Length of the TLSInnerPlaintext a session with padding block `block`
    seals for `n` content bytes."""
    if block <= 1 or n >= t13.MAX_PLAIN:
        return n + 1
    return -(-(n + 1) // block) * block


def pad_len(n: int, block: int) -> int:
    return inner_len(n, block) - n - 1


def seal(impl, ctx, iv: bytes, seq: int, inner_type: int, content: bytes, block: int) -> bytes:
    """The fragment tlsgpu_seal_batch writes for a session with pad_block = block."""
    return t13.seal(impl, ctx, iv, seq, inner_type, content, pad_len(len(content), block))


def seal_wire(impl, ctx, iv: bytes, seq: int, inner_type: int, data: bytes, block: int,
              max_fragment: int = 0) -> bytes:
    """The wire bytes of one tlsgpu_seal_wire stream of such a session."""
    out = b""
    for k, piece in enumerate(t13.frame(data, max_fragment)):
        f = seal(impl, ctx, iv, seq + k, inner_type, piece, block)
        out += t13.header(len(f)) + f
    return out


def seal_wire_size(data_len: int, block: int, max_fragment: int = 0) -> int:
    frag = t13.MAX_PLAIN if max_fragment == 0 or max_fragment > t13.MAX_PLAIN else max_fragment
    return sum(5 + inner_len(min(frag, data_len - o), block) + t13.TAG
               for o in range(0, data_len, frag))
