"""gcm_stream.hip, the GCM128 state machine behind EVP_aes_{128,256}_gcm, driven
directly: talos_amd.EvpCipher calls the cipher object's own ctrl / init /
do_cipher / cleanup the way a generic EVP layer does (include/tlsgpu_evp.h), and
every return value and every output byte is compared with pyoracle.GcmStream,
the CPU restatement of gcm128.c fed the same pieces (tests/
test_gcm_counter_model.py pins that model).  No reference binary is involved.

What the pieces are chosen for (gcm_stream_kernel): whole blocks run on 64
lanes, lane l hashing blocks l, l + 64, ... as a chain in H^64 that is closed
with H^(nblk - jlast), so pieces of 63 / 64 / 65, 127 / 128 / 129, 192 / 193 and
1,000 blocks put the chain lengths and the closing exponents on both sides of
every lane boundary; a 5-byte piece before them makes lane 0's byte loop finish
the open block first (11 bytes) and leaves a tail whose keystream block waits in
EKi for the next call.  The crafted IVs (tests/gcm_iv_craft.py) put the 32-bit
counter wrap in the first block, in a lane other than 0, on a call boundary, on
a carried tail block, and behind a ctrl(COPY) taken inside a block.

Each output buffer lies between 64 bytes of 0xA5 on either side, which must come
back unchanged, also from a failing call.
"""
import ctypes as C
import random

import pytest

import gcm_iv_craft as gic
import pyoracle as po

pytestmark = pytest.mark.gpu

GUARD = 64
KEYS = [pytest.param(16, id="aes128"), pytest.param(32, id="aes256")]
MODES = ["enc", "dec", "dec-inplace"]
BLOCK_PIECES = (1, 63, 64, 65, 127, 128, 129, 192, 193, 1000)


@pytest.fixture(scope="module")
def ta():
    import talos_amd
    talos_amd.load_library()
    return talos_amd


class Guarded:
    """n bytes between two runs of 0xA5."""

    def __init__(self, n: int, fill: bytes = b""):
        self.n = n
        self.buf = (C.c_ubyte * (n + 2 * GUARD)).from_buffer_copy(
            b"\xA5" * GUARD + fill + b"\xA5" * (n - len(fill)) + b"\xA5" * GUARD)
        self.addr = C.addressof(self.buf) + GUARD

    def data(self) -> bytes:
        return bytes(self.buf)[GUARD:GUARD + self.n]

    def guards_intact(self) -> bool:
        b = bytes(self.buf)
        return b[:GUARD] == b"\xA5" * GUARD and b[GUARD + self.n:] == b"\xA5" * GUARD


class Pair:
    """An EvpCipher context and the model stream, stepped together."""

    def __init__(self, ta, oracle, key, iv, enc, inplace=False, *, _parts=None):
        self.ta, self.enc, self.inplace = ta, enc, inplace
        if _parts:
            self.c, self.m = _parts
            return
        kind = ta.AES_128_GCM if len(key) == 16 else ta.AES_256_GCM
        self.c = ta.EvpCipher(kind, enc)
        assert self.c.ok == 1
        if len(iv) != 12:
            assert self.c.ctrl(ta.EvpCipher.GCM_SET_IVLEN, len(iv)) == 1
        assert self.c.init(key, iv) == 1
        self.m = po.GcmStream(oracle, key)
        self.m.setiv(iv)

    def aad(self, data: bytes) -> int:
        rc, want = self.c.update_aad(data), self.m.aad(data)
        assert rc == (len(data) if want == 0 else -1), (rc, want, len(data))
        return rc

    def data(self, data: bytes) -> bytes:
        out = Guarded(len(data), data if self.inplace else b"")
        src = out if self.inplace else (C.c_ubyte * max(len(data), 1)).from_buffer_copy(data or b"\0")
        rc = self.c.do_cipher(out.addr, out.addr if self.inplace else C.addressof(src), len(data))
        want_rc, want = (self.m.encrypt if self.enc else self.m.decrypt)(data)
        assert want_rc == 0 and rc == len(data), (rc, want_rc, len(data))
        assert out.guards_intact(), f"a {len(data)}-byte piece wrote outside its output"
        got = out.data()
        if got != want:
            bad = next(i for i in range(len(want)) if got[i] != want[i])
            raise AssertionError(f"piece of {len(data)} bytes differs first at byte {bad} "
                                 f"(block {bad // 16} of the piece)")
        return got

    def final_encrypt(self) -> bytes:
        assert self.enc and self.c.final() == 0
        tag = self.m.tag(16)
        assert self.c.get_tag(16) == (1, tag) and self.c.get_tag(12) == (1, tag[:12])
        return tag

    def final_decrypt(self, tag: bytes) -> int:
        assert not self.enc and self.c.ctrl(self.ta.EvpCipher.GCM_SET_TAG, len(tag), tag) == 1
        rc, want = self.c.final(), self.m.finish(tag)
        assert rc == want, (rc, want, len(tag))
        return rc

    def finish(self, good_tag: bytes) -> None:
        if self.enc:
            assert self.final_encrypt() == good_tag
        else:
            assert self.final_decrypt(good_tag) == 0

    def copy(self) -> "Pair":
        c = self.c.copy()
        assert c.ok == 1
        return Pair(self.ta, None, None, None, self.enc, self.inplace, _parts=(c, self.m.copy()))

    def close(self) -> None:
        assert self.c.cleanup() == 1


def _stream(ta, oracle, key, iv, aad, pt, pieces, mode):
    """One whole stream in `pieces` (their sum is len(pt)), checked call by call."""
    ct, tag = oracle.gcm(key, iv, aad, pt)
    before = ta.evp_cipher_stats()
    p = Pair(ta, oracle, key, iv, mode == "enc", mode == "dec-inplace")
    if aad:
        p.aad(aad)
    src, got, off = (pt if mode == "enc" else ct), b"", 0
    for k in pieces:
        got += p.data(src[off:off + k])
        off += k
    assert off == len(pt) and got == (ct if mode == "enc" else pt)
    p.finish(tag)
    p.close()
    # every call was a program on the stream kernel: setiv, AAD, the pieces, the tag
    assert ta.evp_cipher_stats() - before == 2 + bool(aad) + len(pieces)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("key_len", KEYS)
@pytest.mark.parametrize("prefixed", [False, True], ids=["aligned", "after5bytes"])
def test_whole_block_pieces(ta, oracle, key_len, mode, prefixed):
    """Pieces of whole blocks at the lane boundaries with mres == 0; then each
    between a 5-byte and an 11-byte piece, so that lane 0 first finishes the
    open block (11 bytes), the piece ends 5 bytes into a block kept in EKi,
    and the 11-byte call that follows is a prefix alone (nblk == 0)."""
    rnd = random.Random(key_len + prefixed)
    key, iv, aad = rnd.randbytes(key_len), rnd.randbytes(12), rnd.randbytes(13)
    pieces = []
    for k in BLOCK_PIECES:
        pieces += [5, 16 * k, 11] if prefixed else [16 * k]
    assert sum(pieces) <= 40 * 1024
    _stream(ta, oracle, key, iv, aad, rnd.randbytes(sum(pieces)), pieces, mode)


@pytest.mark.parametrize("key_len", KEYS)
def test_aad_pieces_and_aad_after_data(ta, oracle, key_len):
    """AAD in pieces of 0, 1, 15, 16, 17 and 300 bytes in two orders (ares of 0,
    1 and 12 carried between calls); AAD after data is refused (gcm128.c: -2,
    do_cipher: -1) and the stream goes on as if it had not been sent."""
    rnd = random.Random(70 + key_len)
    for order in ((0, 1, 15, 16, 17, 300), (17, 300, 1, 0, 15, 16)):
        key, iv = rnd.randbytes(key_len), rnd.randbytes(12)
        for enc in (True, False):
            p = Pair(ta, oracle, key, iv, enc)
            for k in order:
                assert p.aad(rnd.randbytes(k)) == k
            p.data(rnd.randbytes(100))
            assert p.aad(rnd.randbytes(20)) == -1
            assert p.aad(b"") == -1
            p.data(rnd.randbytes(50))
            if enc:
                p.final_encrypt()
            else:
                assert p.final_decrypt(p.m.tag(16)) == 0
            p.close()
    p = Pair(ta, oracle, key, iv, True)   # AAD alone: the tag of an empty message
    assert p.aad(rnd.randbytes(33)) == 33
    p.final_encrypt()
    p.close()


@pytest.mark.parametrize("key_len", KEYS)
@pytest.mark.parametrize("tag_len", [4, 12, 16])
def test_decrypt_final_with_short_and_wrong_tags(ta, oracle, key_len, tag_len):
    rnd = random.Random(90 + key_len + tag_len)
    key, iv, aad, pt = rnd.randbytes(key_len), rnd.randbytes(12), rnd.randbytes(21), rnd.randbytes(77)
    ct, tag = oracle.gcm(key, iv, aad, pt)
    for flip in (None, 0, tag_len - 1):
        t = bytearray(tag[:tag_len])
        if flip is not None:
            t[flip] ^= 0x10
        p = Pair(ta, oracle, key, iv, False)
        p.aad(aad)
        assert p.data(ct) == pt
        assert p.final_decrypt(bytes(t)) == (0 if flip is None else -1)
        p.close()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("key_len", KEYS)
@pytest.mark.parametrize("iv_len", gic.STREAM_IV_LENS)
@pytest.mark.parametrize("where", list(gic.STREAM_WRAPS))
def test_counter_wrap_by_position(ta, oracle, where, iv_len, key_len, mode):
    """The block whose counter is 0 (inc32: bytes 0..11 of the counter block stay)
    in the first block, in lane 6 of a 200-block piece, first in a call, and as a
    tail block whose keystream is used by two calls."""
    w, pieces = gic.STREAM_WRAPS[where]
    rnd = random.Random(key_len + iv_len + w)
    key = rnd.randbytes(key_len)
    iv = gic.craft_iv(oracle, key, iv_len, (1 << 32) - 1 - w, w)
    assert 16 * w < sum(pieces)
    _stream(ta, oracle, key, iv, rnd.randbytes(5), rnd.randbytes(sum(pieces)), pieces, mode)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("key_len", KEYS)
@pytest.mark.parametrize("iv_len", gic.STREAM_IV_LENS)
def test_counter_wrap_behind_a_copy(ta, oracle, iv_len, key_len, mode):
    """ctrl(COPY) with mres == 7; the original and the copy go on with different
    data over the block whose counter is 0, each as its own model does."""
    w, enc = gic.STREAM_COPY_W, mode == "enc"
    rnd = random.Random(300 + key_len + iv_len)
    key = rnd.randbytes(key_len)
    iv = gic.craft_iv(oracle, key, iv_len, (1 << 32) - 1 - w, w)
    a = Pair(ta, oracle, key, iv, enc, mode == "dec-inplace")
    a.aad(rnd.randbytes(13))
    a.data(rnd.randbytes(16 * 30 + 7))
    b = a.copy()
    a.data(rnd.randbytes(9 + 16 * 10))
    b.data(rnd.randbytes(16 * 5 + 3))
    b.data(rnd.randbytes(13 + 16 * 64))
    a.data(rnd.randbytes(16 * 2))
    for p in (a, b):
        if enc:
            p.final_encrypt()
        else:
            assert p.final_decrypt(p.m.tag(16)) == 0
        p.close()


@pytest.mark.parametrize("key_len", KEYS)
def test_tls_record_mode(ta, oracle, key_len):
    """SET_IV_FIXED + AEAD_TLS1_AAD + in-place do_cipher (aes_gcm_tls_cipher,
    e_aes.c:917-985): explicit IV || ciphertext || tag against the oracle with
    the nonce fixed || explicit and the AAD's length set to the payload's; one
    tampered record opens to -1 with its payload zeroed."""
    E = ta.EvpCipher
    kind = ta.AES_128_GCM if key_len == 16 else ta.AES_256_GCM
    rnd = random.Random(500 + key_len)
    key, fixed = rnd.randbytes(key_len), rnd.randbytes(12)
    e, d = E(kind, True), E(kind, False)
    assert e.ok == 1 and d.ok == 1 and e.init(key) == 1 and d.init(key) == 1
    assert e.ctrl(E.GCM_SET_IV_FIXED, -1, fixed) == 1 and d.ctrl(E.GCM_SET_IV_FIXED, 4, fixed[:4]) == 1
    explicit = int.from_bytes(fixed[4:], "big")
    for i, n in enumerate((0, 1, 16, 1024, 16384, 16)):
        pt = rnd.randbytes(n)
        # the AAD's length field as the record layer sets it: explicit IV + payload
        # on a seal, the whole fragment on an open; the cipher reduces both to n
        ad11 = rnd.randbytes(8) + bytes([23, 3, 3])
        ad_seal, ad = ad11 + (n + 8).to_bytes(2, "big"), ad11 + (n + 24).to_bytes(2, "big")
        ex = ((explicit + i) % (1 << 64)).to_bytes(8, "big")   # ctr64_inc after every seal
        ct, tag = oracle.gcm(key, fixed[:4] + ex, ad11 + n.to_bytes(2, "big"), pt)
        rec = Guarded(n + 24, bytes(8) + pt)
        assert e.ctrl(E.AEAD_TLS1_AAD, 13, ad_seal) == 16
        assert e.do_cipher(rec.addr, rec.addr, n + 24) == n + 24
        assert rec.guards_intact() and rec.data() == ex + ct + tag, n
        tamper = i == 5
        wire = bytearray(rec.data())
        if tamper:
            wire[8 + n // 2] ^= 0x40
        rec = Guarded(n + 24, bytes(wire))
        assert d.ctrl(E.AEAD_TLS1_AAD, 13, ad) == 16
        r = d.do_cipher(rec.addr, rec.addr, n + 24)
        assert rec.guards_intact()
        if tamper:
            assert r == -1 and rec.data() == bytes(wire[:8]) + bytes(n) + bytes(wire[8 + n:])
        else:
            assert r == n and rec.data()[8:8 + n] == pt
    # a record shorter than explicit IV + tag, and an out-of-place call, are refused untouched
    assert e.ctrl(E.AEAD_TLS1_AAD, 13, ad) == 16
    rec, other = Guarded(23, bytes(23)), Guarded(40, bytes(40))
    assert e.do_cipher(rec.addr, rec.addr, 23) == -1
    assert e.do_cipher(other.addr, rec.addr, 40) == -1
    for g in (rec, other):
        assert g.guards_intact() and g.data() == bytes(g.n)
    assert e.cleanup() == 1 and d.cleanup() == 1
