"""tlsgpu_open_wire's KeyUpdate cut (include/tlsgpu.h, "KeyUpdate on the wire read
path") restated over the oracle, for the tests' expected values.

The rule has three parts, each written here once:

* the candidate predicate: the first min(16, inner length) plaintext bytes of a
  record, got from one keystream block (the first 16 bytes of sealing 16 zero
  bytes under the record's nonce: all three TLS 1.3 suites are counter-mode),
  are 18 00 00 01 rr 16 00*, rr <= 1, and the inner plaintext has >= 6 bytes;
* the cut: the stream ends after its first candidate (records, consumed), a
  header-level alert behind it is dropped;
* the confirmation, after the normal open: key_update says "KeyUpdate" only for
  a delivered handshake record whose content is exactly 18 00 00 01 rr.

stream_model() is tlsgpu_open_wire for one TLS 1.3 stream with the switch on or
off: framing (RFC 8446 5.1-5.2 as include/tlsgpu.h states it), the cut, the
opens (tls13_helper.open_fragment), the alert order and the confirmation.
"""
import pyoracle as po
import tls13_helper as t13

KU_NONE, KU_UPDATE, KU_UPDATE_REQUESTED, KU_HELD = 0, 1, 2, 3
HANDSHAKE = 22
TAG = 16


def key_update_message(request_update: int) -> bytes:
    """KeyUpdate (RFC 8446 4.6.3): handshake type 24, length 1, request_update."""
    return bytes([0x18, 0, 0, 1, request_update])


def next_generation(secret: bytes, hashname: str) -> bytes:
    """application_traffic_secret_N+1 (RFC 8446 7.2)."""
    return t13.hkdf_expand_label(secret, "traffic upd", len(secret), hashname)


def keys_of(secret: bytes, key_len: int, hashname: str):
    """(write key, write IV) of a traffic secret (RFC 8446 7.3)."""
    return (t13.hkdf_expand_label(secret, "key", key_len, hashname),
            t13.hkdf_expand_label(secret, "iv", 12, hashname))


# suite -> (oracle AEAD kind, key length, hash of the key schedule)
SUITES = {"aes128": (po.AES_128_GCM, 16, "sha256"), "aes256": (po.AES_256_GCM, 32, "sha384"),
          "chacha": (po.CHACHA20_POLY1305, 32, "sha256")}


class Generation:
    """One traffic-key generation of one suite's read direction: seals records
    under its keys (the peer's side) and models the stream (ours)."""

    def __init__(self, impl, suite: str, secret: bytes):
        self.impl, self.suite, self.secret = impl, suite, secret
        self.kind, key_len, self.hashname = SUITES[suite]
        self.key, self.iv = keys_of(secret, key_len, self.hashname)
        self.ctx = impl.aead(self.kind, self.key)

    def next(self):
        return Generation(self.impl, self.suite, next_generation(self.secret, self.hashname))

    def rec(self, seq, content, itype=23, pad=0, inner=None) -> bytes:
        """header || fragment; inner: the TLSInnerPlaintext as given (any bytes)."""
        inner = t13.inner_plaintext(content, itype, pad) if inner is None else inner
        f = t13.seal_inner(self.impl, self.ctx, self.iv, seq, inner)
        return t13.header(len(f)) + f

    def key_update(self, seq, request_update=0, pad=0) -> bytes:
        return self.rec(seq, key_update_message(request_update), HANDSHAKE, pad)

    def model(self, wire, seq, switch, slots=None):
        return stream_model(self.impl, self.ctx, self.iv, wire, seq, switch, slots)


def keystream16(impl, ctx, iv: bytes, seq: int) -> bytes:
    """The record's first keystream block: AES-GCM E_K(nonce || 00000002),
    ChaCha20 the block with counter 1."""
    return t13.seal_inner(impl, ctx, iv, seq, bytes(16))[:16]


def looks_like_key_update(head: bytes) -> bool:
    """The predicate on the first min(16, inner length) plaintext bytes."""
    return (6 <= len(head) <= 16 and head[:4] == b"\x18\x00\x00\x01" and head[4] <= 1
            and head[5] == HANDSHAKE and not any(head[6:]))


def is_candidate(impl, ctx, iv: bytes, seq: int, fragment: bytes) -> bool:
    n = len(fragment) - TAG
    if n < 6:
        return False
    ks = keystream16(impl, ctx, iv, seq)
    return looks_like_key_update(bytes(a ^ b for a, b in zip(fragment[:min(16, n)], ks)))


def frame(wire: bytes, slots=None):
    """Header walk of a TLS 1.3 stream (version 0x0303): ([(pos, fragment length)],
    consumed, alert, records framed before any truncation).  slots: descriptor
    slots left for the stream; a stream that does not fit is cut at a record
    boundary and no alert is reached."""
    framed, pos, alert = [], 0, 0
    while pos + 5 <= len(wire):
        rtype, ver = wire[pos], (wire[pos + 1] << 8) | wire[pos + 2]
        ln = (wire[pos + 3] << 8) | wire[pos + 4]
        if ver != 0x0303:
            alert = 70
            break
        if rtype != 23:
            alert = 10
            break
        if pos + 5 + ln > len(wire):
            break
        if ln > t13.MAX_FRAGMENT:
            alert = 22
            break
        framed.append((pos, ln))
        pos += 5 + ln
    walked = len(framed)
    if slots is not None and slots < walked:
        framed = framed[:slots]
        pos = framed[-1][0] + 5 + framed[-1][1] if framed else 0
        alert = 0
    return framed, pos, alert, walked


def cut_fields(framed, consumed, alert, cand):
    """What the peek makes of the framing's result: (framed, consumed, alert,
    key_update) with the stream cut after record `cand` (None: no candidate)."""
    if cand is None:
        return framed, consumed, alert, KU_NONE
    pos, ln = framed[cand]
    return framed[:cand + 1], pos + 5 + ln, 0, KU_HELD


def confirm(key_update, delivered, records, inner_type, status, plaintext: bytes):
    """key_update after the open: inner_type / status / plaintext are those of the
    stream's last framed record."""
    if key_update != KU_HELD or delivered != records:
        return key_update
    if inner_type != HANDSHAKE or status != 5:
        return key_update
    if plaintext[:4] != b"\x18\x00\x00\x01" or plaintext[4] > 1:
        return key_update
    return KU_UPDATE + plaintext[4]


def stream_model(impl, ctx, iv: bytes, wire: bytes, seq: int, switch: bool, slots=None):
    """tlsgpu_open_wire for one TLS 1.3 stream -> dict(records, delivered,
    consumed, alert, alert_record, key_update, walked, recs = [(status, region,
    inner type)] per framed record; region None for a skipped record)."""
    framed, consumed, alert, walked = frame(wire, slots)
    cand = None
    if switch:
        for i, (p, ln) in enumerate(framed):
            if is_candidate(impl, ctx, iv, seq + i, bytes(wire[p + 5:p + 5 + ln])):
                cand = i
                break
    framed, consumed, alert, ku = cut_fields(framed, consumed, alert, cand)
    recs, dead, alert_rec, delivered = [], False, len(framed), len(framed)
    for i, (p, ln) in enumerate(framed):
        if dead:
            recs.append((t13.SKIPPED, None, 23))
            continue
        st, region = t13.open_fragment(impl, ctx, iv, seq + i, bytes(wire[p + 5:p + 5 + ln]))
        a = {t13.BAD_MAC: 20, t13.PUBLIC_INVALID: 21, t13.NO_CONTENT_TYPE: 10}.get(st, 0)
        if st >= 0 and st > t13.MAX_PLAIN:
            st, a = t13.OVERFLOW, 22
        recs.append((st, region, region[st] if st >= 0 else 23))
        if a:
            dead, alert, alert_rec, delivered = True, a, i, i
    if framed:
        st, region, itype = recs[-1]
        ku = confirm(ku, delivered, len(framed), itype, st, region[:5] if region else b"")
    return dict(records=len(framed), delivered=delivered, consumed=consumed, alert=alert,
                alert_record=alert_rec, key_update=ku, walked=walked, recs=recs, framed=framed)
