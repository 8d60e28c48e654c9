"""TLSGPU_MAX_RECORD (65534 x 16 bytes) and the counter range below it, on the GPU.

The AES-GCM kernels' fast AES form rests on the limit: parse_tls accepts no
plaintext above it, so the counters 2..nb + 1 of a record stay below 2^16.  The
batches here hold plaintexts of 16 * 2^k + 53 bytes for k = 12..15 (the counter
crosses each of its bits 12..15, with a partial last block), TLSGPU_MAX_RECORD -
15 and TLSGPU_MAX_RECORD itself (counter 65535), a 17-byte and a 16384-byte
record between them, and one record of TLSGPU_MAX_RECORD + 1 bytes, which must
get TLSGPU_REC_PUBLIC_INVALID with not a byte written while its neighbours are
exact.  An open batch also holds a long record with a bit flipped in its last
ciphertext block: TLSGPU_REC_BAD_MAC and all n bytes zero.  Every route of
test_gpu_tag_len.py but the pack hint runs them, seal and open, through
batch_image.run_image (whole image, statuses, slack, twice).

A TLS 1.3 AES-GCM table: the limit bounds the inner plaintext, so a content of
TLSGPU_MAX_RECORD - 1 bytes seals and TLSGPU_MAX_RECORD does not.

The ChaCha20-Poly1305 kinds have no 16-bit counter and their kernels do not
enforce the limit (include/tlsgpu.h says so): one record of TLSGPU_MAX_RECORD +
16 bytes of each kind, TLS 1.2 RFC and draft suites and the TLS 1.3 kind, seals
and opens to the oracle's bytes.

The model is batch_image's (tls1_enc over the oracle's AEAD).  A record longer
than 65535 bytes is no TLS record: the 16-bit length in its additional data is
the low 16 bits of the length, in pyoracle.tls_ad and in the TLS 1.3 model below
(tests/tls13_helper.py's framing, whose header() takes real record lengths only)
as in the kernels.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import batch_image as bi
import pyoracle as po
import tls13_helper as t13

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX = 65534 * 16
KINDS = {"aes-128-gcm": po.AES_128_GCM, "aes-256-gcm": po.AES_256_GCM}
ROUTES = [("queue", 3), ("queue", 0), ("split", 0), ("ttable", 0), ("auto", 0),
          ("hybrid", 0), ("bitslice", 0), ("fused", 0)]
EXPERIMENTAL_IMPLS = ("hybrid", "bitslice", "fused")
BITS = [16 * 2 ** k + 53 for k in (12, 13, 14, 15)]
OVER = -1                                        # in a plan: the record above the limit
PLAN = [BITS[0], 17, BITS[1], OVER, 16384, BITS[2], MAX - 15, 17, BITS[3], MAX, 16384, 17]
TAMPERED = BITS[3]


@pytest.fixture(scope="module")
def ta():
    import talos_amd
    talos_amd.load_library()
    return talos_amd


@pytest.fixture(scope="module")
def engine(ta):
    e = ta.Engine(0)
    yield e
    e.close()


@pytest.fixture
def gcm_impl(ta):
    prev = ta.get_gcm_impl()

    def use(impl):
        try:
            ta.set_gcm_impl(impl)
        except ta.TlsGpuError:
            if impl in EXPERIMENTAL_IMPLS:
                pytest.skip(f"gcm impl {impl} not built (make EXPERIMENTAL=1)")
            raise
    yield use
    ta.set_gcm_impl(prev)


_cache = {}


def _flip_last_block(frag, tag):
    b = bytearray(frag)
    b[len(frag) - tag - 7] ^= 0x20
    return bytes(b)


def material12(ta, oracle, kind, lengths, over):
    """Two sessions of `kind`; -> (sessions, seal entries, open entries).  The
    record above the limit is `over` bytes long and publicly invalid (for ChaCha,
    over = 0: there is none); on open its fragment is the model's valid one."""
    key = (kind, tuple(lengths), over)
    if key not in _cache:
        sessions = bi.make_sessions(ta, oracle, [kind] * 2, [0, 16], 40 + kind)
        rng = np.random.default_rng(kind)
        seals, opens = [], []
        for i, n in enumerate(lengths):
            sid, seq, rtype = i % 2, (1 << 35) + i, 23 - i % 2
            s = sessions[sid]
            e = bi.seal_entry(ta, oracle, sessions, sid, seq, rtype, rng.bytes(over if n == OVER else n))
            o = bi.open_entry(ta, oracle, sessions, sid, seq, rtype, e.out)
            assert o.st == len(e.inp) and o.out == e.inp
            if n == OVER:
                e = bi.Entry(sid, seq, rtype, e.inp, ta.REC_PUBLIC_INVALID, b"", s.eiv,
                             reserve=len(e.out))
                o = bi.Entry(sid, seq, rtype, o.inp, ta.REC_PUBLIC_INVALID, b"", s.eiv,
                             reserve=len(o.out))
            seals.append(e)
            opens.append(o)
            if n == TAMPERED:
                o = bi.open_entry(ta, oracle, sessions, sid, seq, rtype, _flip_last_block(e.out, 16))
                assert o.st == ta.REC_BAD_MAC and o.out == bytes(n)
                opens.insert(len(opens) - 1, o)
        _cache[key] = (sessions, seals, opens)
    return _cache[key]


def run12(ta, engine, oracle, kind, lengths, over, mode, hints=None):
    sessions, seals, opens = material12(ta, oracle, kind, lengths, over)
    table = ta.SessionTable(engine, len(sessions))
    table.install(0, [s.params for s in sessions])
    if hints is not None:
        table.hint(hints)
    entries = seals if mode == "seal" else opens
    mix = [3 if i % 2 == 0 else 5 for i in range(len(entries))]
    bi.run_image(ta, engine, table, entries, mode == "seal", label=(kind, mode, hints, "aligned"))
    bi.run_image(ta, engine, table, entries, mode == "seal", in_shifts=mix, out_shifts=mix[::-1],
                 label=(kind, mode, hints, "shifted"))
    table.close()


@pytest.mark.parametrize("mode", ["seal", "open"])
@pytest.mark.parametrize("impl,hints", ROUTES, ids=["%s-%d" % r for r in ROUTES])
@pytest.mark.parametrize("name", list(KINDS))
def test_gcm_counter_range_and_limit(ta, engine, oracle, gcm_impl, name, impl, hints, mode):
    gcm_impl(impl)
    run12(ta, engine, oracle, KINDS[name], PLAN, MAX + 1, mode, hints)


@pytest.mark.parametrize("mode", ["seal", "open"])
@pytest.mark.parametrize("kind", [po.CHACHA20_POLY1305, po.CHACHA20_POLY1305_OLD],
                         ids=["chacha20-poly1305", "chacha20-poly1305-old"])
def test_chacha_has_no_limit(ta, engine, oracle, kind, mode):
    """What the kernels do today and the header says: a ChaCha record above
    TLSGPU_MAX_RECORD is processed, to the oracle's bytes."""
    run12(ta, engine, oracle, kind, [17, MAX + 16, 16384, 17], 0, mode)


def _child(env, body):
    code = ("import sys; sys.path[:0] = [%r, %r]\n"
            "import test_gpu_record_limit as t, pyoracle as po, talos_amd as ta\n"
            "ta.load_library(); e = ta.Engine(0); o = po.Oracle()\n"
            "for mode in ('seal', 'open'):\n"
            "    for kind in %s:\n"
            "        t.run12(ta, e, o, kind, %s, mode)\n"
            "e.close(); print('ok')\n") % (os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"),
                                           body[0], body[1])
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=110,
                       env=dict(os.environ, **env), cwd=ROOT)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stderr[-3000:]


def test_per_wave_session_kernel_forced():
    """TLSGPU_PWS=1 (gcm_pw.hip, which counts on its own), in a child process."""
    _child({"TLSGPU_PWS": "1", "TLSGPU_GCM_IMPL": "queue"},
           ("(po.AES_128_GCM, po.AES_256_GCM)", "t.PLAN, t.MAX + 1"))


def test_legacy_chacha_kernel_forced():
    """TLSGPU_CHACHA_LEGACY=1, in a child process."""
    _child({"TLSGPU_CHACHA_LEGACY": "1"},
           ("(po.CHACHA20_POLY1305, po.CHACHA20_POLY1305_OLD)", "[17, t.MAX + 16, 16384, 17], 0"))


# -- TLS 1.3 ---------------------------------------------------------------------

def seal13(oracle, ctx, iv, seq, itype, content):
    """tls13_helper.seal with the header's length taken mod 2^16."""
    inner = t13.inner_plaintext(content, itype)
    n = len(inner) + t13.TAG
    ok, out = oracle.seal(ctx, t13.nonce(iv, seq), inner, bytes([23, 3, 3, (n >> 8) & 0xFF, n & 0xFF]))
    assert ok and len(out) == n
    if n < 65536:
        assert out == t13.seal(oracle, ctx, iv, seq, itype, content)
    return out


def run13(ta, engine, oracle, kind, okind, lengths, limit, impl_label):
    """One TLS 1.3 session of `kind` (the oracle's AEAD `okind`); contents of
    `lengths` bytes, those above `limit` publicly invalid; seal, then open."""
    rng = np.random.default_rng(13 * kind)
    p = ta.SessionParams(kind, rng.bytes(32 if kind != po.AES_128_GCM else 16), rng.bytes(12),
                         version=t13.VERSION)
    ctx = oracle.aead(okind, p.key)
    table = ta.SessionTable(engine, 1)
    table.install(0, [p])
    seals, opens = [], []
    for i, n in enumerate(lengths):
        seq, itype, content = (1 << 36) + i, 21 + i % 3, rng.bytes(n)
        frag = seal13(oracle, ctx, p.fixed_iv, seq, itype, content)
        if limit is not None and n > limit:
            seals.append(bi.Entry(0, seq, itype, content, ta.REC_PUBLIC_INVALID, b"",
                                  reserve=len(frag)))
            opens.append(bi.Entry(0, seq, 23, frag, ta.REC_PUBLIC_INVALID, b"", reserve=n + 1))
        else:
            seals.append(bi.Entry(0, seq, itype, content, len(frag), frag))
            # open: the status is the content length, the region the inner plaintext
            opens.append(bi.Entry(0, seq, 23, frag, n, content + bytes([itype])))
    for seal, entries in ((True, seals), (False, opens)):
        mix = [3 if i % 2 == 0 else 5 for i in range(len(entries))]
        bi.run_image(ta, engine, table, entries, seal, label=(kind, impl_label, seal, "aligned"))
        bi.run_image(ta, engine, table, entries, seal, in_shifts=mix, out_shifts=mix[::-1],
                     label=(kind, impl_label, seal, "shifted"))
    table.close()


@pytest.mark.parametrize("impl", ["queue", "split", "ttable"])
@pytest.mark.parametrize("name", list(KINDS))
def test_tls13_gcm_limit_bounds_the_inner_plaintext(ta, engine, oracle, gcm_impl, name, impl):
    gcm_impl(impl)
    run13(ta, engine, oracle, KINDS[name], KINDS[name], [17, BITS[1], MAX - 1, 16384, MAX, 17],
          MAX - 1, impl)


def test_tls13_chacha_has_no_limit(ta, engine, oracle):
    run13(ta, engine, oracle, ta.CHACHA20_POLY1305_TLS13, po.CHACHA20_POLY1305,
          [17, MAX + 16, 16384, 17], None, "chacha")
