"""tlsgpu_session_params.tag_len other than 16 on the batch paths, on the GPU.

valid_params accepts a tag of 1..16 bytes for every TLS 1.2 kind, and every batch
kernel has code for it: gcm_tag's lane mask, parse_tls, gcm_pack's byte loops and
keep mask, pack_need / rec_in_bounds, cc_record and the staged ChaCha kernel's end
of record, the fused ChaCha bounds rule, and check_record_bounds.  Here tables of
eight sessions with tag lengths 0 (= 16), 1, 4, 8, 12, 13, 15 and 16 run through
every kernel route, seal and open, against the model of tests/batch_image.py
(pyoracle's tls1_enc framing over the oracle's AEAD at that tag length; checked
on the CPU in test_tag_len_model.py).  batch_image.run_image lays the batches out
and compares the whole output image, every status and the slack behind both
buffers; RecordBatch, whose slots assume 16, is not used.

Per session, plaintexts of 0, 1, 15, 16, 17, 991, 992, 993, 1024, 1040, 4097 and
16384 bytes (the pack limit of 62 blocks is decided from len - eiv - tag_len on
open, so 991..993 are there for every tag length).  A seal must leave the 16 - t
bytes behind a truncated tag alone.  An open batch adds per session:
  (a) the fragment of exactly eiv + t bytes (the empty record): status 0;
  (b) eiv + t - 1 bytes: TLSGPU_REC_PUBLIC_INVALID, nothing written;
  (c) a bit flipped in the last kept tag byte, and one in the first:
      TLSGPU_REC_BAD_MAC, exactly n bytes zeroed;
  (d) a bit flipped in the ciphertext: the same;
  (e) one valid fragment twice, once followed in d_in by the rest of the
      untruncated tag and once by its complement: those bytes are outside the
      record's length, so both open alike.
Orders: grouped by session, interleaved (neighbouring lanes of a ChaCha wave then
hold sessions of different tag lengths), and for the ChaCha tables two whole waves
of one session each ahead of the interleaved records.  Slots are aligned, or
shifted by 3 and 5 bytes in turn.  Every run ends its buffers exactly at the last
record; one run per case ends d_out a byte early.  Open also runs in place.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import batch_image as bi
import pyoracle as po

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAGS = [0, 1, 4, 8, 12, 13, 15, 16]
LENGTHS = [0, 1, 15, 16, 17, 991, 992, 993, 1024, 1040, 4097, 16384]
A1, A2, CC, OLD = po.AES_128_GCM, po.AES_256_GCM, po.CHACHA20_POLY1305, po.CHACHA20_POLY1305_OLD
TABLES = {"aes-128": [A1] * 8, "aes-256": [A2] * 8, "aes-mixed": [A1, A2, A1, A2, A2, A1, A2, A1],
          "chacha": [CC] * 8, "chacha-old": [OLD] * 8, "all-kinds": [A1, CC, A2, OLD, CC, A1, OLD, A2]}
GCM_TABLES = ["aes-128", "aes-256", "aes-mixed"]
CHACHA_TABLES = ["chacha", "chacha-old"]
# (gcm impl, hints): the queue kernel's fused no-pack and pack variants and its
# device-side selection, the split and T-table kernels, the default choice, and
# the experimental kernels where they are built
ROUTES = [("queue", 3), ("queue", 2), ("queue", 0), ("split", 0), ("ttable", 0), ("auto", 0),
          ("hybrid", 0), ("bitslice", 0), ("fused", 0)]
EXPERIMENTAL_IMPLS = ("hybrid", "bitslice", "fused")


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


def _flip(frag, at, bit=0):
    b = bytearray(frag)
    b[at] ^= 1 << bit
    return bytes(b)


def _tampered(ta, oracle, sessions, sid, seq, rtype, frag, at):
    """`frag` with one bit of byte `at` flipped, the first bit with which the model
    rejects it (a one-byte tag lets one forged ciphertext in 256 pass)."""
    for bit in range(8):
        e = bi.open_entry(ta, oracle, sessions, sid, seq, rtype, _flip(frag, at, bit))
        if e.st == ta.REC_BAD_MAC:
            return e
    raise AssertionError("the model accepts every flip")


def material(ta, oracle, name):
    """(sessions, per session the seal entries, per session the open entries),
    computed once per table."""
    if name not in _cache:
        kinds = TABLES[name]
        sessions = bi.make_sessions(ta, oracle, kinds, TAGS, 1000 + sorted(TABLES).index(name))
        rng = np.random.default_rng(len(name))
        seals, opens = [], []
        for sid, s in enumerate(sessions):
            se, oe, frags = [], [], {}
            for j, n in enumerate(LENGTHS):
                seq, rtype = (1 << 33) + 4096 * sid + j, 21 + (sid + j) % 3
                e = bi.seal_entry(ta, oracle, sessions, sid, seq, rtype, rng.bytes(n))
                se.append(e)
                frags[n] = e
                o = bi.open_entry(ta, oracle, sessions, sid, seq, rtype, e.out)
                assert (o.st, o.out) == (n, e.inp)                      # (a) is n = 0
                oe.append(o)
            e = frags[0]                                                # (b)
            assert len(e.out) == s.eiv + s.t
            o = bi.open_entry(ta, oracle, sessions, sid, e.seq, e.rtype, e.out[:-1])
            assert o.st == ta.REC_PUBLIC_INVALID
            oe.append(o)
            for n, at in ((993, -1), (17, -s.t), (1040, -1), (0, -s.t),  # (c) last / first kept byte
                          (1024, s.eiv + 1023), (15, s.eiv), (4097, s.eiv + 4000)):   # (d)
                e = frags[n]
                oe.append(_tampered(ta, oracle, sessions, sid, e.seq, e.rtype, e.out,
                                    at % len(e.out)))
            for n in (991, 16):                                         # (e)
                e = frags[n]
                rest = bi.model_seal(oracle, s, e.seq, e.rtype, e.inp, full=True)[len(e.out):]
                assert len(rest) == 16 - s.t
                for bait in (rest, bytes(b ^ 0xFF for b in rest)):
                    o = bi.open_entry(ta, oracle, sessions, sid, e.seq, e.rtype, e.out, bait)
                    assert o.st == n
                    oe.append(o)
            seals.append(se)
            opens.append(oe)
        _cache[name] = (sessions, seals, opens)
    return _cache[name]


def ordered(per_session, order):
    """grouped: session after session.  interleaved: record j of every session,
    then record j + 1.  waves: 64 records of session 4 and 64 of session 1 (two
    whole ChaCha waves of one session each), then interleaved.  Each order ends
    with a record whose output is not empty, so the buffers can end exactly at it."""
    if order == "grouped":
        out = [e for es in per_session for e in es]
    else:
        depth = max(len(es) for es in per_session)
        out = [es[j] for j in range(depth) for es in per_session if j < len(es)]
        if order == "waves":
            head = [per_session[sid][j % len(per_session[sid])] for sid in (4, 1) for j in range(64)]
            out = head + out
    tail = next(e for e in per_session[3] if e.st > 16)
    return out + [tail]


def run_table(ta, engine, oracle, name, mode, hints=None, orders=("grouped", "interleaved")):
    sessions, seals, opens = material(ta, oracle, name)
    table = ta.SessionTable(engine, len(sessions))
    table.install(0, [s.params for s in sessions])
    if hints is not None:
        table.hint(hints)
    seal = mode == "seal"
    for order in orders:
        entries = ordered(seals if seal else opens, order)
        n = len(entries)
        mix = [3 if i % 2 == 0 else 5 for i in range(n)]
        label = (name, mode, hints, order)
        bi.run_image(ta, engine, table, entries, seal, label=label + ("aligned",))
        bi.run_image(ta, engine, table, entries, seal, in_shifts=mix, out_shifts=mix[1:] + [3],
                     label=label + ("shifted",))
        bi.run_image(ta, engine, table, entries, seal, cut=1, out_shifts=mix,
                     label=label + ("d_out a byte short",))
        if not seal:
            bi.run_image(ta, engine, table, entries, False, in_place=True,
                         label=label + ("in place",))
    table.close()


@pytest.mark.parametrize("mode", ["seal", "open"])
@pytest.mark.parametrize("impl,hints", ROUTES, ids=["%s-%d" % r for r in ROUTES])
@pytest.mark.parametrize("name", GCM_TABLES)
def test_gcm_routes(ta, engine, oracle, gcm_impl, name, impl, hints, mode):
    gcm_impl(impl)
    run_table(ta, engine, oracle, name, mode, hints)


@pytest.mark.parametrize("mode", ["seal", "open"])
@pytest.mark.parametrize("name", CHACHA_TABLES)
def test_chacha_tables(ta, engine, oracle, name, mode):
    """RFC ChaCha only is the fused staged kernel (its own bounds rule); the draft
    suite runs on chacha_batch_kernel (cc_record)."""
    run_table(ta, engine, oracle, name, mode, orders=("grouped", "waves"))


@pytest.mark.parametrize("mode", ["seal", "open"])
@pytest.mark.parametrize("impl,hints", [("queue", 0), ("auto", 0)])
def test_all_kinds_in_one_table(ta, engine, oracle, gcm_impl, impl, hints, mode):
    gcm_impl(impl)
    run_table(ta, engine, oracle, "all-kinds", mode, hints, orders=("grouped", "waves"))


def _child(env, names, orders):
    code = ("import sys; sys.path[:0] = [%r, %r]\n"
            "import test_gpu_tag_len as t, pyoracle as po, talos_amd as ta\n"
            "ta.load_library(); e = ta.Engine(0); o = po.Oracle()\n"
            "for name in %r:\n"
            "    for mode in ('seal', 'open'):\n"
            "        t.run_table(ta, e, o, name, mode, orders=%r)\n"
            "e.close(); print('ok')\n") % (os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"),
                                           names, orders)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=110,
                       env=dict(os.environ, **env), cwd=ROOT)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stderr[-3000:]


def test_per_wave_session_kernel_forced():
    """TLSGPU_PWS=1 (gcm_pw.hip) over the GCM tables, in a child process."""
    _child({"TLSGPU_PWS": "1", "TLSGPU_GCM_IMPL": "queue"}, GCM_TABLES, ("grouped", "interleaved"))


def test_legacy_chacha_kernel_forced():
    """TLSGPU_CHACHA_LEGACY=1 over the ChaCha tables, in a child process."""
    _child({"TLSGPU_CHACHA_LEGACY": "1"}, CHACHA_TABLES, ("grouped", "waves"))
