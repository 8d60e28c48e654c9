"""tlsgpu_session_params.tag_len other than 16 on the record paths, the parts
that need no GPU.

* The model the GPU tests (test_gpu_tag_len.py, test_gpu_tag_len_paths.py)
  compare with: pyoracle's generic framing, tls_seal_record / tls_open_record
  (tls1_enc, t1_enc.c:832-975) over an AEAD of tag length t.  A truncated tag
  is a prefix of the full one, so the sealed body is the 16-byte-tag session's
  body without its last 16 - t bytes; a valid record opens, a tampered one is
  -1 and zeros; and the reference's own AEAD at tag length t (where oracle/_ref
  is built) gives the same bodies.
* The engine's host code under the recording HIP stub (tests/devstub, as in
  test_tls13_padding.py): tlsgpu_seal_host / tlsgpu_open_host on tables whose
  sessions have tag_len 12 and 5 copy back exactly [out_off, out_off + eiv + n
  + t) and [out_off, out_off + n) per chunk; tlsgpu_seal_wire_size with a tag
  length; and the install rules (17 is TLSGPU_EINVAL, 0 means 16).
"""
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import pyoracle as po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUB_DIR = os.path.join(ROOT, "tests", "devstub")
STUB_LIB = os.path.join(STUB_DIR, "libtlsgpu_devstub.so")

KINDS = [po.AES_128_GCM, po.AES_256_GCM, po.CHACHA20_POLY1305, po.CHACHA20_POLY1305_OLD]
TAGS = [1, 4, 8, 12, 13, 15, 16]
LENGTHS = [0, 1, 3, 7, 17, 1000]


def _eiv(kind):
    return 8 if kind in (po.AES_128_GCM, po.AES_256_GCM) else 0


def _cases(impl, oracle, kind):
    """(t, seq, type, plaintext, full body of the 16-byte-tag session, body at t, AEAD at t)"""
    rng = np.random.default_rng(100 + kind)
    key, iv = rng.bytes(po.KEY_LEN[kind]), rng.bytes(po.FIXED_IV_LEN[kind])
    full = oracle.tls_session(kind, key, iv)
    for t in TAGS:
        ctx = impl.aead(kind, key, t)
        assert ctx is not None
        for i, n in enumerate(LENGTHS):
            seq, rtype, pt = (1 << 40) + 97 * t + i, 21 + i % 3, rng.bytes(n)
            yield (t, seq, rtype, pt, iv, oracle.tls_seal(full, seq, rtype, pt),
                   po.tls_seal_record(impl, ctx, kind, iv, seq, rtype, pt), ctx)


def _full_session(oracle, kind):
    """The 16-byte-tag session of _cases' key (the same generator state)."""
    rng = np.random.default_rng(100 + kind)
    return oracle.tls_session(kind, rng.bytes(po.KEY_LEN[kind]), rng.bytes(po.FIXED_IV_LEN[kind]))


@pytest.mark.parametrize("kind", KINDS)
def test_truncated_tag_is_a_prefix_and_opens(oracle, kind):
    for t, seq, rtype, pt, iv, full, body, ctx in _cases(oracle, oracle, kind):
        assert len(full) == _eiv(kind) + len(pt) + 16
        assert body == full[:len(full) - (16 - t)], (t, len(pt))
        assert po.tls_open_record(oracle, ctx, kind, iv, seq, rtype, body, tag_len=t) == (1, pt), \
            (t, len(pt))
        # one byte short of explicit nonce + tag: tls1_enc returns 0
        assert po.tls_open_record(oracle, ctx, kind, iv, seq, rtype, body[:_eiv(kind) + t - 1],
                                  tag_len=t) == (0, b"")


@pytest.mark.parametrize("kind", KINDS)
def test_tampered_record_is_bad_mac_and_zeros(oracle, kind):
    full_sess = _full_session(oracle, kind)
    for t, seq, rtype, pt, iv, full, body, ctx in _cases(oracle, oracle, kind):
        for at in (len(body) - 1, len(body) - t):          # last and first kept tag byte
            bad = bytearray(body)
            bad[at] ^= 0x10
            assert po.tls_open_record(oracle, ctx, kind, iv, seq, rtype, bytes(bad), tag_len=t) == \
                (-1, bytes(len(pt))), (t, len(pt), at)
        if pt:
            # a ciphertext bit: both ciphers are XOR streams, so the tampered ciphertext is
            # the ciphertext of the plaintext with that bit flipped, and the 16-byte-tag
            # session gives its true tag.  A tag of t bytes lets one forgery in 2^(8t) pass.
            e, at = _eiv(kind), len(pt) // 2
            bad = bytearray(body)
            bad[e + at] ^= 0x10
            pt2 = bytearray(pt)
            pt2[at] ^= 0x10
            true = oracle.tls_seal(full_sess, seq, rtype, bytes(pt2))
            assert true[:e + len(pt)] == bytes(bad[:e + len(pt)])
            passes = true[e + len(pt):e + len(pt) + t] == body[e + len(pt):]
            assert not passes or t == 1, (t, len(pt))
            assert po.tls_open_record(oracle, ctx, kind, iv, seq, rtype, bytes(bad), tag_len=t) == \
                ((1, bytes(pt2)) if passes else (-1, bytes(len(pt)))), (t, len(pt))
        # the record type is part of the additional data
        assert po.tls_open_record(oracle, ctx, kind, iv, seq, rtype ^ 1, body, tag_len=t)[0] == -1


@pytest.mark.parametrize("kind", KINDS)
def test_reference_aead_gives_the_same_bodies(oracle, reference, kind):
    for t, seq, rtype, pt, iv, full, body, ctx in _cases(reference, oracle, kind):
        assert body == full[:len(full) - (16 - t)], (t, len(pt))
        assert po.tls_open_record(reference, ctx, kind, iv, seq, rtype, body, tag_len=t) == (1, pt)


# -- under the recording stub --------------------------------------------------

_CHILD = r"""
import ctypes as C, json, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import talos_amd as ta
lib = ta.load_library()
lib.devstub_trace_begin.restype = None
lib.devstub_trace_begin.argtypes = [C.c_int]
lib.devstub_trace_take.restype = C.c_size_t
lib.devstub_trace_take.argtypes = [C.c_char_p, C.c_size_t]
_buf = C.create_string_buffer(1 << 22)
out = {}
E = ta.Engine(0)
KINDS = [ta.AES_128_GCM, ta.AES_256_GCM, ta.CHACHA20_POLY1305, ta.CHACHA20_POLY1305_OLD]

def install(kind, tag):
    tab = ta.SessionTable(E, 1)
    p = ta.SessionParams(kind, bytes(ta.KEY_LEN[kind]), bytes(ta.FIXED_IV_LEN[kind]), tag_len=tag)
    rc = tab.lib.tlsgpu_sessions_install(tab.handle, 0, 1, C.byref(p.to_c()))
    tab.close()
    return rc
out["install"] = {str(t): [install(k, t) for k in KINDS] for t in range(0, 20)}

out["sizes"] = [[k, n, mf, t, int(lib.tlsgpu_seal_wire_size(k, n, mf, t))]
                for k in KINDS for t in (0, 1, 5, 8, 12, 15, 16)
                for mf in (0, 1, 1000, 4096, 16384, 20000)
                for n in (0, 1, 999, 1000, 1001, 16383, 16384, 16385, 40000, 1 << 20)]

# host pipeline traces: N records of 100 bytes, four runs of two sessions (tags 12 and 5)
N, PT, SLOT = 4000, 100, 100 + 8 + 16 + 3
TAGS = [12, 5]
def pinned(nbytes):
    p = C.c_void_p()
    assert lib.tlsgpu_host_alloc(E.handle, nbytes, C.byref(p)) == 0
    return p.value
HB = N * SLOT
h_in, h_out, h_st = pinned(HB), pinned(HB), pinned(4 * N)
i = np.arange(N, dtype=np.uint64)
sess = ((i // np.uint64(N // 4)) % np.uint64(2)).astype(np.uint32)
traces = {}
for name, kinds in (("gcm", (ta.AES_128_GCM, ta.AES_256_GCM)),
                    ("chacha", (ta.CHACHA20_POLY1305, ta.CHACHA20_POLY1305_OLD))):
    eiv = ta.EXPLICIT_NONCE_LEN[kinds[0]]
    for seal in (True, False):
        eng = ta.Engine(0)
        ta.host_pipeline(eng, 4, 64 << 10)
        tab = ta.SessionTable(eng, 2)
        tab.install(0, [ta.SessionParams(k, bytes([j + 1]) * ta.KEY_LEN[k],
                                         bytes(ta.FIXED_IV_LEN[k]), tag_len=t)
                        for j, (k, t) in enumerate(zip(kinds, TAGS))])
        r = np.zeros(N, dtype=ta.RECORD_DTYPE)
        r["in_off"] = i * np.uint64(SLOT)
        r["out_off"] = i * np.uint64(SLOT)
        r["seq"] = i
        r["session"] = sess
        r["len_type"] = (23 << 24) | (PT if seal else PT + eiv + np.asarray(TAGS, dtype=np.uint32)[sess])
        lib.devstub_trace_begin(0)
        try:
            (ta.seal_host if seal else ta.open_host)(tab, r.ctypes.data, N, h_in, HB, h_out, HB, h_st)
        finally:
            k = lib.devstub_trace_take(_buf, len(_buf))
        assert 0 < k < len(_buf)
        traces["%s/%s" % (name, "seal" if seal else "open")] = _buf.value.decode()
        tab.close()
        eng.close()
out["traces"] = traces
out["layout"] = [N, PT, SLOT, TAGS, sess.tolist()]
print("RESULT " + json.dumps(out))
"""


@pytest.fixture(scope="module")
def stub():
    if not shutil.which("hipcc") and not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc not available to build the stub library")
    subprocess.run(["make", "-C", STUB_DIR, "-s"], check=True, capture_output=True)
    env = dict(os.environ, TLSGPU_LIBRARY=STUB_LIB, TLSGPU_STUB_DEVICES="1", TLSGPU_EVP_DOORBELL="0")
    for k in [k for k in env if k.startswith("TLSGPU_") and
              k not in ("TLSGPU_LIBRARY", "TLSGPU_STUB_DEVICES", "TLSGPU_EVP_DOORBELL")]:
        env.pop(k)
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT], env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


def test_install_rules(stub):
    """tag_len 0 means 16 and installs, 1..16 install, 17 and above are TLSGPU_EINVAL,
    for every TLS 1.2 kind."""
    for t in range(0, 17):
        assert stub["install"][str(t)] == [0, 0, 0, 0], t
    for t in (17, 18, 19):
        assert stub["install"][str(t)] == [-1, -1, -1, -1], t


def test_seal_wire_size_with_a_tag_length(stub):
    for kind, n, mf, t, got in stub["sizes"]:
        frag = 16384 if mf == 0 or mf > 16384 else mf
        nrec = (n + frag - 1) // frag
        assert got == nrec * (5 + _eiv(kind) + (t or 16)) + n, (kind, n, mf, t)


def _copies_out(trace):
    """(offset, bytes) of the device-to-host copies of output: every D2H copy but
    the last one, which brings the statuses back."""
    out = []
    for line in trace.splitlines():
        f = dict(x.split("=", 1) for x in line.split()[1:] if "=" in x)
        if line.startswith("hipMemcpyAsync") and f["kind"] == "2":
            dst, src = f["dst"].split("+"), f["src"].split("+")
            out.append((dst[0], int(dst[1]), src[0], int(src[1]), int(f["bytes"])))
    assert out and out[-1][1] == 0 and out[-1][3] == 0          # the statuses
    body = out[:-1]
    assert len({(c[0], c[2]) for c in body}) == 1               # one host buffer, one mirror
    assert all(c[1] == c[3] for c in body)                      # the same offset in both
    return [(c[1], c[4]) for c in body]


@pytest.mark.parametrize("name", ["gcm", "chacha"])
@pytest.mark.parametrize("mode", ["seal", "open"])
def test_host_pipeline_spans(stub, name, mode):
    """Each chunk's copy back runs from its first record's out_off to the end of
    its last record's output span: explicit nonce + n + the session's tag on
    seal, n on open.  The chunks partition the records, and chunks end inside
    runs of both sessions."""
    n, pt, slot, tags, sess = stub["layout"]
    eiv = 8 if name == "gcm" else 0
    copies = _copies_out(stub["traces"]["%s/%s" % (name, mode)])
    assert len(copies) >= 5
    at, last_sessions = 0, set()
    for off, nbytes in copies:
        assert off == at * slot, (off, at)
        end = off + nbytes
        last = (end - 1) // slot
        span = eiv + pt + tags[sess[last]] if mode == "seal" else pt
        assert end == last * slot + span and last >= at, (off, nbytes, last, sess[last])
        last_sessions.add(sess[last])
        at = last + 1
    assert at == n and last_sessions == {0, 1}
