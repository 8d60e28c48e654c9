"""TLS 1.3 record padding on seal (tlsgpu_session_params.pad_block), the parts
that need no GPU.

* The rule and the framing model (tests/tls13_padding.py) against OpenSSL: a
  connection captured under RecordPadding = 512, AES-256-GCM and
  ChaCha20-Poly1305.  inner_len reproduces every record's inner plaintext
  length and the helper re-seals every record to the captured bytes.
* The engine's host code under the recording HIP stub (tests/devstub, as in
  test_batch_plan_trace.py): which pad_block values install, the arithmetic of
  tlsgpu_seal_wire_size_p, and the trace of tlsgpu_seal_host on padded tables:
  each chunk's device-to-host copy covers the padded fragments exactly, the
  derived hints follow the padded inner length, and the same descriptors on a
  table without padding give the copy and the launches of before.
"""
import base64
import json
import os
import shutil
import subprocess
import sys

import pytest

import pyoracle as po
import tls13_helper as t13
import tls13_padding as tp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUB_DIR = os.path.join(ROOT, "tests", "devstub")
STUB_LIB = os.path.join(STUB_DIR, "libtlsgpu_devstub.so")
FIXTURES = {tp.GOLDEN_PADDED: None, tp.GOLDEN_CHACHA_PADDED: po.CHACHA20_POLY1305}


def test_inner_len_rule():
    assert [tp.inner_len(n, 0) for n in (0, 1, 16383, 16384, 48000)] == [1, 2, 16384, 16385, 48001]
    assert [tp.inner_len(n, 1) for n in (0, 5)] == [1, 6]
    assert [tp.inner_len(n, 16) for n in (0, 14, 15, 16, 31, 991, 992)] == \
        [16, 16, 16, 32, 32, 992, 1008]
    assert [tp.inner_len(n, 512) for n in (0, 1, 510, 511, 512, 16382, 16383, 16384, 16400)] == \
        [512, 512, 512, 512, 1024, 16384, 16384, 16385, 16401]
    assert [tp.inner_len(n, 16384) for n in (0, 1, 16383, 16384)] == [16384, 16384, 16384, 16385]
    # RFC 8446 5.4: a padded TLSInnerPlaintext stays within 2^14 + 1
    for block in (2, 16, 64, 512, 4096, 16384):
        assert max(tp.inner_len(n, block) for n in range(0, 16385)) == 16385


@pytest.mark.parametrize("path", list(FIXTURES), ids=["aes-256-gcm", "chacha20-poly1305"])
def test_rule_and_framing_against_the_openssl_capture(oracle, path):
    fx = t13.load_fixture(path)
    block = fx["record_padding"]
    assert block == 512
    kind = FIXTURES[path] if FIXTURES[path] is not None else t13.SUITES[fx["suite"]][0]
    seen = []
    for d in fx["directions"]:
        ctx = oracle.aead(kind, d["key"])
        for r in d["records"]:
            hdr, frag = r["wire"][:5], r["wire"][5:]
            inner = len(frag) - t13.TAG
            assert inner == tp.inner_len(len(r["content"]), block), (r["seq"], inner)
            again = tp.seal(oracle, ctx, d["iv"], r["seq"], r["inner_type"], r["content"], block)
            assert hdr == t13.header(len(again)) and again == frag, r["seq"]
            if r["inner_type"] == 23:      # (the tickets' length depends on the suite's hash)
                seen.append((len(r["content"]), inner))
            else:
                assert r["inner_type"] == 22 and inner == 512
        # every write again as a tlsgpu_seal_wire stream would frame it
        app = [r for r in d["records"] if r["inner_type"] == 23]
        k = 0
        for w in d["writes"]:
            n = len(t13.frame(bytes(w)))
            recs = app[k:k + n]
            k += n
            data = b"".join(r["content"] for r in recs)
            want = b"".join(r["wire"] for r in recs)
            assert tp.seal_wire(oracle, ctx, d["iv"], recs[0]["seq"], 23, data, block) == want
            assert tp.seal_wire_size(len(data), block) == len(want)
    assert seen == [(1, 512), (16, 512), (1008, 1024), (49, 512), (992, 1024), (16384, 16385),
                    (1, 512)]


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

# install rules
def install(kind, key, iv, version, block):
    tab = ta.SessionTable(E, 1)
    p = ta.SessionParams(kind, key, iv, version=version, pad_block=block)
    rc = tab.lib.tlsgpu_sessions_install(tab.handle, 0, 1, C.byref(p.to_c()))
    tab.close()
    return rc
BLOCKS = [0, 1, 2, 16, 512, 16384, 3, 24, 32768, 65535]
out["install13"] = {str(b): [install(ta.AES_128_GCM, bytes(16), bytes(12), 0x0304, b),
                             install(ta.AES_256_GCM, bytes(32), bytes(12), 0x0304, b),
                             install(ta.CHACHA20_POLY1305_TLS13, bytes(32), bytes(12), 0x0304, b)]
                    for b in BLOCKS}
out["install12"] = {str(b): [install(ta.AES_128_GCM, bytes(16), bytes(4), 0x0303, b),
                             install(ta.CHACHA20_POLY1305, bytes(32), bytes(12), 0x0303, b),
                             install(ta.CHACHA20_POLY1305_OLD, bytes(32), b"", 0x0301, b)]
                    for b in BLOCKS}

# tlsgpu_seal_wire_size_p
sizes = []
for kind in (ta.AES_128_GCM, ta.AES_256_GCM, ta.CHACHA20_POLY1305, ta.CHACHA20_POLY1305_TLS13):
    for version in (0x0303, 0x0304):
        for block in (0, 1, 2, 16, 512, 4096, 16384):
            for frag in (0, 1, 1000, 16384, 20000):
                for n in (0, 1, 15, 511, 512, 999, 1000, 1001, 16383, 16384, 16385, 40000, 1 << 20):
                    sizes.append([kind, version, block, frag, n,
                                  int(lib.tlsgpu_seal_wire_size_p(kind, version, n, frag, 0, block)),
                                  int(lib.tlsgpu_seal_wire_size_v(kind, version, n, frag, 0))])
out["sizes"] = sizes

# tlsgpu_seal_host traces: N records of 100 bytes, two sessions
N, SLOT = 12000, 100 + 1024 + 16 + 2
r = np.zeros(N, dtype=ta.RECORD_DTYPE)
i = np.arange(N, dtype=np.uint64)
r["in_off"] = i * np.uint64(102)
r["out_off"] = i * np.uint64(SLOT)
r["seq"] = i
r["session"] = i // np.uint64(N // 2)
r["len_type"] = (23 << 24) | 100
def pinned(nbytes):
    p = C.c_void_p()
    assert lib.tlsgpu_host_alloc(E.handle, nbytes, C.byref(p)) == 0
    return p.value
HB = N * SLOT
h_in, h_out, h_st = pinned(HB), pinned(HB), pinned(4 * N)
traces = {}
for kind, name in ((ta.AES_128_GCM, "gcm"), (ta.CHACHA20_POLY1305_TLS13, "chacha")):
    for block in (0, 64, 1024):
        eng = ta.Engine(0)
        tab = ta.SessionTable(eng, 2)
        tab.install(0, [ta.SessionParams(kind, bytes([k + 1]) * ta.KEY_LEN[kind], bytes(12),
                                         version=0x0304, pad_block=block) for k in range(2)])
        lib.devstub_trace_begin(0)
        try:
            ta.seal_host(tab, r.ctypes.data, N, h_in, HB, h_out, HB, h_st)
        finally:
            k = lib.devstub_trace_take(_buf, len(_buf))
        assert 0 < k < len(_buf)
        traces["%s/%d" % (name, block)] = _buf.value.decode()
        tab.close()
        eng.close()
out["traces"] = traces
out["layout"] = [N, SLOT]
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
    """0x0304: 0 and 1 are no padding, a power of two from 2 to 16384 is the
    block, anything else is TLSGPU_EINVAL; every other version ignores the field."""
    for b in (0, 1, 2, 16, 512, 16384):
        assert stub["install13"][str(b)] == [0, 0, 0], b
    for b in (3, 24, 32768, 65535):
        assert stub["install13"][str(b)] == [-1, -1, -1], b
    for b, rcs in stub["install12"].items():
        assert rcs == [0, 0, 0], b


def test_seal_wire_size_p(stub):
    import talos_amd as ta
    for kind, version, block, frag, n, got, size_v in stub["sizes"]:
        t13_framing = kind == ta.CHACHA20_POLY1305_TLS13 or \
            (version == 0x0304 and kind in (ta.AES_128_GCM, ta.AES_256_GCM))
        if block <= 1 or not t13_framing or version != 0x0304:
            assert got == size_v, (kind, version, block, frag, n)
        else:
            assert got == tp.seal_wire_size(n, block, frag), (kind, version, block, frag, n)
        if t13_framing:
            assert size_v == t13.seal_wire_size(n, frag)


def _copies_out(trace):
    """(offset, bytes) of the device-to-host copies out of the output mirror (the
    second allocation of the trace), in order."""
    out = []
    for line in trace.splitlines():
        f = dict(x.split("=", 1) for x in line.split()[1:] if "=" in x)
        if line.startswith("hipMemcpyAsync") and f["kind"] == "2" and f["src"].startswith("a1+"):
            out.append((int(f["src"][3:]), int(f["bytes"])))
    return out


def _launches(trace):
    return [dict(x.split("=", 1) for x in line.split()[1:] if "=" in x) | {"name": line.split()[0]}
            for line in trace.splitlines() if line.startswith("launch_")]


@pytest.mark.parametrize("name", ["gcm", "chacha"])
def test_seal_host_spans_and_hints(stub, name):
    n, slot = stub["layout"]
    for block in (0, 64, 1024):
        trace = stub["traces"]["%s/%d" % (name, block)]
        frag = tp.inner_len(100, block) + 16
        copies = _copies_out(trace)
        assert len(copies) >= 2          # several chunks
        # the chunks partition the records; each copy is first out_off .. last fragment's end
        at = 0
        for off, nbytes in copies:
            assert off == at * slot, (block, off, at)
            last, rem = divmod(off + nbytes - frag, slot)
            assert rem == 0 and last >= at, (block, off, nbytes)
            at = last + 1
        assert at == n
        ls = _launches(trace)
        if name == "gcm":
            # no short records with a block of 1024 (inner 1024 > 992): the pack variant is
            # ruled out; 100-byte records pack with a block of 64 (inner 128) and with none
            q = [l for l in ls if l["name"] == "launch_gcm_queue"]
            assert q and all(l["pack"] == ("0" if block == 1024 else "1") for l in q), block
        else:
            assert ls and all(l["name"] == "launch_chacha" for l in ls)
    # without padding: the copy of the unpadded fragments, content + type + tag
    assert all((off + nbytes - 117) % slot == 0 for off, nbytes in
               _copies_out(stub["traces"][name + "/0"]))
    # the launches of a padded table differ from the unpadded one's in nothing the trace
    # shows but the hints (block 64 packs like no padding: the same launches)
    strip = lambda t: [l for l in t.splitlines() if l.startswith("launch_")]
    assert strip(stub["traces"][name + "/64"]) == strip(stub["traces"][name + "/0"])
