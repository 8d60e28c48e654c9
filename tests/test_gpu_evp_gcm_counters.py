"""EVP_AEAD AES-GCM on the GPU where the block counter is not small: the 32-bit
wrap, counters past 2^16 and 2^24, and jobs above 1 MiB.

With an IV that is not 12 bytes J0 = GHASH(IV), so the low 32 bits of the
counter block start anywhere, and gcm128.c increments those 32 bits alone
(inc32, no carry into byte 11).  Random IVs come within a job's length of 2^32
about once in 10^6 cases; the IVs here are solved (tests/gcm_iv_craft.py) so the
counter is 0 at a chosen block w of the job: in the first block, inside wave 0's
range, at a wave-range boundary of gcm_raw_job (64 * spw blocks), in the
two-steps-per-iteration loop of gcm_blocks with ctr0 + i and ctr0 + i + 64 on
either side, on the partial last block, and for n = 0 in E_K(J0) alone.  Two
controls cross 2^16 and 2^24 without wrapping (a carry into the wrong byte, the
16-bit-counter fast path).  A 2^20 + 33 byte job per kind has more than 2^16
blocks, spw = 65 steps per wave and about 1,000 extra Horner steps in the
closing loop of every wave but the last.

The expected bytes are the CPU oracle's, computed once; tests/
test_gcm_counter_model.py pins the oracle on the same cases to the
block-by-block inc32 model, to the reference and to a reference-made golden
file.  Every case runs on each EVP route in a fresh process (the doorbell can
only be set before the first EVP call), which asserts its route by the stats:
the launched gcm_raw_kernel, the doorbell server, the coalescing queue.  Per
case: the seal equals the oracle's, the open of the oracle's output gives the
plaintext, and one flipped bit returns 0 and zero-fills max_out = n + 5 bytes.
"""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

import gcm_iv_craft as gic
import pyoracle as po
from conftest import ROOT

pytestmark = pytest.mark.gpu

LARGE_N = (1 << 20) + 33
ROUTES = {  # route: its environment; the queue child calls evp_set_batching(300, 0, 64)
    "launch": {"TLSGPU_EVP_DOORBELL": "0"},
    "doorbell": {"TLSGPU_EVP_DOORBELL": "4"},
    "queue": {},
}

_CHILD = r"""
import faulthandler; faulthandler.enable()
import os, pickle, sys, threading
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "oracle"))
import talos_amd as ta
route, jobs = sys.argv[2], pickle.load(open(sys.argv[3], "rb"))
ta.load_library()
if route == "queue":
    ta.evp_set_batching(300, 0, 64)
errors = []
def run(job):
    name, kind, key, tag_len, iv, aad, pt, sealed = job
    ctx = ta.EvpAead(kind, key, tag_len)
    try:
        assert ctx.ok == 1, name
        ok, got, ol = ctx.seal(iv, pt, aad)
        assert ok == 1 and ol == len(sealed), (name, "seal", ok, ol)
        if got != sealed:
            bad = next(i for i in range(len(sealed)) if got[i] != sealed[i])
            raise AssertionError((name, "seal differs from the oracle first at byte", bad,
                                  "block", bad // 16, "of", len(pt)))
        ok, back, ol = ctx.open(iv, sealed, aad)
        assert ok == 1 and ol == len(pt) and back == pt, (name, "open", ok, ol)
        # one flipped bit: in the ciphertext's middle block, or in the tag's last byte
        pos = len(pt) // 2 if len(key) == 16 else len(sealed) - 1
        bad = bytearray(sealed)
        bad[pos] ^= 0x20
        ok, z, ol = ctx.open(iv, bytes(bad), aad, max_out=len(pt) + 5)
        assert ok == 0 and ol == 0 and z == bytes(len(pt) + 5), (name, "tampered", pos, ok, ol)
    finally:
        ctx.cleanup()
def worker(t, nthreads):
    try:
        for job in jobs[t::nthreads]:
            run(job)
    except BaseException as exc:
        errors.append(repr(exc))
nthreads = 4 if route == "queue" else 1
ths = [threading.Thread(target=worker, args=(t, nthreads)) for t in range(nthreads)]
[th.start() for th in ths]; [th.join() for th in ths]
assert not errors, errors[:3]
db_jobs, _ = ta.evp_doorbell_stats()
_, q_jobs = ta.evp_batch_stats()
if route == "launch":
    assert db_jobs == 0 and q_jobs == 0, (db_jobs, q_jobs)
elif route == "doorbell":
    # the opens are never a context's first call: all of them are served by the doorbell
    assert db_jobs >= 2 * len(jobs) and q_jobs == 0, (db_jobs, q_jobs, len(jobs))
else:
    assert q_jobs >= 3 * len(jobs), (q_jobs, len(jobs))   # seal, open, tampered open
print("OK", route, len(jobs), db_jobs, q_jobs)
"""


def _job(oracle, name, kind, key, tag_len, iv, aad, pt):
    ctx = oracle.aead(kind, key, tag_len)
    ok, sealed = oracle.seal(ctx, iv, pt, aad)
    assert ok == 1 and len(sealed) == len(pt) + tag_len
    return (name, kind, key, tag_len, iv, aad, pt, sealed)


@pytest.fixture(scope="module")
def job_files(oracle, tmp_path_factory):
    """The inputs and the oracle's sealed outputs, computed once for all routes."""
    d = tmp_path_factory.mktemp("evp_gcm_counters")
    wrap = []
    for index, case in enumerate(gic.wrap_cases()):
        for key_len in gic.KEY_LENS:
            key, iv, aad, pt = gic.case_inputs(oracle, case, key_len, index)
            kind = po.AES_128_GCM if key_len == 16 else po.AES_256_GCM
            wrap.append(_job(oracle, f"{case['id']}-iv{case['iv_len']}-k{key_len * 8}", kind, key,
                             case["tag_len"], iv, aad, pt))
    rng = np.random.default_rng(0xC712)
    large = []
    for kind in (po.AES_128_GCM, po.AES_256_GCM, po.CHACHA20_POLY1305):
        key, iv, aad = (rng.integers(0, 256, n, dtype=np.uint8).tobytes()
                        for n in (po.KEY_LEN[kind], 12, 13))
        pt = rng.integers(0, 256, LARGE_N, dtype=np.uint8).tobytes()
        large.append(_job(oracle, f"large-kind{kind}", kind, key, 16, iv, aad, pt))
    files = {}
    for part, jobs in (("wrap", wrap), ("large", large)):
        files[part] = str(d / f"{part}.pickle")
        with open(files[part], "wb") as f:
            pickle.dump(jobs, f)
    return files


@pytest.mark.parametrize("part", ["wrap", "large"])
@pytest.mark.parametrize("route", list(ROUTES))
def test_evp_gcm_counters(job_files, route, part):
    env = dict(os.environ, TLSGPU_CRASH_TRACE="1")
    for name in ("TLSGPU_EVP_BATCH_US", "TLSGPU_EVP_DOORBELL"):
        env.pop(name, None)
    env.update(ROUTES[route])
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, route, job_files[part]], env=env,
                       capture_output=True, text=True, timeout=100)
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
