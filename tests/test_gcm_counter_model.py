"""CPU checks behind the GCM counter tests (tests/test_gpu_evp_gcm_counters.py,
tests/test_gpu_gcm_stream.py).

The GPU tests compare the engine with oracle.seal / pyoracle.GcmStream on IVs
made by tests/gcm_iv_craft.py so that the 32-bit block counter wraps (or
crosses 2^16 / 2^24) at a chosen block.  Here, without a GPU:

* craft_iv gives the start counter it was asked for, at every (key size, IV
  length, wrap index) the GPU tests use;
* the oracle's ciphertext on those IVs is the block-by-block inc32 model
  pt ^ E_K(J0[0:12] || be32((ctr + 1 + i) mod 2^32)), built from
  oracle.aes_encrypt alone: no carry into byte 11 of the counter block;
* oracle.seal and oracle.gcm agree, the reference itself (libref.so, where
  built) seals the same bytes, and tests/golden/gcm_ctr_wrap.json pins a dozen
  reference outputs for machines without the reference;
* pyoracle.GcmStream, the piecewise model of the stream-kernel test, equals
  one-shot oracle.gcm however the input is cut, and keeps gcm128.c's return
  codes (AAD after data: -2, state untouched).
"""
import hashlib
import json
import os
import random

import pytest

import gcm_iv_craft as gic
import pyoracle as po
from conftest import ROOT

CASES = gic.wrap_cases()
KINDS = {16: po.AES_128_GCM, 32: po.AES_256_GCM}
PARAMS = [pytest.param(i, kl, id=f"{c['id']}-iv{c['iv_len']}-k{kl * 8}")
          for i, c in enumerate(CASES) for kl in gic.KEY_LENS]
GOLDEN = os.path.join(ROOT, "tests", "golden", "gcm_ctr_wrap.json")
# (IV length, j0_ctr) of the stream-kernel test's crafted IVs
STREAM_IVS = [(ivl, (1 << 32) - 1 - w) for ivl in gic.STREAM_IV_LENS
              for w in [w for w, _ in gic.STREAM_WRAPS.values()] + [gic.STREAM_COPY_W]]


def test_gf128_helpers_match_the_oracle(oracle):
    rnd = random.Random(11)
    for _ in range(8):
        a, b = rnd.getrandbits(128), rnd.getrandbits(128)
        got = gic.gf_mul(a, b).to_bytes(16, "big")
        assert got == oracle.gf128_mul(a.to_bytes(16, "big"), b.to_bytes(16, "big"))
        assert gic.gf_mul(a, gic.gf_inv(a)) == gic.ONE
        assert gic.gf_pow(a, 5) == gic.gf_mul(gic.gf_mul(gic.gf_mul(a, a), gic.gf_mul(a, a)), a)
    from talos_amd.workload import fill_bytes
    for n in (0, 1, 8, 100):
        assert gic.fill(0x5EED0001, 7, n) == fill_bytes(0x5EED0001, 7, n)


def test_case_list_is_the_issue_table():
    """The shapes and wrap indices are fixed; every IV / tag / AAD length is used."""
    assert len(CASES) == 1 + 8 + 3 + 7 + 4 + 3 + 2
    assert {c["iv_len"] for c in CASES} == {16, 33, 60, 64}
    assert {(c["tag_len"], c["aad_len"]) for c in CASES} == {(t, a) for t in (16, 12)
                                                            for a in (0, 13, 100)}
    for c in CASES:
        if c["w"] is not None:
            assert (c["j0_ctr"] + 1 + c["w"]) % (1 << 32) == 0
            assert c["w"] <= (c["n"] + 15) // 16   # w == block count: only the counter after the last block is 0
    assert [c["j0_ctr"] for c in CASES if c["w"] is None] == [0x0000FFF0, 0x00FFFFC0]


@pytest.mark.parametrize("key_len", gic.KEY_LENS)
@pytest.mark.parametrize("iv_len,j0_ctr", STREAM_IVS)
def test_craft_iv_for_the_stream_cases(oracle, key_len, iv_len, j0_ctr):
    key = gic.fill(0xC7130000 + iv_len, key_len, key_len)
    iv = gic.craft_iv(oracle, key, iv_len, j0_ctr, 5)
    assert len(iv) == iv_len
    assert int.from_bytes(gic.j0_of(oracle, key, iv)[12:], "big") == j0_ctr
    pt = bytes(48)
    assert oracle.gcm(key, iv, b"", pt)[0] == gic.ctr_model_encrypt(oracle, key, iv, pt)


@pytest.mark.parametrize("index,key_len", PARAMS)
def test_oracle_is_the_inc32_model(oracle, index, key_len):
    case = CASES[index]
    key, iv, aad, pt = gic.case_inputs(oracle, case, key_len, index)
    j0 = gic.j0_of(oracle, key, iv)
    assert len(iv) == case["iv_len"] and int.from_bytes(j0[12:], "big") == case["j0_ctr"]
    ct, tag = oracle.gcm(key, iv, aad, pt)
    assert ct == gic.ctr_model_encrypt(oracle, key, iv, pt)
    if case["w"] is not None and 16 * case["w"] < len(pt):
        # the wrapped block's keystream is E_K(J0[0:12] || 0^32): bytes 0..11 unchanged
        w = case["w"]
        ks = oracle.aes_encrypt(key, j0[:12] + bytes(4))
        assert ct[16 * w:16 * w + 16] == bytes(a ^ b for a, b in zip(pt[16 * w:16 * w + 16], ks))
    ctx = oracle.aead(KINDS[key_len], key, case["tag_len"])
    ok, sealed = oracle.seal(ctx, iv, pt, aad)
    assert ok == 1 and sealed == ct + tag[:case["tag_len"]]
    ok, back = oracle.open(ctx, iv, sealed, aad)
    assert ok == 1 and back == pt


@pytest.mark.parametrize("index,key_len", PARAMS)
def test_reference_seals_the_same_bytes(oracle, reference, index, key_len):
    """The 32-bit wrap is the reference's behaviour, not only the oracle's reading of it."""
    case = CASES[index]
    key, iv, aad, pt = gic.case_inputs(oracle, case, key_len, index)
    octx = oracle.aead(KINDS[key_len], key, case["tag_len"])
    rctx = reference.aead(KINDS[key_len], key, case["tag_len"])
    exp = reference.seal(rctx, iv, pt, aad)
    assert exp[0] == 1 and oracle.seal(octx, iv, pt, aad) == exp
    assert reference.open(rctx, iv, exp[1], aad) == (1, pt)


def test_oracle_matches_the_reference_made_golden_file(oracle):
    """tests/golden/gcm_ctr_wrap.json (make_golden.py --ctr-wrap, from libref.so):
    the anchor where the reference is not built."""
    g = json.load(open(GOLDEN))
    assert len(g["cases"]) >= 12
    seen = set()
    for c in g["cases"]:
        key, iv, aad = (bytes.fromhex(c[k]) for k in ("key", "iv", "aad"))
        pt = gic.fill(c["pt_seed"], c["pt_index"], c["pt_len"])
        assert int.from_bytes(gic.j0_of(oracle, key, iv)[12:], "big") == c["j0_ctr"]
        ctx = oracle.aead(KINDS[len(key)], key, c["tag_len"])
        ok, sealed = oracle.seal(ctx, iv, pt, aad)
        assert ok == 1 and len(sealed) == c["sealed_len"], c["id"]
        assert hashlib.sha256(sealed).hexdigest() == c["sealed_sha256"], c["id"]
        assert sealed[:32].hex() == c["first32"] and sealed[-32:].hex() == c["last32"], c["id"]
        seen.add((len(key), c["w"] is None))
    assert seen == {(16, False), (32, False), (16, True), (32, True)}


# ---- the streaming model -------------------------------------------------------

@pytest.mark.parametrize("key_len", gic.KEY_LENS)
@pytest.mark.parametrize("decrypt", [False, True])
def test_gcm_stream_piecewise_equals_one_shot(oracle, key_len, decrypt):
    rnd = random.Random(40 + key_len + decrypt)
    for trial, iv_len in enumerate((12, 16, 60, 1)):
        key = rnd.randbytes(key_len)
        iv = (gic.craft_iv(oracle, key, iv_len, (1 << 32) - 3, trial) if iv_len >= 16
              else rnd.randbytes(iv_len))
        aad, data = rnd.randbytes(rnd.choice([0, 13, 77])), rnd.randbytes(16 * 70 + 9)
        want, want_tag = oracle.gcm(key, iv, aad, data, decrypt=decrypt)
        s = po.GcmStream(oracle, key)
        s.setiv(iv)
        p = 0
        while p < len(aad):
            k = rnd.randrange(1, 20)
            assert s.aad(aad[p:p + k]) == 0
            p += k
        got, p = b"", 0
        while p < len(data):
            k = rnd.choice([1, 5, 16, 33, 160, 1024 + 7])
            rc, out = (s.decrypt if decrypt else s.encrypt)(data[p:p + k])
            assert rc == 0
            got += out
            p += k
        assert got == want
        assert s.tag(16) == want_tag and s.tag(12) == want_tag[:12]
        assert s.tag(16) == want_tag                     # reading the tag leaves the state alone
        assert s.finish(want_tag) == 0 and s.finish(want_tag[:4]) == 0
        assert s.finish(bytes([want_tag[0] ^ 1]) + want_tag[1:]) == -1


def test_gcm_stream_return_codes_and_copy(oracle):
    key, iv = bytes(range(16)), bytes(range(12))
    s = po.GcmStream(oracle, key)
    s.setiv(iv)
    assert s.aad(b"header") == 0
    rc, c1 = s.encrypt(b"x" * 21)
    assert rc == 0
    # gcm128.c:838-839: AAD after data is refused with -2 and changes nothing
    assert s.aad(b"late") == -2
    fork = s.copy()
    rc, c2 = s.encrypt(b"y" * 30)
    assert rc == 0 and (c1 + c2, s.tag()) == oracle.gcm(key, iv, b"header", b"x" * 21 + b"y" * 30)
    rc, c3 = fork.encrypt(b"z" * 11)   # the copy went its own way from a partial block
    assert rc == 0 and (c1 + c3, fork.tag()) == oracle.gcm(key, iv, b"header", b"x" * 21 + b"z" * 11)
    s.setiv(iv)                        # setiv resets the stream
    assert s.aad(b"header") == 0
