"""The device key schedule's hash code on the host: talos_amd/csrc/hkdf_device.h
(SHA-256 / SHA-384 compression, HMAC from the two states a key leaves behind,
HKDF-Expand-Label) compiled into tests/hkdf_host with its own main, every line
it prints compared with hashlib / hmac and tls13_helper.hkdf_expand_label.  The
same program runs once under the address and undefined-behaviour sanitizers.
No GPU: the kernels of key_schedule.hip run this very code, one lane each
(tests/test_gpu_key_update.py checks them on the device)."""
import hashlib
import hmac
import os
import shutil
import subprocess

import pytest

import tls13_helper as t13

HERE = os.path.dirname(os.path.abspath(__file__))
DIR = os.path.join(HERE, "hkdf_host")
LENS = (0, 1, 55, 56, 63, 64, 111, 112, 127, 128, 200)     # both block sizes' padding boundaries
MSG = bytes((7 * i + 1) & 0xFF for i in range(200))
KEY = bytes((0xA0 + 3 * i) & 0xFF for i in range(48))
DIGEST = {"sha256": 32, "sha384": 48}
ONE_BLOCK = {"sha256": 64 - 1 - 8, "sha384": 128 - 1 - 16}  # longest message in the key's block
LABELS = (("key", 16), ("key", 32), ("iv", 12), ("traffic upd", 32), ("traffic upd", 48))


def expected():
    out = []
    for h in ("sha256", "sha384"):
        for n in LENS:
            out.append(f"hash {h} {n} {hashlib.new(h, MSG[:n]).hexdigest()}")
        for klen in (32, 48):
            for n in (0, 1, 22, ONE_BLOCK[h]):
                out.append(f"hmac {h} {klen} {n} {hmac.new(KEY[:klen], MSG[:n], h).hexdigest()}")
        for label, n in LABELS:
            if n <= DIGEST[h]:
                v = t13.hkdf_expand_label(KEY[:DIGEST[h]], label, n, h)
                out.append(f"label {h} {label.replace(' ', '_')} {n} {v.hex()}")
    return out


@pytest.fixture(scope="module")
def programs():
    if not shutil.which(os.environ.get("CXX", "g++")):
        pytest.skip("no host C++ compiler")
    r = subprocess.run(["make", "-C", DIR, "-s"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return os.path.join(DIR, "_build", "hkdf_host"), os.path.join(DIR, "_build", "hkdf_host_san")


def run(path):
    r = subprocess.run([path], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout.splitlines()


def test_every_line_matches_hashlib(programs):
    got, want = run(programs[0]), expected()
    assert len(want) == 2 * len(LENS) + 2 * 8 + 4 + 5   # SHA-256 has no 48-byte "traffic upd"
    for g, w in zip(got, want):
        assert g == w
    assert len(got) == len(want)


def test_the_reference_is_the_rfc():
    """hashlib is the reference; one published value keeps the test's own inputs
    honest: RFC 8448 section 3's server application traffic secret 0 and its
    write key and IV (SHA-256, TLS_AES_128_GCM_SHA256)."""
    secret = bytes.fromhex("a11af9f05531f856ad47116b45a950328204b4f44bfb6b3a4b4f1f3fcb631643")
    assert t13.hkdf_expand_label(secret, "key", 16, "sha256").hex() == \
        "9f02283b6c9c07efc26bb9f2ac92e356"
    assert t13.hkdf_expand_label(secret, "iv", 12, "sha256").hex() == "cf782b88dd83549aadf1e984"


def test_clean_under_address_and_undefined_sanitizers(programs):
    """Host code with its own main: the sanitizers' runtime is linked in, nothing
    is preloaded.  Any report aborts the program (-fno-sanitize-recover)."""
    assert run(programs[1]) == expected()
