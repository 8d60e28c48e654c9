"""GCM IVs with a chosen start counter, and the case list of the counter tests.

With an IV that is not 12 bytes, J0 = GHASH_H(IV || pad || 0^64 || [len(IV)]_64)
(gcm128.c:770-812), so the 32-bit block counter starts anywhere.  GHASH is
linear in each block: with m = ceil(iv_len / 16) IV blocks B1..Bm and the
length block L,

    J0 = B1*H^(m+1) ^ B2*H^m ^ ... ^ Bm*H^2 ^ L*H,

so for any target T the first block is B1 = (T ^ GHASH(B2..Bm, L)) * H^-(m+1).
craft_iv() picks T with chosen low 32 bits and solves for B1; the counter of
block i of the message is then (j0_ctr + 1 + i) mod 2^32 (inc32: no carry into
byte 11).  The wrap index w of a case is the 0-based block whose counter is 0:
j0_ctr = 2^32 - 1 - w, and w = 0 means inc32(J0) itself wraps.

Pure Python ints; nothing here is a hot path.
"""
from __future__ import annotations

import random

import numpy as np

_R = 0xE1 << 120
ONE = 1 << 127   # x^0 is the most significant bit of byte 0 (GCM bit order)


def gf_mul(x: int, y: int) -> int:
    """Product in GF(2^128), operands and result as big-endian ints of the blocks."""
    z, v = 0, y
    for i in range(127, -1, -1):
        if (x >> i) & 1:
            z ^= v
        v = (v >> 1) ^ (_R if v & 1 else 0)
    return z


def gf_pow(x: int, e: int) -> int:
    r = ONE
    while e:
        if e & 1:
            r = gf_mul(r, x)
        x = gf_mul(x, x)
        e >>= 1
    return r


def gf_inv(x: int) -> int:
    assert x
    return gf_pow(x, (1 << 128) - 2)


def ghash(h: int, data: bytes, y: int = 0) -> int:
    """Y <- (Y ^ B) * H over the zero-padded 16-byte blocks of data."""
    for off in range(0, len(data), 16):
        b = data[off:off + 16]
        y = gf_mul(y ^ int.from_bytes(b + bytes(16 - len(b)), "big"), h)
    return y


def hash_key(oracle, key: bytes) -> int:
    return int.from_bytes(oracle.aes_encrypt(key, bytes(16)), "big")


def j0_of(oracle, key: bytes, iv: bytes) -> bytes:
    """J0 of any IV (gcm128.c:749-824)."""
    if len(iv) == 12:
        return iv + b"\0\0\0\1"
    h = hash_key(oracle, key)
    y = ghash(h, iv)
    return ghash(h, bytes(8) + (8 * len(iv)).to_bytes(8, "big"), y).to_bytes(16, "big")


def craft_iv(oracle, key: bytes, iv_len: int, j0_ctr: int, rest_seed: int) -> bytes:
    """An IV of iv_len >= 16 bytes whose J0 has low 32 bits j0_ctr.  The bytes
    after the first block and the upper 96 bits of J0 are random (rest_seed)."""
    assert iv_len >= 16 and 0 <= j0_ctr < 1 << 32
    rnd = random.Random(rest_seed)
    rest = bytes(rnd.randrange(256) for _ in range(iv_len - 16))
    target = (rnd.getrandbits(96) << 32) | j0_ctr
    h = hash_key(oracle, key)
    m = (iv_len + 15) // 16
    tail = ghash(h, bytes(8) + (8 * iv_len).to_bytes(8, "big"), ghash(h, rest))
    b1 = gf_mul(target ^ tail, gf_inv(gf_pow(h, m + 1)))
    return b1.to_bytes(16, "big") + rest


def ctr_model_encrypt(oracle, key: bytes, iv: bytes, pt: bytes) -> bytes:
    """pt ^ E_K(J0[0:12] || be32((ctr(J0) + 1 + i) mod 2^32)), block by block."""
    j0 = j0_of(oracle, key, iv)
    ctr = int.from_bytes(j0[12:], "big")
    out = bytearray()
    for i in range((len(pt) + 15) // 16):
        ks = oracle.aes_encrypt(key, j0[:12] + ((ctr + 1 + i) & 0xFFFFFFFF).to_bytes(4, "big"))
        out += bytes(a ^ b for a, b in zip(pt[16 * i:16 * i + 16], ks))
    return bytes(out)


def fill(seed: int, index: int, n: int) -> bytes:
    """talos_amd.workload.fill_bytes (the SplitMix64 stream of oracle_fill_bytes), in numpy."""
    m64 = (1 << 64) - 1
    st = np.uint64((seed ^ (index * 0xD1B54A32D192ED03)) & m64)
    with np.errstate(over="ignore"):
        z = st + np.arange(1, (n + 7) // 8 + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z ^= z >> np.uint64(31)
    return z.astype("<u8").tobytes()[:n]


# ---- the EVP_AEAD counter cases (tests/test_gpu_evp_gcm_counters.py) ----------

IV_LENS, TAG_LENS, AAD_LENS = (16, 33, 60, 64), (16, 12), (0, 13, 100)
# (plaintext bytes, wrap indices w): the 32-bit counter is 0 at block w
WRAP_TABLE = [
    (0, (0,)),                                             # tag only: E_K(J0), counter 0xFFFFFFFF
    (1, (0, 1)), (15, (0, 1)), (16, (0, 1)), (17, (0, 1)),
    (100, (0, 1, 6)),                                      # wrap on the partial last block
    (16 * 1024, (0, 1, 63, 64, 65, 511, 1023)),            # one 64-block step per wave
    (16 * 1024 + 5, (64, 127, 128, 1024)),                 # spw = 2; block 1024 is the partial tail
    (16 * 2112 + 9, (81, 145, 209)),                       # spw = 3: ctr0+i / ctr0+i+64 astride the wrap
]
# controls without a 32-bit wrap: the counter crosses 2^16 and 2^24 inside the job
CONTROL_TABLE = [(16 * 1024, 0x0000FFF0), (16 * 1024, 0x00FFFFC0)]
KEY_LENS = (16, 32)


def wrap_cases():
    """[{n, j0_ctr, w (None for a control), iv_len, tag_len, aad_len, id}]: IV
    lengths, tag lengths and AAD lengths in turn, each combination of the three
    reached; every case is run for both key sizes."""
    plain = [(n, (1 << 32) - 1 - w, w) for n, ws in WRAP_TABLE for w in ws]
    plain += [(n, c, None) for n, c in CONTROL_TABLE]
    cases = []
    for i, (n, j0_ctr, w) in enumerate(plain):
        cases.append({"n": n, "j0_ctr": j0_ctr, "w": w, "iv_len": IV_LENS[i % 4],
                      "tag_len": TAG_LENS[(i // 4) % 2], "aad_len": AAD_LENS[i % 3],
                      "id": f"n{n}-" + (f"w{w}" if w is not None else f"ctr{j0_ctr:08x}")})
    return cases


# ---- the stream-kernel wrap cases (tests/test_gpu_gcm_stream.py) -------------
STREAM_IV_LENS = (16, 60)
# name: (wrap index w, pieces in bytes): where block w falls in the calls
STREAM_WRAPS = {
    "first": (0, (16 * 3 + 7, 16 * 4 + 9)),               # inc32(J0) itself wraps
    "lane": (70, (16 * 200, 40)),                          # inside a 200-block piece, lane 6's second block
    "boundary": (64, (16 * 64, 16 * 65)),                  # the first block of the second call
    "tail": (129, (16 * 129 + 7, 9 + 16 * 3)),             # its keystream carried in EKi across two calls
}
STREAM_COPY_W = 33   # reached after a ctrl(COPY) taken 7 bytes into block 30


def case_seed(index: int, key_len: int) -> int:
    return 0xC7120000 + 2 * index + (key_len == 32)


def case_inputs(oracle, case: dict, key_len: int, index: int):
    """(key, iv, aad, pt) of case number `index` for a key size: seeded, so the
    CPU model tests, the golden file and the GPU children build the same bytes."""
    seed = case_seed(index, key_len)
    key = fill(seed, 1, key_len)
    iv = craft_iv(oracle, key, case["iv_len"], case["j0_ctr"], seed)
    return key, iv, fill(seed, 2, case["aad_len"]), fill(seed, 3, case["n"])
