"""The round-2 cache of the queue kernel's open no-pack variants, as a CPU model.

For a counter block nonce(12) || ctr(4, big endian) with ctr < 2^16 only bytes
14 (ctr >> 8) and 15 (ctr & 0xFF) change.  ShiftRows of round 1 moves byte 15
into column 0 and byte 14 into column 1, so after round 1 column 0 depends on
the low byte alone, column 1 on the high byte alone and columns 2 and 3 on
neither.  SubBytes works byte by byte and ShiftRows, MixColumns and
AddRoundKey are linear, so the state after round 2 separates exactly:

    state2(ctr) = F(ctr & 0xFF) ^ G(ctr >> 8) ^ K2

F the image of round 1's column 0, G that of column 1, K2 that of columns 2 and
3 plus the round key.  The kernel (gcm_device.h, gcm_blocks_xN with R2C) keeps
F and G per lane, and this is the map it must follow:

  * block i of a record has counter 2 + i and runs in lane i % 64 at step i // 64;
  * F variant of step s: s & 3, built once per record from counter 2 + lane + 64 v
    (the low byte of 2 + lane + 64 s depends on s & 3 only);
  * high byte: s >> 2 in lanes 0..61, (s + 1) >> 2 in lanes 62 and 63, which
    carry one step early, at steps 3, 7, 11, 15 — it is not wave-uniform;
  * G is looked up at steps s % 4 == 0, for the high byte of step s + 3; lanes
    60..63 use the words of the lane two below at steps s, s + 1, s + 2 and
    their own at step s + 3.

The model below follows that map literally (a dictionary per lane, filled when
the kernel fills its registers) and every keystream block is compared with the
oracle's AES.
"""
import numpy as np
import pytest

SBOX = [0] * 256


def _init_sbox():
    p = q = 1
    while True:
        p = p ^ ((p << 1) & 0xFF) ^ (0x1B if p & 0x80 else 0)      # p *= 3
        q ^= q << 1
        q ^= q << 2
        q ^= q << 4
        q &= 0xFF
        if q & 0x80:
            q ^= 0x09                                                # q /= 3
        x = q ^ (q << 1 | q >> 7) ^ (q << 2 | q >> 6) ^ (q << 3 | q >> 5) ^ (q << 4 | q >> 4)
        SBOX[p] = (x ^ 0x63) & 0xFF
        if p == 1:
            break
    SBOX[0] = 0x63


_init_sbox()


def _xt(a):
    return ((a << 1) ^ (0x1B if a & 0x80 else 0)) & 0xFF


def expand_key(key):
    nk = len(key) // 4
    rounds = nk + 6
    w = [list(key[4 * i:4 * i + 4]) for i in range(nk)]
    rcon = 1
    for i in range(nk, 4 * (rounds + 1)):
        t = list(w[i - 1])
        if i % nk == 0:
            t = [SBOX[t[1]] ^ rcon, SBOX[t[2]], SBOX[t[3]], SBOX[t[0]]]
            rcon = _xt(rcon)
        elif nk > 6 and i % nk == 4:
            t = [SBOX[b] for b in t]
        w.append([a ^ b for a, b in zip(w[i - nk], t)])
    return [sum(w[4 * r:4 * r + 4], []) for r in range(rounds + 1)], rounds


def shift_mix(s):
    """ShiftRows then MixColumns of a column-major 16-byte state (both linear)."""
    sr = [s[4 * ((c + r) & 3) + r] for c in range(4) for r in range(4)]
    out = []
    for c in range(4):
        a = sr[4 * c:4 * c + 4]
        for r in range(4):
            out.append(_xt(a[r]) ^ _xt(a[(r + 1) & 3]) ^ a[(r + 1) & 3] ^ a[(r + 2) & 3] ^ a[(r + 3) & 3])
    return out


def xor(a, b):
    return [x ^ y for x, y in zip(a, b)]


def full_round(s, rk):
    return xor(shift_mix([SBOX[b] for b in s]), rk)


def last_round(s, rk):
    sb = [SBOX[b] for b in s]
    return xor([sb[4 * ((c + r) & 3) + r] for c in range(4) for r in range(4)], rk)


class Round2Model:
    """F, G and K2 of one record (key schedule, nonce), as the kernel splits them."""

    def __init__(self, key, nonce):
        self.rks, self.rounds = expand_key(key)
        self.nonce = list(nonce)
        self.k2 = xor(self._image(self._state1(0), (2, 3)), self.rks[2])

    def _state1(self, ctr):
        block = self.nonce + list(ctr.to_bytes(4, "big"))
        return full_round(xor(block, self.rks[0]), self.rks[1])

    @staticmethod
    def _image(s1, cols):
        """Round 2 without its key, of the named columns of the round-1 state alone."""
        part = [SBOX[s1[i]] if i // 4 in cols else 0 for i in range(16)]
        return shift_mix(part)

    def f(self, low):           # column 0 of round 1 sees the low byte only
        return self._image(self._state1(low), (0,))

    def g(self, high):          # column 1 the high byte only
        return self._image(self._state1(high << 8), (1,))

    def finish(self, state2):
        s = state2
        for r in range(3, self.rounds):
            s = full_round(s, self.rks[r])
        return bytes(last_round(s, self.rks[self.rounds]))


def kernel_keystream(model, nblocks):
    """Keystream blocks 0..nblocks-1 of a record by the kernel's lane / step map."""
    ctr0 = 2
    steps = (nblocks + 63) // 64
    F = [[model.f((ctr0 + lane + 64 * v) & 0xFF) for v in range(4)] for lane in range(64)]
    for lane in range(64):      # K2 is folded into F
        F[lane] = [xor(f, model.k2) for f in F[lane]]
    out = [None] * nblocks
    G = [None] * 64
    for s in range(steps):
        if s % 4 == 0:          # one lookup per four steps, for the high byte of step s + 3
            G = [model.g((ctr0 + lane + 64 * (s + 3)) >> 8) for lane in range(64)]
        for lane in range(64):
            i = 64 * s + lane
            if i >= nblocks:
                continue
            before_carry = G[lane - 2] if lane >= 60 else G[lane]
            g = G[lane] if s % 4 == 3 else before_carry
            out[i] = model.finish(xor(F[lane][s & 3], g))
    return out


def test_lane_step_map():
    """The counter bytes behind the map: four low bytes per lane, the high byte
    s >> 2 except in lanes 62 and 63, which carry at steps 3, 7, 11 and 15."""
    for lane in range(64):
        for s in range(17):
            ctr = 2 + lane + 64 * s
            assert ctr & 0xFF == (2 + lane + 64 * (s & 3)) & 0xFF
            assert ctr >> 8 == ((s + 1) >> 2 if lane >= 62 else s >> 2)
    for s in (3, 7, 11, 15):
        for lane in (62, 63):
            assert (2 + lane + 64 * s) >> 8 == ((2 + 61 + 64 * s) >> 8) + 1 == (s >> 2) + 1
            assert (2 + lane + 64 * (s - 1)) >> 8 == s >> 2
    # lanes 58..61 never carry early: what lanes 60..63 borrow is the window's own high byte
    for lane in range(58, 62):
        for s in range(17):
            assert (2 + lane + 64 * s) >> 8 == s >> 2


@pytest.mark.parametrize("klen", [16, 32])
def test_separation_identity(oracle, klen):
    """state2 = F(low) ^ G(high) ^ K2 finished with rounds 3.. equals AES for
    arbitrary (low, high), not only the pairs a record visits."""
    rng = np.random.default_rng(40 + klen)
    key, nonce = rng.bytes(klen), rng.bytes(12)
    m = Round2Model(key, nonce)
    for _ in range(64):
        low, high = int(rng.integers(256)), int(rng.integers(256))
        got = m.finish(xor(xor(m.f(low), m.g(high)), m.k2))
        assert got == oracle.aes_encrypt(key, nonce + bytes([0, 0, high, low]))


@pytest.mark.parametrize("klen", [16, 32])
def test_kernel_map_against_oracle(oracle, klen):
    """Counters 2..1043 (a 16,640-byte TLS 1.3 record and its type byte's
    block), several nonces, every block against the oracle's AES; lanes 62 and
    63 at steps 3, 7, 11 and 15 are among them."""
    rng = np.random.default_rng(50 + klen)
    key = rng.bytes(klen)
    nblocks = 1042
    for nonce in (rng.bytes(12), bytes(12), b"\xff" * 12):
        ks = kernel_keystream(Round2Model(key, nonce), nblocks)
        for i in range(nblocks):
            exp = oracle.aes_encrypt(key, nonce + (2 + i).to_bytes(4, "big"))
            assert ks[i] == exp, (klen, nonce.hex(), "block", i, "lane", i % 64, "step", i // 64)
        for s in (3, 7, 11, 15):
            for lane in (62, 63):
                assert ks[64 * s + lane] is not None
