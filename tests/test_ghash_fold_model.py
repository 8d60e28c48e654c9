"""The queue kernel's one-reduction GHASH multiply, as a CPU model.

gcm128.c's 4-bit method computes X * H as a Horner chain over X's 32 nibbles,
z = s(z) ^ T[nib_k], with s(Z) = (Z >> 4) ^ rem(Z & 0xF) the multiplication by
x^4 modulo the GCM polynomial.  s is linear, so the kernel's record finish
(gcm_device.h: mul_shoup_fold, gh_fold) adds the 32 table entries up unreduced,
each at its own bit offset in a 256-bit value W, and reduces once:

  * group j = 7..0 takes the nibble at bit 4 j of each of X's four BE words;
    the entry of word c sits c words down, so the four entries XOR into a
    seven-word sum by word placement;
  * the sum moves down 4 (7 - j) bits across the words and is XORed into W;
  * O = W[4..7] holds x^128 and above (bit 127 - i: x^(128 + i)), and
    x^128 = 1 + x + x^2 + x^7 gives Z = W[0..3] ^ O ^ O>>1 ^ O>>2 ^ O>>7;
  * O >> 7 drops bits 6..4 of O (x^128 .. x^130 again): folded once more.

load_len_table builds the lengths-block table the same way: one entry moved
down 4 (31 - k) bits, one fold.

The model follows that order literally on 32-bit words and is checked against
the 32-step chain (with s() derived from the polynomial, not from the kernel's
rem4), against the oracle's gf128_mul for X * H^e, e = 1..65, and the table
rows as len_term reads them against gf128_mul(LEN, H).
"""
import random

import pytest

M32 = 0xFFFFFFFF
M128 = (1 << 128) - 1
POLY = 0xE1 << 120       # 1 + x + x^2 + x^7, x^0 at bit 127
K_LEN_ROWS = 6
K_POW_MAX = 65


# ---- references -----------------------------------------------------------
def s_ref(z):
    """z * x^4: bit i < 4 of z is x^(127 - i) and becomes x^(128 + 3 - i)."""
    out = z >> 4
    for i in range(4):
        if (z >> i) & 1:
            out ^= POLY >> (3 - i)
    return out


def chain(x, tab):
    """gcm128.c's 4-bit method: nibble k = 0 is the low nibble of byte 15."""
    z = tab[x & 0xF]
    for k in range(1, 32):
        z = s_ref(z) ^ tab[(x >> (4 * k)) & 0xF]
    return z


def shoup_table(oracle, h):
    """T[v] = v * H, v's high bit x^0 (the Htable of gcm_init_4bit)."""
    return [int.from_bytes(oracle.gf128_mul(bytes([v << 4]) + bytes(15), h), "big")
            for v in range(16)]


# ---- the kernel's evaluation order ------------------------------------------
def words(z):
    return [(z >> (96 - 32 * i)) & M32 for i in range(4)]


def alignbit(hi, lo, sh):
    return (((hi << 32) | lo) >> (sh & 31)) & M32


def gh_fold(w):
    o = w[4:]
    t = (o[3] << 25) & M32
    z = [w[0] ^ o[0] ^ (o[0] >> 1) ^ (o[0] >> 2) ^ (o[0] >> 7) ^ t ^ (t >> 1) ^ (t >> 2) ^ (t >> 7)]
    for i in range(1, 4):
        z.append(w[i] ^ o[i] ^ alignbit(o[i - 1], o[i], 1) ^ alignbit(o[i - 1], o[i], 2) ^
                 alignbit(o[i - 1], o[i], 7))
    return z, t


def mul_shoup_fold(x, tab):
    xw = words(x)
    w = [0] * 8
    for j in range(7, -1, -1):
        t = [words(tab[(xw[c] >> (4 * j)) & 0xF]) for c in range(4)]
        s = [t[0][0],
             t[0][1] ^ t[1][0],
             t[0][2] ^ t[1][1] ^ t[2][0],
             t[0][3] ^ t[1][2] ^ t[2][1] ^ t[3][0],
             t[1][3] ^ t[2][2] ^ t[3][1],
             t[2][3] ^ t[3][2],
             t[3][3]]
        if j == 7:
            w[:7] = s
        else:
            sh = 4 * (7 - j)
            w[0] ^= s[0] >> sh
            for i in range(1, 7):
                w[i] ^= alignbit(s[i - 1], s[i], sh)
            w[7] ^= (s[6] << (32 - sh)) & M32
    z, t = gh_fold(w)
    return sum(v << (96 - 32 * i) for i, v in enumerate(z)), t


def flat_sum(x, tab):
    """The same product from the definition: W as one integer, one reduction."""
    w = 0
    for k in range(32):
        w ^= (tab[(x >> (4 * k)) & 0xF] << 128) >> (4 * (31 - k))
    hi, o = w >> 128, w & M128
    z = hi ^ o ^ (o >> 1) ^ (o >> 2) ^ (o >> 7)
    d = (o << 121) & M128
    return z ^ d ^ (d >> 1) ^ (d >> 2) ^ (d >> 7)


def len_table(tab, ab):
    """load_len_table: entry 16 p + v (BE words as one integer)."""
    out = []
    for i in range(128):
        p = i >> 4
        aad = p == K_LEN_ROWS
        z = words(tab[ab >> 4 if aad else i & 15])
        r = 24 if aad else 28 - 4 * p
        v = [z[0] >> r, alignbit(z[0], z[1], r), alignbit(z[1], z[2], r), alignbit(z[2], z[3], r),
             alignbit(z[3], 0, r)]
        if aad:
            u = words(tab[ab & 15])
            v = [v[0] ^ (u[0] >> 28), v[1] ^ alignbit(u[0], u[1], 28), v[2] ^ alignbit(u[1], u[2], 28),
                 v[3] ^ alignbit(u[2], u[3], 28), v[4] ^ ((u[3] << 4) & M32)]
        w = [0] + v + [0, 0] if aad else [0, 0, 0] + v
        f, _ = gh_fold(w)
        out.append(0 if p > K_LEN_ROWS else sum(x << (96 - 32 * k) for k, x in enumerate(f)))
    return out


def len_term_sum(table, n):
    """The wave sum of len_term: lane p < 6 nibble p of the bit count, lane 6
    the AAD entry, lanes 7.. a zero entry of row 7."""
    acc = 0
    for lane in range(64):
        row = min(lane, 7)
        acc ^= table[(row << 4) + (((n * 8) >> (4 * row)) & 0xF)]
    return acc


# ---- inputs -----------------------------------------------------------------
def _inputs():
    rnd = random.Random(0x6F1D)
    xs = [0, M128] + [rnd.getrandbits(128) for _ in range(24)]
    xs += [v << (4 * k) for k in range(32) for v in range(1, 16)]
    return xs


XS = _inputs()


def test_fold_equals_chain_random_tables():
    """Arbitrary tables: the identity needs s() linear and nothing of T."""
    rnd = random.Random(1)
    for it in range(40):
        tab = [rnd.getrandbits(128) for _ in range(16)]
        for x in (XS if it < 3 else XS[:26] + rnd.sample(XS[26:], 40)):
            ref = chain(x, tab)
            assert mul_shoup_fold(x, tab)[0] == ref
            assert flat_sum(x, tab) == ref
    ones = [M128] * 16
    for x in XS:
        assert mul_shoup_fold(x, ones)[0] == chain(x, ones)


def test_second_fold_all_three_bits():
    """An X whose unreduced sum has bits 6..4 of its low word all set: the
    second fold's three bits.  With T[v] = 0 but T[1], X = 1 << 4 k puts T[1]
    down 4 (31 - k) bits; k = 0 moves T[1]'s bits 2..0 to bits 6..4 of O."""
    tab = [0] * 16
    tab[1] = 0x7 | (0xDEADBEEF << 64)
    z, t = mul_shoup_fold(1, tab)
    assert t >> 29 == 7
    assert z == chain(1, tab) == flat_sum(1, tab)
    rnd = random.Random(2)
    hits = 0
    for _ in range(400):
        tab = [rnd.getrandbits(128) for _ in range(16)]
        x = rnd.getrandbits(128)
        z, t = mul_shoup_fold(x, tab)
        hits += t >> 29 == 7
        assert z == chain(x, tab)
    assert hits > 10   # about one in eight


def test_against_oracle_powers(oracle):
    """X * H^e, e = 1..65, with the Shoup tables the session install writes."""
    rnd = random.Random(3)
    h = bytes(rnd.randrange(256) for _ in range(16))
    he = h
    sample = XS[:26] + [v << (4 * k) for k in range(32) for v in (1, 8, 15)]
    for e in range(1, K_POW_MAX + 1):
        tab = shoup_table(oracle, he)
        for x in (XS if e in (1, 2, 64, 65) else sample):
            exp = int.from_bytes(oracle.gf128_mul(x.to_bytes(16, "big"), he), "big")
            assert mul_shoup_fold(x, tab)[0] == exp, (e, hex(x))
        he = oracle.gf128_mul(he, h)


@pytest.mark.parametrize("ab", [13 * 8, 5 * 8])
def test_len_table_rows(oracle, ab):
    rnd = random.Random(4 + ab)
    for _ in range(4):
        h = bytes(rnd.randrange(256) for _ in range(16))
        tab = shoup_table(oracle, h)
        table = len_table(tab, ab)

        def mul_h(block):
            return int.from_bytes(oracle.gf128_mul(block.to_bytes(16, "big"), h), "big")
        for p in range(K_LEN_ROWS):
            for v in range(16):
                assert table[16 * p + v] == mul_h(v << (4 * p)), (p, v)
                assert table[16 * p + v] == chain(v << (4 * p), tab)
        for v in range(16):
            assert table[16 * K_LEN_ROWS + v] == mul_h(ab << 64)
            assert table[16 * 7 + v] == 0
        for n in (0, 1, 2, 30, 510, 8190, 16384, 16384 + 255, (1 << 21) - 1):
            assert len_term_sum(table, n) == mul_h((ab << 64) | (8 * n)), n
