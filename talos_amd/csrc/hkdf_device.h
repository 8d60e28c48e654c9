// hkdf_device.h — the part of the TLS 1.3 key schedule that follows a traffic
// secret (RFC 8446 7.1-7.3): SHA-256 and SHA-384 compression (FIPS 180-4), HMAC
// (RFC 2104) and HKDF-Expand-Label (RFC 5869 2.3 with RFC 8446 7.1's HkdfLabel)
// for an output of at most one hash length and an empty context.
//
// Written for the device (key_schedule.hip, one lane per session) and compiled
// unchanged for the host (tests/hkdf_host, any C++17 compiler).  Plain integer
// code: no table indexed by secret data and no branch on secret data; the only
// table is the round constants, indexed by the round number (__constant__ memory
// on the device, a static const array on the host).  The message schedule is a
// rolling window of 16 words at compile-time indices, so it stays in registers.
//
// An HkdfLabel here is at most 2 + 1 + 6 + 11 + 1 = 21 bytes, 22 with HKDF's
// counter byte, and a hash value at most 48: every HMAC message, inner and
// outer, is one block behind the key block.  HmacKey holds the two states a key
// leaves behind (after its ipad and its opad block); each label then costs two
// compressions.  A KeyUpdate is 2 + 2 ("traffic upd") for the old secret and
// 2 + 2 + 2 (key, iv) for the new one: 10 compressions.
//
// Byte strings are big-endian 32-bit words throughout (`be`): a 48-byte secret
// is 12 words, word 0 holding bytes 0..3.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define TG_HKDF_FN __host__ __device__ inline
#else
#define TG_HKDF_FN inline
#endif

namespace tg {
namespace hkdf {

#define TG_SHA256_K                                                                               \
  {0x428a2f98u, 0x71374491u, 0xb5c0fbcfu, 0xe9b5dba5u, 0x3956c25bu, 0x59f111f1u, 0x923f82a4u,     \
   0xab1c5ed5u, 0xd807aa98u, 0x12835b01u, 0x243185beu, 0x550c7dc3u, 0x72be5d74u, 0x80deb1feu,     \
   0x9bdc06a7u, 0xc19bf174u, 0xe49b69c1u, 0xefbe4786u, 0x0fc19dc6u, 0x240ca1ccu, 0x2de92c6fu,     \
   0x4a7484aau, 0x5cb0a9dcu, 0x76f988dau, 0x983e5152u, 0xa831c66du, 0xb00327c8u, 0xbf597fc7u,     \
   0xc6e00bf3u, 0xd5a79147u, 0x06ca6351u, 0x14292967u, 0x27b70a85u, 0x2e1b2138u, 0x4d2c6dfcu,     \
   0x53380d13u, 0x650a7354u, 0x766a0abbu, 0x81c2c92eu, 0x92722c85u, 0xa2bfe8a1u, 0xa81a664bu,     \
   0xc24b8b70u, 0xc76c51a3u, 0xd192e819u, 0xd6990624u, 0xf40e3585u, 0x106aa070u, 0x19a4c116u,     \
   0x1e376c08u, 0x2748774cu, 0x34b0bcb5u, 0x391c0cb3u, 0x4ed8aa4au, 0x5b9cca4fu, 0x682e6ff3u,     \
   0x748f82eeu, 0x78a5636fu, 0x84c87814u, 0x8cc70208u, 0x90befffau, 0xa4506cebu, 0xbef9a3f7u,     \
   0xc67178f2u}
#define TG_SHA512_K                                                                               \
  {0x428a2f98d728ae22ull, 0x7137449123ef65cdull, 0xb5c0fbcfec4d3b2full, 0xe9b5dba58189dbbcull,    \
   0x3956c25bf348b538ull, 0x59f111f1b605d019ull, 0x923f82a4af194f9bull, 0xab1c5ed5da6d8118ull,    \
   0xd807aa98a3030242ull, 0x12835b0145706fbeull, 0x243185be4ee4b28cull, 0x550c7dc3d5ffb4e2ull,    \
   0x72be5d74f27b896full, 0x80deb1fe3b1696b1ull, 0x9bdc06a725c71235ull, 0xc19bf174cf692694ull,    \
   0xe49b69c19ef14ad2ull, 0xefbe4786384f25e3ull, 0x0fc19dc68b8cd5b5ull, 0x240ca1cc77ac9c65ull,    \
   0x2de92c6f592b0275ull, 0x4a7484aa6ea6e483ull, 0x5cb0a9dcbd41fbd4ull, 0x76f988da831153b5ull,    \
   0x983e5152ee66dfabull, 0xa831c66d2db43210ull, 0xb00327c898fb213full, 0xbf597fc7beef0ee4ull,    \
   0xc6e00bf33da88fc2ull, 0xd5a79147930aa725ull, 0x06ca6351e003826full, 0x142929670a0e6e70ull,    \
   0x27b70a8546d22ffcull, 0x2e1b21385c26c926ull, 0x4d2c6dfc5ac42aedull, 0x53380d139d95b3dfull,    \
   0x650a73548baf63deull, 0x766a0abb3c77b2a8ull, 0x81c2c92e47edaee6ull, 0x92722c851482353bull,    \
   0xa2bfe8a14cf10364ull, 0xa81a664bbc423001ull, 0xc24b8b70d0f89791ull, 0xc76c51a30654be30ull,    \
   0xd192e819d6ef5218ull, 0xd69906245565a910ull, 0xf40e35855771202aull, 0x106aa07032bbd1b8ull,    \
   0x19a4c116b8d2d0c8ull, 0x1e376c085141ab53ull, 0x2748774cdf8eeb99ull, 0x34b0bcb5e19b48a8ull,    \
   0x391c0cb3c5c95a63ull, 0x4ed8aa4ae3418acbull, 0x5b9cca4f7763e373ull, 0x682e6ff3d6b2b8a3ull,    \
   0x748f82ee5defb2fcull, 0x78a5636f43172f60ull, 0x84c87814a1f0ab72ull, 0x8cc702081a6439ecull,    \
   0x90befffa23631e28ull, 0xa4506cebde82bde9ull, 0xbef9a3f7b2c67915ull, 0xc67178f2e372532bull,    \
   0xca273eceea26619cull, 0xd186b8c721c0c207ull, 0xeada7dd6cde0eb1eull, 0xf57d4f7fee6ed178ull,    \
   0x06f067aa72176fbaull, 0x0a637dc5a2c898a6ull, 0x113f9804bef90daeull, 0x1b710b35131c471bull,    \
   0x28db77f523047d84ull, 0x32caab7b40c72493ull, 0x3c9ebe0a15c9bebcull, 0x431d67c49c100d4cull,    \
   0x4cc5d4becb3e42b6ull, 0x597f299cfc657e2aull, 0x5fcb6fab3ad6faecull, 0x6c44198c4a475817ull}

static const uint32_t kSha256KHost[64] = TG_SHA256_K;
static const uint64_t kSha512KHost[80] = TG_SHA512_K;
#if defined(__HIPCC__)
static __constant__ const uint32_t kSha256KDev[64] = TG_SHA256_K;
static __constant__ const uint64_t kSha512KDev[80] = TG_SHA512_K;
#endif
#undef TG_SHA256_K
#undef TG_SHA512_K

// rotates by 1..63: the builtin where the compiler has it, shifts elsewhere
#if defined(__has_builtin)
#if __has_builtin(__builtin_rotateright32) && __has_builtin(__builtin_rotateright64)
#define TG_HKDF_ROTATE_BUILTIN 1
#endif
#endif
#if defined(TG_HKDF_ROTATE_BUILTIN)
TG_HKDF_FN uint32_t rotr(uint32_t x, int n) { return __builtin_rotateright32(x, (uint32_t)n); }
TG_HKDF_FN uint64_t rotr(uint64_t x, int n) { return __builtin_rotateright64(x, (uint64_t)n); }
#else
TG_HKDF_FN uint32_t rotr(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }
TG_HKDF_FN uint64_t rotr(uint64_t x, int n) { return (x >> n) | (x << (64 - n)); }
#endif

// The two hashes as traits of one compression function.  SHA-384 is SHA-512
// with its own initial value and the first six state words as the digest.
struct Sha256 {
  typedef uint32_t word;
  static constexpr int kRounds = 64, kBlock = 64, kDigest = 32;
  TG_HKDF_FN static word iv(int i) {
    constexpr word v[8] = {0x6a09e667u, 0xbb67ae85u, 0x3c6ef372u, 0xa54ff53au,
                           0x510e527fu, 0x9b05688cu, 0x1f83d9abu, 0x5be0cd19u};
    return v[i];
  }
  TG_HKDF_FN static word k(int i) {
#if defined(__HIP_DEVICE_COMPILE__)
    return kSha256KDev[i];
#else
    return kSha256KHost[i];
#endif
  }
  TG_HKDF_FN static word S0(word x) { return rotr(x, 2) ^ rotr(x, 13) ^ rotr(x, 22); }
  TG_HKDF_FN static word S1(word x) { return rotr(x, 6) ^ rotr(x, 11) ^ rotr(x, 25); }
  TG_HKDF_FN static word s0(word x) { return rotr(x, 7) ^ rotr(x, 18) ^ (x >> 3); }
  TG_HKDF_FN static word s1(word x) { return rotr(x, 17) ^ rotr(x, 19) ^ (x >> 10); }
};
struct Sha384 {
  typedef uint64_t word;
  static constexpr int kRounds = 80, kBlock = 128, kDigest = 48;
  TG_HKDF_FN static word iv(int i) {
    constexpr word v[8] = {0xcbbb9d5dc1059ed8ull, 0x629a292a367cd507ull, 0x9159015a3070dd17ull,
                           0x152fecd8f70e5939ull, 0x67332667ffc00b31ull, 0x8eb44a8768581511ull,
                           0xdb0c2e0d64f98fa7ull, 0x47b5481dbefa4fa4ull};
    return v[i];
  }
  TG_HKDF_FN static word k(int i) {
#if defined(__HIP_DEVICE_COMPILE__)
    return kSha512KDev[i];
#else
    return kSha512KHost[i];
#endif
  }
  TG_HKDF_FN static word S0(word x) { return rotr(x, 28) ^ rotr(x, 34) ^ rotr(x, 39); }
  TG_HKDF_FN static word S1(word x) { return rotr(x, 14) ^ rotr(x, 18) ^ rotr(x, 41); }
  TG_HKDF_FN static word s0(word x) { return rotr(x, 1) ^ rotr(x, 8) ^ (x >> 7); }
  TG_HKDF_FN static word s1(word x) { return rotr(x, 19) ^ rotr(x, 61) ^ (x >> 6); }
};

// One block into the state.  m: the block's 16 big-endian words.  Sixteen rounds
// are unrolled so that every index into the window is a constant; the loop
// around them is not, which keeps the code of the ten call sites of a KeyUpdate
// small (the round constant's index is the only thing it makes dynamic).
template <class H>
TG_HKDF_FN void compress(typename H::word st[8], const typename H::word m[16]) {
  typedef typename H::word word;
  word w[16];
#pragma unroll
  for (int i = 0; i < 16; i++) w[i] = m[i];
  word a = st[0], b = st[1], c = st[2], d = st[3], e = st[4], f = st[5], g = st[6], h = st[7];
#pragma unroll 1
  for (int t = 0; t < H::kRounds; t += 16) {
#pragma unroll
    for (int i = 0; i < 16; i++) {
      if (t != 0)
        w[i] += H::s1(w[(i + 14) & 15]) + w[(i + 9) & 15] + H::s0(w[(i + 1) & 15]);
      const word t1 = h + H::S1(e) + ((e & f) ^ (~e & g)) + H::k(t + i) + w[i];
      const word t2 = H::S0(a) + ((a & b) ^ (a & c) ^ (b & c));
      h = g; g = f; f = e; e = d + t1;
      d = c; c = b; b = a; a = t1 + t2;
    }
  }
  st[0] += a; st[1] += b; st[2] += c; st[3] += d;
  st[4] += e; st[5] += f; st[6] += g; st[7] += h;
}

// byte b at byte position pos of a block held as big-endian words (OR into zeros)
template <class W>
TG_HKDF_FN void put_byte(W m[16], int pos, uint8_t b) {
  constexpr int kW = (int)sizeof(W);
  m[pos / kW] |= (W)b << (8 * (kW - 1 - pos % kW));
}

// The end of a message whose last block holds `used` bytes so far, `total`
// bytes in all: 0x80, and the bit length in the block's last word (a message
// here is far below 2^32 bits, so the upper length word stays zero).
template <class H>
TG_HKDF_FN void put_padding(typename H::word m[16], int used, uint64_t total) {
  put_byte(m, used, 0x80);
  m[15] |= (typename H::word)(total * 8);
}

// digest word i of a state as big-endian 32-bit words out[0 .. kDigest / 4)
TG_HKDF_FN void digest_words(const uint32_t st[8], uint32_t* out, Sha256*) {
#pragma unroll
  for (int i = 0; i < 8; i++) out[i] = st[i];
}
TG_HKDF_FN void digest_words(const uint64_t st[8], uint32_t* out, Sha384*) {
#pragma unroll
  for (int i = 0; i < 6; i++) {
    out[2 * i] = (uint32_t)(st[i] >> 32);
    out[2 * i + 1] = (uint32_t)st[i];
  }
}
// word i of a block from big-endian 32-bit words
TG_HKDF_FN uint32_t block_word(const uint32_t* be, int i, Sha256*) { return be[i]; }
TG_HKDF_FN uint64_t block_word(const uint32_t* be, int i, Sha384*) {
  return ((uint64_t)be[2 * i] << 32) | be[2 * i + 1];
}

// What an HMAC key leaves behind: the states after its ipad and its opad block.
template <class H>
struct HmacKey {
  typename H::word inner[8], outer[8];
};

// key: key_words big-endian 32-bit words (at most one block; 8 or 12 here)
template <class H>
TG_HKDF_FN void hmac_key(HmacKey<H>& k, const uint32_t* key_be, int key_words) {
  typedef typename H::word word;
  constexpr int kPer = (int)sizeof(word) / 4;  // 32-bit words per block word
  const word ipad = (word)0x3636363636363636ull, opad = (word)0x5c5c5c5c5c5c5c5cull;
  word kb[16], m[16];
#pragma unroll
  for (int i = 0; i < 16; i++)
    kb[i] = i * kPer < key_words ? block_word(key_be, i, (H*)nullptr) : (word)0;
#pragma unroll
  for (int i = 0; i < 8; i++) k.inner[i] = k.outer[i] = H::iv(i);
#pragma unroll
  for (int i = 0; i < 16; i++) m[i] = kb[i] ^ ipad;
  compress<H>(k.inner, m);
#pragma unroll
  for (int i = 0; i < 16; i++) m[i] = kb[i] ^ opad;
  compress<H>(k.outer, m);
}

// HMAC of a message that is one block with its padding: m holds the message's
// msg_len bytes (msg_len <= kBlock - 1 - 8, the rest zero); m is consumed.
// out: kDigest / 4 big-endian words.
template <class H>
TG_HKDF_FN void hmac_block(const HmacKey<H>& k, typename H::word m[16], int msg_len,
                           uint32_t* out) {
  typedef typename H::word word;
  word st[8];
#pragma unroll
  for (int i = 0; i < 8; i++) st[i] = k.inner[i];
  put_padding<H>(m, msg_len, (uint64_t)H::kBlock + (uint64_t)msg_len);
  compress<H>(st, m);
  constexpr int kDw = H::kDigest / (int)sizeof(word);  // digest words: 8 (SHA-256), 6 (SHA-384)
#pragma unroll
  for (int i = 0; i < 16; i++) m[i] = i < kDw ? st[i] : (word)0;
  put_padding<H>(m, H::kDigest, (uint64_t)H::kBlock + H::kDigest);
#pragma unroll
  for (int i = 0; i < 8; i++) st[i] = k.outer[i];
  compress<H>(st, m);
  digest_words(st, out, (H*)nullptr);
}

// HKDF-Expand-Label(secret, label, "", out_len) for out_len <= Hash.length, the
// secret given as its HmacKey: T(1) = HMAC(secret, HkdfLabel || 0x01) with
// HkdfLabel = uint16 out_len || uint8 (6 + label_len) || "tls13 " || label ||
// uint8 0 (RFC 8446 7.1).  label_len <= 11.  out: kDigest / 4 big-endian words,
// of which the caller keeps the first out_len bytes.
template <class H>
TG_HKDF_FN void expand_label(const HmacKey<H>& k, const char* label, int label_len, int out_len,
                             uint32_t* out) {
  typename H::word m[16];
#pragma unroll
  for (int i = 0; i < 16; i++) m[i] = 0;
  const char prefix[7] = "tls13 ";
  put_byte(m, 0, (uint8_t)(out_len >> 8));
  put_byte(m, 1, (uint8_t)out_len);
  put_byte(m, 2, (uint8_t)(6 + label_len));
#pragma unroll
  for (int i = 0; i < 6; i++) put_byte(m, 3 + i, (uint8_t)prefix[i]);
#pragma unroll
  for (int i = 0; i < 11; i++)
    if (i < label_len) put_byte(m, 9 + i, (uint8_t)label[i]);
  // byte 9 + label_len: the empty context's length, 0; then HKDF's counter
  put_byte(m, 10 + label_len, 1);
  hmac_block<H>(k, m, 11 + label_len, out);
}

// ---------------------------------------------------------------------------
// Whole messages from bytes, for the tests (tests/hkdf_host): the compression
// function over every padding boundary, and HMAC from a key and a message.

template <class H>
TG_HKDF_FN void hash_bytes(const uint8_t* msg, size_t len, uint8_t* out) {
  typedef typename H::word word;
  word st[8], m[16];
  for (int i = 0; i < 8; i++) st[i] = H::iv(i);
  size_t pos = 0;
  bool closed = false, done = false;  // the 0x80 is written; the length is written
  while (!done) {
    for (int i = 0; i < 16; i++) m[i] = 0;
    int used = 0;
    for (; used < H::kBlock && pos < len; used++, pos++) put_byte(m, used, msg[pos]);
    if (used < H::kBlock && !closed) {
      put_byte(m, used, 0x80);
      used++;
      closed = true;
    }
    if (closed && used <= H::kBlock - 2 * (int)sizeof(word)) {
      m[15] |= (word)((uint64_t)len * 8);
      done = true;
    }
    compress<H>(st, m);
  }
  uint32_t be[12];
  digest_words(st, be, (H*)nullptr);
  for (int i = 0; i < H::kDigest; i++) out[i] = (uint8_t)(be[i / 4] >> (24 - 8 * (i % 4)));
}

// key_len a multiple of 4 and at most one block; msg_len <= kBlock - 9
template <class H>
TG_HKDF_FN void hmac_bytes(const uint8_t* key, int key_len, const uint8_t* msg, int msg_len,
                           uint8_t* out) {
  uint32_t key_be[32], be[12];
  for (int i = 0; i < key_len / 4; i++)
    key_be[i] = ((uint32_t)key[4 * i] << 24) | ((uint32_t)key[4 * i + 1] << 16) |
                ((uint32_t)key[4 * i + 2] << 8) | key[4 * i + 3];
  HmacKey<H> k;
  hmac_key<H>(k, key_be, key_len / 4);
  typename H::word m[16];
  for (int i = 0; i < 16; i++) m[i] = 0;
  for (int i = 0; i < msg_len; i++) put_byte(m, i, msg[i]);
  hmac_block<H>(k, m, msg_len, be);
  for (int i = 0; i < H::kDigest; i++) out[i] = (uint8_t)(be[i / 4] >> (24 - 8 * (i % 4)));
}

}  // namespace hkdf
}  // namespace tg
