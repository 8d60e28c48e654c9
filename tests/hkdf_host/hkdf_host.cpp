// hkdf_host.cpp — TEST HARNESS: talos_amd/csrc/hkdf_device.h compiled for the
// host, its results printed one per line for tests/test_hkdf_host.py to compare
// with hashlib / hmac.  The inputs are fixed patterns both sides compute:
//   message byte i = (7 i + 1) mod 256, key / secret byte i = (0xA0 + 3 i) mod 256.
// Lines:
//   hash <sha256|sha384> <message bytes> <digest>
//   hmac <sha256|sha384> <key bytes> <message bytes> <mac>
//   label <sha256|sha384> <label, '_' for ' '> <output bytes> <output>
#include <cstdio>
#include <cstring>

#include "../../talos_amd/csrc/hkdf_device.h"

using namespace tg::hkdf;

static void hex(const uint8_t* p, int n) {
  for (int i = 0; i < n; i++) printf("%02x", p[i]);
  printf("\n");
}

template <class H>
static void run(const char* name) {
  static const int kLens[] = {0, 1, 55, 56, 63, 64, 111, 112, 127, 128, 200};
  uint8_t msg[200], key[48], out[48];
  for (int i = 0; i < 200; i++) msg[i] = (uint8_t)(7 * i + 1);
  for (int i = 0; i < 48; i++) key[i] = (uint8_t)(0xA0 + 3 * i);
  for (int len : kLens) {
    hash_bytes<H>(msg, (size_t)len, out);
    printf("hash %s %d ", name, len);
    hex(out, H::kDigest);
  }
  // one-block messages: empty, one byte, an HkdfLabel's length, the longest that fits
  const int mlens[] = {0, 1, 22, H::kBlock - 1 - 2 * (int)sizeof(typename H::word)};
  const int klens[] = {32, 48};
  for (int klen : klens)
    for (int mlen : mlens) {
      hmac_bytes<H>(key, klen, msg, mlen, out);
      printf("hmac %s %d %d ", name, klen, mlen);
      hex(out, H::kDigest);
    }
  // the secret is Hash.length bytes of the key pattern, as a traffic secret is
  uint32_t sec[12], be[12];
  for (int i = 0; i < H::kDigest / 4; i++)
    sec[i] = ((uint32_t)key[4 * i] << 24) | ((uint32_t)key[4 * i + 1] << 16) |
             ((uint32_t)key[4 * i + 2] << 8) | key[4 * i + 3];
  HmacKey<H> k;
  hmac_key<H>(k, sec, H::kDigest / 4);
  struct { const char* label; int len; } cases[] = {
      {"key", 16}, {"key", 32}, {"iv", 12}, {"traffic upd", 32}, {"traffic upd", 48}};
  for (const auto& c : cases) {
    if (c.len > H::kDigest) continue;  // one HKDF block: at most the hash length
    expand_label<H>(k, c.label, (int)strlen(c.label), c.len, be);
    for (int i = 0; i < c.len; i++) out[i] = (uint8_t)(be[i / 4] >> (24 - 8 * (i % 4)));
    printf("label %s %s %d ", name, strcmp(c.label, "traffic upd") ? c.label : "traffic_upd", c.len);
    hex(out, c.len);
  }
}

int main() {
  run<Sha256>("sha256");
  run<Sha384>("sha384");
  return 0;
}
