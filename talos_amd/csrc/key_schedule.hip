// key_schedule.hip — the TLS 1.3 key schedule behind a traffic secret, on the
// device (RFC 8446 7.1-7.3; include/tlsgpu.h tlsgpu_sessions_install_secrets,
// tlsgpu_sessions_key_update, tlsgpu_wire_key_update_ids).
//
// Two kernels and a memset per chunk of a call:
//   tls13_derive_kernel   one LANE per entry: checks the entry, runs the HKDF
//                         steps (hkdf_device.h) and leaves a scratch entry — the
//                         tlsgpu_session_params an install takes, the secret the
//                         slot keeps, a status;
//   tls13_install_kernel  one WAVE per scratch entry: install_body
//                         (session_install.h), the install of
//                         tlsgpu_sessions_install, then the secret into the slot;
//   hipMemsetAsync        the scratch back to zero.
// A derivation is ten serial compressions with no parallelism inside, so a wave
// per session would idle 63 lanes; the install is the opposite (64 GHASH powers,
// one per lane).  Hence the split, and the kernel boundary between them is also
// what makes every derivation of a call read the old generation before any
// install writes a new one.
#include "hkdf_device.h"
#include "session_install.h"
#include "tlsgpu_internal.h"

namespace tg {

namespace {

// One secret's step.  sec: the secret as big-endian words (H::kDigest / 4 of
// them), replaced by the next generation's when `update`.  key / iv: the first
// key_len / 12 bytes of the two labels' outputs, as big-endian words.
template <class H>
__device__ __forceinline__ void derive(uint32_t sec[12], bool update, uint32_t key_len,
                                       uint32_t key[8], uint32_t iv[3]) {
  constexpr int kWords = H::kDigest / 4;
  hkdf::HmacKey<H> k;
  uint32_t out[12];
  hkdf::hmac_key<H>(k, sec, kWords);
  if (update) {  // the same in every lane
    hkdf::expand_label<H>(k, "traffic upd", 11, H::kDigest, out);
#pragma unroll
    for (int i = 0; i < kWords; i++) sec[i] = out[i];
    hkdf::hmac_key<H>(k, sec, kWords);
  }
  hkdf::expand_label<H>(k, "key", 3, (int)key_len, out);
#pragma unroll
  for (int i = 0; i < 8; i++) key[i] = 4u * i < key_len ? out[i] : 0u;
  hkdf::expand_label<H>(k, "iv", 2, 12, out);
#pragma unroll
  for (int i = 0; i < 3; i++) iv[i] = out[i];
}

__device__ __forceinline__ bool secret_kind(uint32_t kind, uint32_t secret_len) {
  return ((kind == TLSGPU_AES_128_GCM || kind == TLSGPU_CHACHA20_POLY1305_TLS13) &&
          secret_len == 32) ||
         (kind == TLSGPU_AES_256_GCM && secret_len == 48);
}

}  // namespace

__global__ __launch_bounds__(64) void tls13_derive_kernel(
    const tlsgpu_secret_params* __restrict__ secrets, const DevSession* __restrict__ sessions,
    uint32_t capacity, const uint32_t* __restrict__ ids, uint32_t first, uint32_t n,
    uint32_t* __restrict__ claim, uint32_t epoch, KeyScratch* __restrict__ scratch,
    int32_t* __restrict__ status) {
  const uint32_t i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  const bool update = secrets == nullptr;
  uint32_t sec[12];
#pragma unroll
  for (int w = 0; w < 12; w++) sec[w] = 0;
  uint32_t id = 0, kind = 0, secret_len = 0, pad_block = 0;
  int32_t st = TLSGPU_OK;
  bool install = false;  // this entry derives and installs
  if (!update) {
    const tlsgpu_secret_params& p = secrets[i];
    id = first + i;
    kind = (uint32_t)p.aead;
    secret_len = p.secret_len;
    pad_block = p.pad_block;
    const bool pad_ok =
        pad_block <= 1 || (pad_block <= 16384 && (pad_block & (pad_block - 1)) == 0);
    if (id >= capacity) st = TLSGPU_ERANGE;
    else if (!secret_kind(kind, secret_len) || !pad_ok) st = TLSGPU_EINVAL;
    else {
      install = true;
      const uint32_t* w = reinterpret_cast<const uint32_t*>(p.secret);  // 4-B aligned
#pragma unroll
      for (int k = 0; k < 12; k++)
        if (4u * k < secret_len) sec[k] = __builtin_bswap32(w[k]);
    }
  } else {
    id = ids[i];
    if (id == TLSGPU_SESSION_NONE) st = TLSGPU_REKEY_SKIPPED;
    else if (id >= capacity) st = TLSGPU_ERANGE;
    else {
      const DevSession& S = sessions[id];
      kind = S.kind;
      secret_len = S.secret_len;
      pad_block = S.pad_mask ? S.pad_mask + 1u : 0u;  // tls13_pad_mask gives pad_mask back
      if (!scratch || !secret_kind(kind, secret_len)) st = TLSGPU_EINVAL;
      else {
        // an id listed several times: the entry that swaps this call's epoch in
        // derives and installs, the others only report the rekey
        install = atomicExch(&claim[id], epoch) != epoch;
        const uint32_t* w = reinterpret_cast<const uint32_t*>(S.secret);
#pragma unroll
        for (int k = 0; k < 12; k++)
          if (4u * k < secret_len) sec[k] = __builtin_bswap32(w[k]);
      }
    }
  }
  if (status) status[i] = st;
  if (!scratch) return;
  KeyScratch& e = scratch[i];
  if (!install) {  // the rest of the entry stays zero
    e.status = st != TLSGPU_OK ? st : TLSGPU_REKEY_SKIPPED;
    return;
  }
  const uint32_t key_len = kind == TLSGPU_AES_128_GCM ? 16u : 32u;
  uint32_t key[8], iv[3];
  if (secret_len == 48) derive<hkdf::Sha384>(sec, update, key_len, key, iv);
  else derive<hkdf::Sha256>(sec, update, key_len, key, iv);
  e.params.aead = (int32_t)kind;
  e.params.key_len = key_len;
  uint32_t* kw = reinterpret_cast<uint32_t*>(e.params.key);  // offsets 8, 44, 64: 4-B aligned
#pragma unroll
  for (int k = 0; k < 8; k++) kw[k] = __builtin_bswap32(key[k]);
  e.params.fixed_iv_len = 12;
  uint32_t* vw = reinterpret_cast<uint32_t*>(e.params.fixed_iv);
#pragma unroll
  for (int k = 0; k < 3; k++) vw[k] = __builtin_bswap32(iv[k]);
  e.params.tag_len = 16;
  e.params.version = 0x0304;
  e.params.pad_block = (uint16_t)pad_block;
  uint32_t* sw = reinterpret_cast<uint32_t*>(e.secret);
#pragma unroll
  for (int k = 0; k < 12; k++) sw[k] = __builtin_bswap32(sec[k]);  // zero past secret_len
  e.secret_len = secret_len;
  e.id = id;
  e.status = TLSGPU_OK;
}

// One wave per scratch entry: the install of tlsgpu_sessions_install for the
// derived parameters, then the secret the slot keeps.  install_body writes the
// whole header, lane l its 16-byte chunk l, with zeros in the secret fields; the
// four lanes whose chunks hold those fields then store the secret's words into
// their own chunk.  Both stores of every such byte come from one lane, in
// program order, so nothing has to wait for the install's 27 KB of table stores
// (a fence here made this kernel three times as slow as install_sessions).
__global__ __launch_bounds__(64) void tls13_install_kernel(DevSession* __restrict__ sessions,
                                                           DevGcmTables* __restrict__ tables,
                                                           const KeyScratch* __restrict__ scratch,
                                                           uint32_t n) {
  if (blockIdx.x >= n) return;
  const KeyScratch& e = scratch[blockIdx.x];
  if (e.status != TLSGPU_OK) return;  // per entry, so per wave
  const uint32_t id = e.id;
  install_body(sessions, tables, e.params, id);
  constexpr uint32_t kFirst = offsetof(DevSession, secret_len) / 4;  // secret_len, then secret[48]
  constexpr uint32_t kEnd = offsetof(DevSession, reserved) / 4;
  static_assert(offsetof(DevSession, secret) - offsetof(DevSession, secret_len) ==
                        offsetof(KeyScratch, secret) - offsetof(KeyScratch, secret_len) &&
                    kEnd - kFirst == 13,
                "the secret's words are copied as one run");
  uint32_t* slot = reinterpret_cast<uint32_t*>(sessions + id);
  const uint32_t* src = &e.secret_len;
#pragma unroll
  for (uint32_t k = 0; k < 4; k++) {
    const uint32_t w = 4 * threadIdx.x + k;
    if (w >= kFirst && w < kEnd) slot[w] = src[w - kFirst];
  }
}

__global__ void wire_ku_ids_kernel(const tlsgpu_wire_stream* __restrict__ streams,
                                   const tlsgpu_wire_result* __restrict__ results,
                                   uint32_t n_streams, uint32_t* __restrict__ ids) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_streams) return;
  const uint32_t ku = results[i].key_update;
  ids[i] = ku == TLSGPU_WIRE_KU_UPDATE || ku == TLSGPU_WIRE_KU_UPDATE_REQUESTED
               ? streams[i].session
               : TLSGPU_SESSION_NONE;
}

int launch_tls13_derive(const tlsgpu_secret_params* secrets, const DevSession* sessions,
                        uint32_t capacity, const uint32_t* ids, uint32_t first, uint32_t n,
                        uint32_t* claim, uint32_t epoch, KeyScratch* scratch, int32_t* status,
                        hipStream_t s) {
  if (n == 0) return 0;
  hipLaunchKernelGGL(tls13_derive_kernel, dim3((n + 63) / 64), dim3(64), 0, s, secrets, sessions,
                     capacity, ids, first, n, claim, epoch, scratch, status);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_tls13_install(DevSession* sessions, DevGcmTables* tables, const KeyScratch* scratch,
                         uint32_t n, hipStream_t s) {
  if (n == 0) return 0;
  hipLaunchKernelGGL(tls13_install_kernel, dim3(n), dim3(64), 0, s, sessions, tables, scratch, n);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_wire_ku_ids(const tlsgpu_wire_stream* streams, const tlsgpu_wire_result* results,
                       uint32_t n_streams, uint32_t* ids, hipStream_t s) {
  if (n_streams == 0) return 0;
  hipLaunchKernelGGL(wire_ku_ids_kernel, dim3((n_streams + 255) / 256), dim3(256), 0, s, streams,
                     results, n_streams, ids);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace tg
