// session_kernels.hip — device session install and synthetic-data kernels.
//
// tlsgpu_sessions_install() runs install_sessions: one wave per session does
// what aead_aes_gcm_init / CRYPTO_gcm128_init (crypto/evp/e_aes.c:1372-1413,
// crypto/modes/gcm128.c:681-747) and aead_chacha20_poly1305_init
// (e_chacha20poly1305.c:52-79) do at ChangeCipherSpec, plus the GHASH power
// tables the batch kernels need (install_body, session_install.h).
#include "aes_common.h"
#include "session_install.h"
#include "tlsgpu_internal.h"

namespace tg {

__global__ __launch_bounds__(64) void install_sessions(DevSession* __restrict__ sessions,
                                                       DevGcmTables* __restrict__ tables,
                                                       const tlsgpu_session_params* __restrict__ params,
                                                       uint32_t first, uint32_t n) {
  if (blockIdx.x >= n) return;
  install_body(sessions, tables, params[blockIdx.x], first + blockIdx.x);
}

// One session with its parameters as a kernel argument (EVP_AEAD_CTX_init):
// no staging buffer and no copy, so the caller need not wait for the install
// before it reuses its memory (round 3, asynchronous context init).
__global__ __launch_bounds__(64) void install_session_arg(DevSession* __restrict__ sessions,
                                                          DevGcmTables* __restrict__ tables,
                                                          tlsgpu_session_params p, uint32_t id) {
  install_body(sessions, tables, p, id);
}

// Counter-based SplitMix64 bytes (identical to oracle_fill_bytes).
__global__ void fill_synthetic(uint8_t* __restrict__ out, uint64_t stride, uint32_t span_len,
                               uint32_t n, uint64_t seed, uint64_t index0) {
  uint32_t words = (span_len + 7) / 8;
  uint64_t total = (uint64_t)words * n;
  for (uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; g < total;
       g += (uint64_t)gridDim.x * blockDim.x) {
    uint64_t span = g / words, w = g % words;
    uint64_t st = seed ^ ((index0 + span) * 0xD1B54A32D192ED03ull);
    uint64_t z = st + (w + 1) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    uint8_t* p = out + span * stride + w * 8;
    uint32_t left = span_len - (uint32_t)(w * 8);
    if (left >= 8 && ((uintptr_t)p & 7) == 0) {
      *(uint64_t*)p = z;
    } else {
      for (uint32_t k = 0; k < 8 && k < left; k++) p[k] = (uint8_t)(z >> (8 * k));
    }
  }
}

// Variable-length spans in one launch: span i (offs[i], lens[i]) keyed index0 + i.
// One workgroup per span (grid-strided), 8 B per thread-step.
__global__ void fill_synthetic_spans(uint8_t* __restrict__ out, const uint64_t* __restrict__ offs,
                                     const uint32_t* __restrict__ lens, uint32_t n, uint64_t seed,
                                     uint64_t index0) {
  for (uint32_t span = blockIdx.x; span < n; span += gridDim.x) {
    const uint32_t len = lens[span];
    uint8_t* base = out + offs[span];
    const uint64_t st = seed ^ ((index0 + span) * 0xD1B54A32D192ED03ull);
    for (uint32_t w = threadIdx.x; w * 8 < len; w += blockDim.x) {
      uint64_t z = st + (uint64_t)(w + 1) * 0x9E3779B97F4A7C15ull;
      z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
      z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
      z ^= z >> 31;
      uint8_t* p = base + (uint64_t)w * 8;
      const uint32_t left = len - w * 8;
      if (left >= 8 && ((uintptr_t)p & 7) == 0) {
        *(uint64_t*)p = z;
      } else {
        for (uint32_t k = 0; k < 8 && k < left; k++) p[k] = (uint8_t)(z >> (8 * k));
      }
    }
  }
}

int launch_fill_synthetic_spans(uint8_t* d_out, const uint64_t* d_offs, const uint32_t* d_lens,
                                uint32_t n, uint64_t seed, uint64_t index0, hipStream_t s) {
  if (n == 0) return 0;
  const uint32_t blocks = n < 65536 ? n : 65536;
  hipLaunchKernelGGL(fill_synthetic_spans, dim3(blocks), dim3(256), 0, s, d_out, d_offs, d_lens, n,
                     seed, index0);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

// Batch ABI bounds (tlsgpu_open_batch / _seal_batch take the sizes of d_in and
// d_out): a record whose input or output span leaves its buffer is dropped
// from the kernels' copy of the descriptors (session 0xFFFFFFFF, which every
// batch kernel skips) and gets TLSGPU_REC_OUT_OF_BOUNDS.  Output span = the
// plaintext on open (fragment - explicit nonce - tag), the fragment on seal.
// Also the batch's setup (one launch instead of three): every record's
// initial status (TLSGPU_REC_PUBLIC_INVALID, the status of a record no kernel
// takes, or TLSGPU_REC_OUT_OF_BOUNDS) and, from block 0, the zeroed control
// words of the queue kernels (ctl_words uint32s, may be 0).
__global__ void check_record_bounds(const tlsgpu_record* __restrict__ recs,
                                    tlsgpu_record* __restrict__ safe, uint32_t n,
                                    const DevSession* __restrict__ sessions, uint32_t n_sessions,
                                    uint64_t in_bytes, uint64_t out_bytes, int seal,
                                    int32_t* __restrict__ status, uint32_t* __restrict__ ctl,
                                    uint32_t ctl_words) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (blockIdx.x == 0)
    for (uint32_t w = threadIdx.x; w < ctl_words; w += blockDim.x) ctl[w] = 0;
  if (i >= n) return;
  tlsgpu_record r = recs[i];
  int32_t st = TLSGPU_REC_PUBLIC_INVALID;
  if (r.session < n_sessions) {
    const DevSession& S = sessions[r.session];
    const uint64_t eiv = S.nonce_in_record ? 8u : 0u, tag = S.tag_len;
    // a TLS 1.3 seal writes content || type || padding || tag (RFC 8446 5.2, 5.4)
    const uint64_t len = r.len_type & 0xFFFFFFu;
    const uint64_t extra = tls13_session(S.kind, S.nonce_in_record)
                               ? tls13_inner_len((uint32_t)len, S.pad_mask) - len
                               : 0u;
    const uint64_t in_len = len;
    const uint64_t out_len =
        seal ? len + eiv + extra + tag : (len >= eiv + tag ? len - eiv - tag : 0);
    if (r.in_off > in_bytes || in_len > in_bytes - r.in_off || r.out_off > out_bytes ||
        out_len > out_bytes - r.out_off) {
      r.session = 0xFFFFFFFFu;
      st = TLSGPU_REC_OUT_OF_BOUNDS;
    }
  }
  status[i] = st;
  safe[i] = r;
}

int launch_check_bounds(const tlsgpu_record* recs, tlsgpu_record* safe, uint32_t n,
                        const DevSession* sessions, uint32_t n_sessions, uint64_t in_bytes,
                        uint64_t out_bytes, bool seal, int32_t* status, uint32_t* ctl,
                        uint32_t ctl_words, hipStream_t s) {
  if (n == 0) return 0;
  hipLaunchKernelGGL(check_record_bounds, dim3((n + 255) / 256), dim3(256), 0, s, recs, safe, n,
                     sessions, n_sessions, in_bytes, out_bytes, seal ? 1 : 0, status, ctl,
                     ctl_words);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

// TLS 1.3 open, the unpad pass (RFC 8446 5.4): the cipher kernels left every
// record's status = the length m of its decrypted TLSInnerPlaintext (content ||
// type || zeros) at out_off, or a negative status, BAD_MAC's zero-fill done.
// Records of TLS 1.3 sessions with status >= 0 get the content length instead:
// the index of the last non-zero byte (the inner content type sits there), or
// TLSGPU_REC_NO_CONTENT_TYPE when there is none; the bytes stay as decrypted.
// One lane per record looks at the last byte, which is the type whenever the
// sender did not pad; for the others the wave scans backwards, 64 x 16 B per
// step, one record after the other.  Negative statuses and records of other
// sessions are left alone.  Launched by the TLS 1.3 launchers only, once per
// AES key size after that size's kernels and once for the ChaCha sessions after
// theirs (`rounds`: a record is taken in the pass of its own session's AES
// rounds, 0 for ChaCha, so never twice): a TLS 1.2 batch launches nothing new,
// and a TLS 1.3 batch no pass for a kind its table does not hold.
// type_out != null (tlsgpu_open_wire): the record's
// inner content type also replaces the type bits of type_out[r].len_type.
__global__ __launch_bounds__(256) void tls13_unpad_kernel(const tlsgpu_record* recs,  // may be type_out
                                                          uint32_t n,
                                                          const DevSession* __restrict__ sessions,
                                                          uint32_t n_sessions, uint32_t rounds,
                                                          const uint8_t* __restrict__ out,
                                                          int32_t* __restrict__ status,
                                                          tlsgpu_record* type_out) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  const uint8_t* p = nullptr;
  uint32_t m = 0, lt = 0;
  bool scan = false;
  // the content length is known: the status, and the type where it is wanted
  auto done = [&](int32_t cl) {
    status[r] = cl;
    if (type_out && cl >= 0) type_out[r].len_type = ((uint32_t)p[cl] << 24) | (lt & 0xFFFFFFu);
  };
  if (r < n) {
    const tlsgpu_record d = recs[r];
    const int32_t st = status[r];
    if (d.session < n_sessions && st >= 0) {
      const DevSession& S = sessions[d.session];
      if (tls13_session(S.kind, S.nonce_in_record) && S.rounds == rounds) {
        p = out + d.out_off;
        m = (uint32_t)st;
        lt = d.len_type;
        if (m == 0) done(TLSGPU_REC_NO_CONTENT_TYPE);
        else if (p[m - 1] != 0) done((int32_t)(m - 1));
        else scan = true;
      }
    }
  }
  // padded records: bytes [0, end) still unknown, byte end is zero
  for (uint64_t todo = __ballot(scan); todo != 0; todo &= todo - 1) {
    const int k = __builtin_ctzll(todo);
    const uint64_t pa = ((uint64_t)(uint32_t)__shfl((int)((uintptr_t)p >> 32), k) << 32) |
                        (uint32_t)__shfl((int)(uint32_t)(uintptr_t)p, k);
    const uint8_t* pk = reinterpret_cast<const uint8_t*>(pa);
    int32_t found = -1;
    for (uint32_t end = (uint32_t)__shfl((int)m, k) - 1; end != 0 && found < 0;
         end -= min(end, 16u * kWave)) {
      int32_t idx = -1;
      if (16u * lane < end) {  // this lane's piece [lo, hi), nearest the end for lane 0
        const uint32_t hi = end - 16u * lane, lo = hi > 16u ? hi - 16u : 0u;
        uint32_t v[4];
        if (hi - lo == 16u) load16_any(pk + lo, v);
        else load16_upto(pk + lo, hi - lo, v);  // whole dwords: bytes past the piece masked here
#pragma unroll
        for (int w = 3; w >= 0; w--) {
          const int32_t b = (int32_t)(hi - lo) - 4 * w;
          v[w] &= b >= 4 ? 0xFFFFFFFFu : (b <= 0 ? 0u : ((1u << (8 * b)) - 1u));
        }
#pragma unroll
        for (int w = 3; w >= 0; w--)
          if (idx < 0 && v[w] != 0) idx = (int32_t)(lo + 4 * w + (31 - __builtin_clz(v[w])) / 8);
      }
      const uint64_t has = __ballot(idx >= 0);
      if (has) found = __shfl(idx, __builtin_ctzll(has));  // the lowest lane holds the last one
    }
    if ((int)lane == k) done(found >= 0 ? found : TLSGPU_REC_NO_CONTENT_TYPE);
  }
}

int launch_tls13_unpad(const BatchArgs& a, int rounds, hipStream_t s) {
  if (a.n == 0) return 0;
  hipLaunchKernelGGL(tls13_unpad_kernel, dim3((a.n + 255) / 256), dim3(256), 0, s,
                     reinterpret_cast<const tlsgpu_record*>(a.descs), a.n, a.sessions, a.n_sessions,
                     (uint32_t)rounds, a.out, a.status, a.type_out);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_session_install(DevSession* sessions, DevGcmTables* tables,
                           const tlsgpu_session_params* d_params, uint32_t first, uint32_t n,
                           hipStream_t s) {
  if (n == 0) return 0;
  hipLaunchKernelGGL(install_sessions, dim3(n), dim3(64), 0, s, sessions, tables,
                     d_params, first, n);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_session_install_arg(DevSession* sessions, DevGcmTables* tables,
                               const tlsgpu_session_params& p, uint32_t id, hipStream_t s) {
  hipLaunchKernelGGL(install_session_arg, dim3(1), dim3(64), 0, s, sessions, tables, p, id);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

// EVP_AEAD_CTX_init's install (round 5): the calling thread built the slot's
// image on the host (session_host.cpp) in its pinned key area; one 256-thread
// workgroup copies it into the slot (zero-copy reads of the pinned image), the
// GCM tables only when `table_bytes` != 0.  Kernel arguments carry pointers
// only — no key material.
__global__ __launch_bounds__(256) void upload_session(const uint4* __restrict__ img,
                                                      DevSession* __restrict__ sess,
                                                      DevGcmTables* __restrict__ tab,
                                                      uint32_t table_bytes) {
  constexpr uint32_t kS = sizeof(DevSession) / 16;
  const uint32_t n = kS + table_bytes / 16;
  for (uint32_t i = threadIdx.x; i < n; i += 256) {
    const uint4 v = img[i];
    if (i < kS) reinterpret_cast<uint4*>(sess)[i] = v;
    else reinterpret_cast<uint4*>(tab)[i - kS] = v;
  }
}

// EVP_AEAD_CTX_cleanup's scrub (e_aes.c:1415-1422 explicit_bzero analogue):
// the slot's DevSession and GCM tables zeroed in one launch.
__global__ __launch_bounds__(256) void scrub_session(DevSession* __restrict__ sess,
                                                     DevGcmTables* __restrict__ tab) {
  constexpr uint32_t kS = sizeof(DevSession) / 16, kT = sizeof(DevGcmTables) / 16;
  for (uint32_t i = threadIdx.x; i < kS + kT; i += 256) {
    if (i < kS) reinterpret_cast<uint4*>(sess)[i] = make_uint4(0, 0, 0, 0);
    else reinterpret_cast<uint4*>(tab)[i - kS] = make_uint4(0, 0, 0, 0);
  }
}

int launch_upload_session(const void* img, DevSession* sess, DevGcmTables* tab,
                          uint32_t table_bytes, hipStream_t s) {
  hipLaunchKernelGGL(upload_session, dim3(1), dim3(256), 0, s,
                     reinterpret_cast<const uint4*>(img), sess, tab, table_bytes);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_scrub_session(DevSession* sess, DevGcmTables* tab, hipStream_t s) {
  hipLaunchKernelGGL(scrub_session, dim3(1), dim3(256), 0, s, sess, tab);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_fill_synthetic(uint8_t* d_out, uint64_t stride, uint32_t span_len, uint32_t n,
                          uint64_t seed, uint64_t index0, hipStream_t s) {
  if (n == 0 || span_len == 0) return 0;
  uint64_t words = (uint64_t)((span_len + 7) / 8) * n;
  uint64_t blocks = (words + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  hipLaunchKernelGGL(fill_synthetic, dim3((uint32_t)blocks), dim3(256), 0, s, d_out, stride,
                     span_len, n, seed, index0);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace tg
