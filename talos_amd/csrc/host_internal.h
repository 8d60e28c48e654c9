// host_internal.h — what the host units share: error reporting, the engine and
// session-table objects, run_batch, the env helpers (env_knobs.h).  Never
// included by a .hip.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <vector>

#include "../../include/tlsgpu.h"
#include "../../include/tlsgpu_evp.h"
#include "env_knobs.h"
#include "tlsgpu_internal.h"

// Per-stream scratch for the per-record constants (RecPre) of the queue
// kernels: grow-only hipMalloc buffers, reused in stream order.  (The stream-
// ordered pool — hipMallocAsync — was measured to hand the queue kernel stale
// bytes on MI355X: ~20 % of seal batches in a loop of fresh batches read
// constants the prep kernel had not made visible; plain hipMalloc memory: 0 of
// 240.  See DESIGN.md §4.1.)
struct PreScratch {
  void* ptr = nullptr;
  size_t cap = 0;
};

// Host-resident pipeline state (tlsgpu_open_host): HBM mirrors of the host
// buffers (grow-only), a copy-in stream, `nstreams` compute streams and a
// copy-out stream, chained per chunk by events, so the host-to-device and
// device-to-host DMA engines each stream continuously.
struct HostPipe {
  std::mutex mu;
  unsigned nstreams = 2;
  size_t chunk_bytes = (size_t)32 << 20;
  std::vector<hipStream_t> streams;  // [0] copy in, [1] copy out, [2..] compute
  std::vector<hipEvent_t> events;    // 2 per chunk
  uint8_t *d_in = nullptr, *d_out = nullptr;
  tlsgpu_record* d_recs = nullptr;
  int32_t* d_status = nullptr;
  size_t cap_in = 0, cap_out = 0, cap_recs = 0, cap_status = 0;
};

struct tlsgpu_engine {
  int device;
  hipStream_t stream;
  int num_cus;
  std::mutex pre_mu;
  std::vector<std::pair<hipStream_t, PreScratch>> pre;  // few streams per engine
  HostPipe host;
};

struct tlsgpu_sessions {
  tlsgpu_engine* eng;
  uint32_t capacity;
  tg::DevSession* d_sess;
  tg::DevGcmTables* d_gcm;
  std::vector<int32_t> kinds;  // host mirror of installed kinds
  std::vector<uint8_t> tag_lens;  // and tag lengths (host pipeline output spans)
  std::vector<uint16_t> pad_masks;  // and TLS 1.3 padding masks (DevSession::pad_mask: spans, hints)
  bool cc_padded = false;      // a TLS 1.3 ChaCha session with a padding block was installed
                               // (BatchArgs::cc_pad; never cleared: the PAD kernel runs any table)
  std::vector<const void*> owners;  // SSL* per session for the TaLoS hooks (set_owner)
  int generation = 0;          // 0: nothing installed yet; 12 / 13: every session is TLS <= 1.2 /
                               // TLS 1.3 (version 0x0304, RFC 8446 record layout) — set by
                               // the first install, one generation per table
  bool have[tg::kKinds];       // any session of kind k installed (enum tlsgpu_aead)
  std::atomic<unsigned> hints{0};  // TLSGPU_HINT_* (tlsgpu_sessions_hint)
  std::atomic<bool> wire_key_update{false};  // tlsgpu_sessions_wire_key_update: tlsgpu_open_wire
                                             // cuts TLS 1.3 streams at a KeyUpdate (not a hint)
  // EVP contexts: per-slot event of the slot's last install or scrub, so init
  // and cleanup need not wait on the device (created on a slot's first use)
  std::vector<hipEvent_t> slot_ev;
  // The device key schedule (tlsgpu_sessions_install_secrets / _key_update):
  // kKeyScratchEntries scratch entries and one claim word per slot, allocated by
  // the first secret install (under mu) and never by a key update, which finds
  // them there whenever a slot can hold a secret at all
  tg::KeyScratch* d_key_scratch = nullptr;
  uint32_t* d_key_claim = nullptr;
  std::atomic<uint32_t> key_epoch{0};  // the last key update's claim value
  std::mutex mu;               // host mirrors, when several threads install at once
};

namespace tg {

// bounds: {in_bytes, out_bytes} of a caller's TLS batch (checked by a pre-pass
// that hands the kernels a sanitized copy of the descriptors), or null for
// descriptors the engine built itself (raw EVP jobs, wire framing).
struct Bounds {
  uint64_t in_bytes, out_bytes;
};

int fail(int code, const char* fmt, ...);

#define HIPCHK(x)                                                              \
  do {                                                                         \
    hipError_t _e = (x);                                                       \
    if (_e != hipSuccess)                                                      \
      return tg::fail(TLSGPU_EHIP, "%s: %s", #x, hipGetErrorString(_e));      \
  } while (0)

// tlsgpu_session_params::version of a TLS 1.3 session (include/tlsgpu.h): the
// RFC 8446 section 5 record layout instead of the TLS 1.2 AEAD layout
constexpr uint16_t kTls13Version = 0x0304;
bool valid_params(const tlsgpu_session_params& p);

// batch.cpp.  `kinds`: bit k set = the batch may hold records of AEAD kind k
// (a kernel is launched only for kinds that are installed AND in the mask; the
// EVP queue passes the kinds its jobs use).  type_out: the descriptors again,
// writable, when a TLS 1.3 open shall leave each record's inner content type in
// their type bits (tlsgpu_open_wire).
int run_batch(tlsgpu_sessions* t, const void* d_descs, uint32_t n, const uint8_t* d_in,
              uint8_t* d_out, int32_t* d_status, hipStream_t s, bool seal, bool raw,
              const Bounds* bounds = nullptr, unsigned kinds = ~0u, unsigned hints = ~0u,
              tlsgpu_record* type_out = nullptr);

// batch.cpp: stream s's grow-only scratch of at least `bytes` (null: out of
// memory).  Work queued on s owns it until the next call for s queues more, so
// a pass that uses it must finish reading it in the launches it queues.
void* pre_scratch(tlsgpu_engine* e, hipStream_t s, size_t bytes);

inline uint64_t mono_ns() {
  return (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(
             std::chrono::steady_clock::now().time_since_epoch())
      .count();
}

}  // namespace tg
