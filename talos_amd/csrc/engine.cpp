// engine.cpp — the base of libtlsgpu.so's C ABI (include/tlsgpu.h): error
// reporting, engines, session tables and their install (valid_params), the
// device key schedule's calls (tlsgpu_sessions_install_secrets, _key_update), the
// bitsliced AES-ECB self-test entry and the thin device helper API (memory,
// streams, events).  The other host units: batch.cpp (the knobs, plan_batch /
// run_batch, tlsgpu_open_batch / tlsgpu_seal_batch), host_paths.cpp
// (host-resident and wire paths), evp_aead.cpp, evp_doorbell.cpp,
// evp_queue.cpp, evp_cipher.cpp (the drop-in EVP surfaces), group.cpp,
// session_host.cpp, talos_hooks.cpp.
#include <cstdarg>

#include "host_internal.h"

using namespace tg;

// ---------------------------------------------------------------------------
// error reporting
static thread_local char g_err[256] = "";

int tg::fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}

extern "C" const char* tlsgpu_last_error(void) { return g_err; }

// For group.cpp (same library, not exported): set the calling thread's
// tlsgpu_last_error, e.g. to a member worker's reason.
extern "C" int tg_internal_set_error(int code, const char* msg) {
  return fail(code, "%s", msg ? msg : "");
}

extern "C" int tlsgpu_device_count(int* count) {
  if (!count) return fail(TLSGPU_EINVAL, "null out");
  *count = 0;
  HIPCHK(hipGetDeviceCount(count));
  return TLSGPU_OK;
}

extern "C" int tlsgpu_engine_create(int device, tlsgpu_engine** out) {
  if (!out) return fail(TLSGPU_EINVAL, "null out");
  *out = nullptr;
  int count = 0;
  HIPCHK(hipGetDeviceCount(&count));
  if (device < 0 || device >= count)
    return fail(TLSGPU_EINVAL, "device %d out of range (%d GPUs)", device, count);
  HIPCHK(hipSetDevice(device));
  auto* e = new (std::nothrow) tlsgpu_engine();
  if (!e) return fail(TLSGPU_ENOMEM, "engine alloc");
  e->device = device;
  HIPCHK(hipDeviceGetAttribute(&e->num_cus, hipDeviceAttributeMultiprocessorCount, device));
  HIPCHK(hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking));
  *out = e;
  return TLSGPU_OK;
}

extern "C" void tlsgpu_engine_destroy(tlsgpu_engine* e) {
  if (!e) return;
  (void)hipSetDevice(e->device);
  (void)hipStreamSynchronize(e->stream);
  (void)hipDeviceSynchronize();  // batches on user streams may still use the scratch
  for (auto& kv : e->pre) (void)hipFree(kv.second.ptr);
  for (hipStream_t hs : e->host.streams) (void)hipStreamDestroy(hs);  // host pipeline
  for (hipEvent_t ev : e->host.events) (void)hipEventDestroy(ev);
  (void)hipFree(e->host.d_in);
  (void)hipFree(e->host.d_out);
  (void)hipFree(e->host.d_recs);
  (void)hipFree(e->host.d_status);
  (void)hipStreamDestroy(e->stream);
  delete e;
}

extern "C" void* tlsgpu_engine_stream(tlsgpu_engine* e) { return e ? (void*)e->stream : nullptr; }

extern "C" int tlsgpu_engine_sync(tlsgpu_engine* e) {
  if (!e) return fail(TLSGPU_EINVAL, "null engine");
  HIPCHK(hipSetDevice(e->device));
  HIPCHK(hipStreamSynchronize(e->stream));
  return TLSGPU_OK;
}

extern "C" int tlsgpu_engine_num_cus(tlsgpu_engine* e) { return e ? e->num_cus : 0; }

extern "C" int tlsgpu_sessions_create(tlsgpu_engine* e, uint32_t capacity, tlsgpu_sessions** out) {
  if (!e || !out || capacity == 0) return fail(TLSGPU_EINVAL, "bad arguments");
  *out = nullptr;
  HIPCHK(hipSetDevice(e->device));
  auto* t = new (std::nothrow) tlsgpu_sessions();
  if (!t) return fail(TLSGPU_ENOMEM, "sessions alloc");
  t->eng = e;
  t->capacity = capacity;
  t->kinds.assign(capacity, 0);
  t->tag_lens.assign(capacity, 16);
  t->pad_masks.assign(capacity, 0);
  t->owners.assign(capacity, nullptr);
  memset(t->have, 0, sizeof(t->have));
  if (hipMalloc(&t->d_sess, sizeof(DevSession) * (size_t)capacity) != hipSuccess ||
      hipMalloc(&t->d_gcm, sizeof(DevGcmTables) * (size_t)capacity) != hipSuccess) {
    (void)hipFree(t->d_sess);
    delete t;
    return fail(TLSGPU_ENOMEM, "device session table (%u sessions)", capacity);
  }
  HIPCHK(hipMemsetAsync(t->d_sess, 0, sizeof(DevSession) * (size_t)capacity, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  *out = t;
  return TLSGPU_OK;
}

extern "C" void tlsgpu_sessions_destroy(tlsgpu_sessions* t) {
  if (!t) return;
  (void)hipSetDevice(t->eng->device);
  (void)hipStreamSynchronize(t->eng->stream);
  for (hipEvent_t ev : t->slot_ev)
    if (ev) {
      (void)hipEventSynchronize(ev);  // a scrub still running on a call stream
      (void)hipEventDestroy(ev);
    }
  (void)hipFree(t->d_sess);
  (void)hipFree(t->d_gcm);
  if (t->d_key_scratch) (void)hipFree(t->d_key_scratch);  // zero between calls
  if (t->d_key_claim) (void)hipFree(t->d_key_claim);
  delete t;
}

bool tg::valid_params(const tlsgpu_session_params& p) {
  uint32_t tag = p.tag_len == 0 ? 16 : p.tag_len;
  if (tag > 16 || p.fixed_iv_len > 12) return false;
  // TLS 1.3 (RFC 8446 section 5.3): AES-GCM or the TLS 1.3 ChaCha kind (the TLS 1.2
  // ChaCha kinds name TLS 1.2 record layouts), the whole 12-byte write IV, a 16-byte tag
  if (p.version == kTls13Version &&
      (p.fixed_iv_len != 12 || tag != 16 ||
       (p.aead != TLSGPU_AES_128_GCM && p.aead != TLSGPU_AES_256_GCM &&
        p.aead != TLSGPU_CHACHA20_POLY1305_TLS13)))
    return false;
  // ... and that kind exists in TLS 1.3 only
  if (p.aead == TLSGPU_CHACHA20_POLY1305_TLS13 && p.version != kTls13Version) return false;
  // the TLS 1.3 padding block (read for that version only): none, or a power of
  // two up to 16384 (tls13_inner_len rounds with a mask)
  if (p.version == kTls13Version && p.pad_block > 1 &&
      (p.pad_block > 16384 || (p.pad_block & (p.pad_block - 1)) != 0))
    return false;
  switch (p.aead) {
    case TLSGPU_AES_128_GCM: return p.key_len == 16;
    case TLSGPU_AES_256_GCM:
    case TLSGPU_CHACHA20_POLY1305:
    case TLSGPU_CHACHA20_POLY1305_OLD:
    case TLSGPU_CHACHA20_POLY1305_TLS13: return p.key_len == 32;
  }
  return false;
}

extern "C" int tlsgpu_sessions_install(tlsgpu_sessions* t, uint32_t first, uint32_t n,
                                       const tlsgpu_session_params* params) {
  if (!t || (!params && n)) return fail(TLSGPU_EINVAL, "bad arguments");
  if ((uint64_t)first + n > t->capacity)
    return fail(TLSGPU_ERANGE, "sessions [%u, %u) exceed capacity %u", first, first + n,
                t->capacity);
  for (uint32_t i = 0; i < n; i++)
    if (!valid_params(params[i])) return fail(TLSGPU_EINVAL, "invalid session params at %u", i);
  if (n == 0) return TLSGPU_OK;
  // one record generation per table (include/tlsgpu.h): the GCM kernels are
  // compiled per generation and run_batch launches the table's set
  {
    std::lock_guard<std::mutex> lk(t->mu);
    int gen = t->generation;
    for (uint32_t i = 0; i < n; i++) {
      const int g = params[i].version == kTls13Version ? 13 : 12;
      if (gen != 0 && g != gen)
        return fail(TLSGPU_EINVAL, "session %u: TLS 1.%d params in a TLS 1.%d session table", i,
                    g - 10, gen - 10);
      gen = g;
    }
    t->generation = gen;
  }
  HIPCHK(hipSetDevice(t->eng->device));
  tlsgpu_session_params* d_params = nullptr;
  HIPCHK(hipMalloc(&d_params, sizeof(tlsgpu_session_params) * n));
  hipError_t err = hipMemcpyAsync(d_params, params, sizeof(tlsgpu_session_params) * n,
                                  hipMemcpyHostToDevice, t->eng->stream);
  int rc = err == hipSuccess
               ? launch_session_install(t->d_sess, t->d_gcm, d_params, first, n, t->eng->stream)
               : -1;
  // the raw keys do not outlive the install in device memory
  (void)hipMemsetAsync(d_params, 0, sizeof(tlsgpu_session_params) * n, t->eng->stream);
  hipError_t serr = hipStreamSynchronize(t->eng->stream);
  (void)hipFree(d_params);
  if (err != hipSuccess || rc != 0 || serr != hipSuccess)
    return fail(TLSGPU_EHIP, "session install failed: %s",
                hipGetErrorString(err != hipSuccess ? err : serr));
  std::lock_guard<std::mutex> lk(t->mu);
  for (uint32_t i = 0; i < n; i++) {
    t->kinds[first + i] = params[i].aead;
    t->tag_lens[first + i] = (uint8_t)(params[i].tag_len ? params[i].tag_len : 16);
    t->pad_masks[first + i] = (uint16_t)tls13_pad_mask(params[i].version, params[i].pad_block);
    if (params[i].aead == TLSGPU_CHACHA20_POLY1305_TLS13 && t->pad_masks[first + i])
      t->cc_padded = true;
    t->have[params[i].aead] = true;
  }
  return TLSGPU_OK;
}

// ---------------------------------------------------------------------------
// The device key schedule (include/tlsgpu.h; key_schedule.hip).
// The launchers are weak references for the reason host_paths.cpp's are: a link
// of the host objects against a launcher list written before these calls
// existed (the CPU tests' recording HIP stub) must still resolve, and there the
// calls fail loudly, after their argument checks and before any HIP call.
namespace tg {
__attribute__((weak)) int launch_tls13_derive(const tlsgpu_secret_params* secrets,
                                              const DevSession* sessions, uint32_t capacity,
                                              const uint32_t* ids, uint32_t first, uint32_t n,
                                              uint32_t* claim, uint32_t epoch, KeyScratch* scratch,
                                              int32_t* status, hipStream_t s);
__attribute__((weak)) int launch_tls13_install(DevSession* sessions, DevGcmTables* tables,
                                               const KeyScratch* scratch, uint32_t n,
                                               hipStream_t s);
__attribute__((weak)) int launch_wire_ku_ids(const tlsgpu_wire_stream* streams,
                                             const tlsgpu_wire_result* results, uint32_t n_streams,
                                             uint32_t* ids, hipStream_t s);
}  // namespace tg

static bool valid_secret(const tlsgpu_secret_params& p) {
  uint32_t want = 0;
  switch (p.aead) {
    case TLSGPU_AES_128_GCM:
    case TLSGPU_CHACHA20_POLY1305_TLS13: want = 32; break;  // SHA-256 suites
    case TLSGPU_AES_256_GCM: want = 48; break;              // SHA-384
    default: return false;
  }
  if (p.secret_len != want) return false;
  // the padding block as valid_params has it
  return p.pad_block <= 1 || (p.pad_block <= 16384 && (p.pad_block & (p.pad_block - 1)) == 0);
}

// derive + install + scrub of one chunk's scratch entries, queued on s
static int queue_key_chunk(tlsgpu_sessions* t, const tlsgpu_secret_params* d_secrets,
                           const uint32_t* d_ids, uint32_t first, uint32_t n, uint32_t epoch,
                           int32_t* d_status, hipStream_t s) {
  if (launch_tls13_derive(d_secrets, t->d_sess, t->capacity, d_ids, first, n, t->d_key_claim, epoch,
                          t->d_key_scratch, d_status, s))
    return -1;
  if (!t->d_key_scratch) return 0;  // no slot of this table ever held a secret: statuses only
  if (launch_tls13_install(t->d_sess, t->d_gcm, t->d_key_scratch, n, s)) return -1;
  // the derived keys and secrets do not outlive the call in the scratch
  return hipMemsetAsync(t->d_key_scratch, 0, sizeof(KeyScratch) * (size_t)n, s) == hipSuccess ? 0
                                                                                               : -1;
}

extern "C" int tlsgpu_sessions_install_secrets(tlsgpu_sessions* t, uint32_t first, uint32_t n,
                                               const tlsgpu_secret_params* params) {
  if (!t || (!params && n)) return fail(TLSGPU_EINVAL, "bad arguments");
  if ((uint64_t)first + n > t->capacity)
    return fail(TLSGPU_ERANGE, "sessions [%u, %u) exceed capacity %u", first, first + n,
                t->capacity);
  for (uint32_t i = 0; i < n; i++)
    if (!valid_secret(params[i])) return fail(TLSGPU_EINVAL, "invalid secret params at %u", i);
  if (n == 0) return TLSGPU_OK;
  {
    // a TLS 1.3 install under the one-generation-per-table rule
    std::lock_guard<std::mutex> lk(t->mu);
    if (t->generation == 12)
      return fail(TLSGPU_EINVAL, "TLS 1.3 traffic secrets in a TLS 1.2 session table");
    if (!launch_tls13_derive || !launch_tls13_install)
      return fail(TLSGPU_EHIP, "the key schedule kernels are not linked into this library");
    t->generation = 13;
  }
  HIPCHK(hipSetDevice(t->eng->device));
  hipStream_t s = t->eng->stream;
  {
    std::lock_guard<std::mutex> lk(t->mu);
    if (!t->d_key_scratch) {
      KeyScratch* sc = nullptr;
      uint32_t* claim = nullptr;
      if (hipMalloc(&sc, sizeof(KeyScratch) * (size_t)kKeyScratchEntries) != hipSuccess ||
          hipMalloc(&claim, sizeof(uint32_t) * (size_t)t->capacity) != hipSuccess) {
        (void)hipFree(sc);
        return fail(TLSGPU_ENOMEM, "key schedule scratch");
      }
      hipError_t e1 = hipMemsetAsync(sc, 0, sizeof(KeyScratch) * (size_t)kKeyScratchEntries, s);
      hipError_t e2 = hipMemsetAsync(claim, 0, sizeof(uint32_t) * (size_t)t->capacity, s);
      if (e1 != hipSuccess || e2 != hipSuccess) {
        (void)hipStreamSynchronize(s);
        (void)hipFree(sc);
        (void)hipFree(claim);
        return fail(TLSGPU_EHIP, "key schedule scratch: %s",
                    hipGetErrorString(e1 != hipSuccess ? e1 : e2));
      }
      t->d_key_claim = claim;
      t->d_key_scratch = sc;
    }
  }
  tlsgpu_secret_params* d_in = nullptr;
  HIPCHK(hipMalloc(&d_in, sizeof(tlsgpu_secret_params) * (size_t)n));
  hipError_t err = hipMemcpyAsync(d_in, params, sizeof(tlsgpu_secret_params) * (size_t)n,
                                  hipMemcpyHostToDevice, s);
  int rc = err == hipSuccess ? 0 : -1;
  for (uint32_t off = 0; rc == 0 && off < n; off += kKeyScratchEntries)
    rc = queue_key_chunk(t, d_in + off, nullptr, first + off, std::min(n - off, kKeyScratchEntries),
                         0, nullptr, s);
  // the secrets do not outlive the install in the staging copy
  (void)hipMemsetAsync(d_in, 0, sizeof(tlsgpu_secret_params) * (size_t)n, s);
  hipError_t serr = hipStreamSynchronize(s);
  (void)hipFree(d_in);
  if (err != hipSuccess || rc != 0 || serr != hipSuccess)
    return fail(TLSGPU_EHIP, "secret install failed: %s",
                hipGetErrorString(err != hipSuccess ? err : serr));
  std::lock_guard<std::mutex> lk(t->mu);
  for (uint32_t i = 0; i < n; i++) {
    t->kinds[first + i] = params[i].aead;
    t->tag_lens[first + i] = 16;
    t->pad_masks[first + i] = (uint16_t)tls13_pad_mask(kTls13Version, params[i].pad_block);
    if (params[i].aead == TLSGPU_CHACHA20_POLY1305_TLS13 && t->pad_masks[first + i])
      t->cc_padded = true;
    t->have[params[i].aead] = true;
  }
  return TLSGPU_OK;
}

extern "C" int tlsgpu_sessions_key_update(tlsgpu_sessions* t, const uint32_t* d_ids, uint32_t n,
                                          int32_t* d_status, void* stream) {
  if (!t || (n && (!d_ids || !d_status))) return fail(TLSGPU_EINVAL, "bad arguments");
  if (n == 0) return TLSGPU_OK;
  if (!launch_tls13_derive || !launch_tls13_install)
    return fail(TLSGPU_EHIP, "the key schedule kernels are not linked into this library");
  HIPCHK(hipSetDevice(t->eng->device));
  hipStream_t s = stream ? (hipStream_t)stream : t->eng->stream;
  // this call's claim value: unique among the table's calls and never 0, the
  // value of a slot no call has claimed (a wrap after 2^32 calls skips it)
  uint32_t epoch = t->key_epoch.fetch_add(1, std::memory_order_relaxed) + 1;
  if (epoch == 0) epoch = t->key_epoch.fetch_add(1, std::memory_order_relaxed) + 1;
  for (uint32_t off = 0; off < n; off += kKeyScratchEntries)
    if (queue_key_chunk(t, nullptr, d_ids + off, 0, std::min(n - off, kKeyScratchEntries), epoch,
                        d_status + off, s))
      return fail(TLSGPU_EHIP, "key update: %s", hipGetErrorString(hipGetLastError()));
  return TLSGPU_OK;
}

extern "C" int tlsgpu_wire_key_update_ids(tlsgpu_sessions* t, const tlsgpu_wire_stream* d_streams,
                                          const tlsgpu_wire_result* d_results, uint32_t n_streams,
                                          uint32_t* d_ids, void* stream) {
  if (!t || (n_streams && (!d_streams || !d_results || !d_ids)))
    return fail(TLSGPU_EINVAL, "bad arguments");
  if (n_streams == 0) return TLSGPU_OK;
  if (!launch_wire_ku_ids)
    return fail(TLSGPU_EHIP, "the key schedule kernels are not linked into this library");
  HIPCHK(hipSetDevice(t->eng->device));
  if (launch_wire_ku_ids(d_streams, d_results, n_streams, d_ids,
                         stream ? (hipStream_t)stream : t->eng->stream))
    return fail(TLSGPU_EHIP, "key update ids: %s", hipGetErrorString(hipGetLastError()));
  return TLSGPU_OK;
}

extern "C" int tlsgpu_aes_ecb_bitsliced(tlsgpu_sessions* t, uint32_t session, const uint8_t* d_in,
                                        uint8_t* d_out, uint32_t nblocks, void* stream) {
  if (!t || (nblocks && (!d_in || !d_out))) return fail(TLSGPU_EINVAL, "bad arguments");
  if (session >= t->capacity ||
      (t->kinds[session] != TLSGPU_AES_128_GCM && t->kinds[session] != TLSGPU_AES_256_GCM))
    return fail(TLSGPU_EINVAL, "session %u is not an installed AES-GCM session", session);
#ifdef TG_EXPERIMENTAL
  HIPCHK(hipSetDevice(t->eng->device));
  int rounds = t->kinds[session] == TLSGPU_AES_128_GCM ? 10 : 14;
  if (launch_bs_ecb(t->d_sess, session, rounds, d_in, d_out, nblocks,
                    stream ? (hipStream_t)stream : t->eng->stream))
    return fail(TLSGPU_EHIP, "bs ecb launch: %s", hipGetErrorString(hipGetLastError()));
  return TLSGPU_OK;
#else
  (void)stream;
  return fail(TLSGPU_EINVAL, "bitsliced AES not built (make EXPERIMENTAL=1)");
#endif
}

// ---------------------------------------------------------------------------
// memory / streams / events
#define ENG_OR_FAIL(e) \
  if (!(e)) return fail(TLSGPU_EINVAL, "null engine"); \
  HIPCHK(hipSetDevice((e)->device))

static hipStream_t pick(tlsgpu_engine* e, void* s) { return s ? (hipStream_t)s : e->stream; }

extern "C" int tlsgpu_malloc(tlsgpu_engine* e, size_t bytes, void** d_ptr) {
  ENG_OR_FAIL(e);
  if (!d_ptr) return fail(TLSGPU_EINVAL, "null out");
  if (hipMalloc(d_ptr, bytes ? bytes : 1) != hipSuccess)
    return fail(TLSGPU_ENOMEM, "hipMalloc(%zu)", bytes);
  return TLSGPU_OK;
}
extern "C" int tlsgpu_free(tlsgpu_engine* e, void* d_ptr) {
  ENG_OR_FAIL(e);
  HIPCHK(hipFree(d_ptr));
  return TLSGPU_OK;
}
extern "C" int tlsgpu_host_alloc(tlsgpu_engine* e, size_t bytes, void** h_ptr) {
  ENG_OR_FAIL(e);
  if (!h_ptr) return fail(TLSGPU_EINVAL, "null out");
  if (hipHostMalloc(h_ptr, bytes ? bytes : 1, hipHostMallocDefault) != hipSuccess)
    return fail(TLSGPU_ENOMEM, "hipHostMalloc(%zu)", bytes);
  return TLSGPU_OK;
}
extern "C" int tlsgpu_host_free(tlsgpu_engine* e, void* h_ptr) {
  ENG_OR_FAIL(e);
  HIPCHK(hipHostFree(h_ptr));
  return TLSGPU_OK;
}
extern "C" int tlsgpu_memcpy(tlsgpu_engine* e, void* dst, const void* src, size_t bytes,
                             void* stream) {
  ENG_OR_FAIL(e);
  if (bytes) HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDefault, pick(e, stream)));
  return TLSGPU_OK;
}
extern "C" int tlsgpu_memset(tlsgpu_engine* e, void* d_ptr, int value, size_t bytes,
                             void* stream) {
  ENG_OR_FAIL(e);
  if (bytes) HIPCHK(hipMemsetAsync(d_ptr, value, bytes, pick(e, stream)));
  return TLSGPU_OK;
}
extern "C" int tlsgpu_stream_create(tlsgpu_engine* e, void** stream) {
  ENG_OR_FAIL(e);
  hipStream_t s;
  HIPCHK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
  *stream = s;
  return TLSGPU_OK;
}
extern "C" int tlsgpu_stream_destroy(tlsgpu_engine* e, void* stream) {
  ENG_OR_FAIL(e);
  HIPCHK(hipStreamDestroy((hipStream_t)stream));
  return TLSGPU_OK;
}
extern "C" int tlsgpu_stream_sync(tlsgpu_engine* e, void* stream) {
  ENG_OR_FAIL(e);
  HIPCHK(hipStreamSynchronize(pick(e, stream)));
  return TLSGPU_OK;
}
extern "C" int tlsgpu_event_create(tlsgpu_engine* e, void** event) {
  ENG_OR_FAIL(e);
  hipEvent_t ev;
  HIPCHK(hipEventCreate(&ev));
  *event = ev;
  return TLSGPU_OK;
}
extern "C" int tlsgpu_event_destroy(tlsgpu_engine* e, void* event) {
  ENG_OR_FAIL(e);
  HIPCHK(hipEventDestroy((hipEvent_t)event));
  return TLSGPU_OK;
}
extern "C" int tlsgpu_event_record(tlsgpu_engine* e, void* event, void* stream) {
  ENG_OR_FAIL(e);
  HIPCHK(hipEventRecord((hipEvent_t)event, pick(e, stream)));
  return TLSGPU_OK;
}
extern "C" int tlsgpu_event_elapsed_ms(tlsgpu_engine* e, void* start, void* end, float* ms) {
  ENG_OR_FAIL(e);
  HIPCHK(hipEventSynchronize((hipEvent_t)end));
  HIPCHK(hipEventElapsedTime(ms, (hipEvent_t)start, (hipEvent_t)end));
  return TLSGPU_OK;
}
