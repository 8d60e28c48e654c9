// evp_aead.cpp — the drop-in EVP_AEAD ABI (include/tlsgpu_evp.h; LibreSSL
// include/openssl/evp.h:1211-1315): descriptors, the EVP devices, the pinned
// pools, session slabs, key install and scrub, EVP_AEAD_CTX_init / _cleanup /
// _seal / _open over the per-call path (gpu_call), and their stats getters.
//
// The EVP_AEAD functions keep LibreSSL 2.4.1's argument checks and error
// behaviour (crypto/evp/evp_aead.c:50-144, e_aes.c:1372-1510,
// e_chacha20poly1305.c:52-286): same return values, ERR queue entries when a
// LibreSSL libcrypto is present in the process (weak ERR_put_error), zero-fill
// of out[0..max_out_len) and *out_len = 0 on every failure.  The cipher work of
// each call runs on the GPU as a one-record "raw" batch; this library contains
// no CPU cipher path.
#include <sched.h>
#include <unistd.h>

#include "evp_internal.h"

using namespace tg;

// ERR queue hook: resolved only when a LibreSSL libcrypto is in the process.
extern "C" void ERR_put_error(int lib, int func, int reason, const char* file, int line)
    __attribute__((weak));

// Values from LibreSSL include/openssl/evp.h:1327-1491 and err.h:163.
enum {
  ERR_LIB_EVP_ = 6,
  F_AEAD_AES_GCM_INIT = 187, F_AEAD_AES_GCM_OPEN = 188, F_AEAD_AES_GCM_SEAL = 189,
  F_AEAD_CHACHA20_POLY1305_INIT = 192, F_AEAD_CHACHA20_POLY1305_OPEN = 193,
  F_AEAD_CHACHA20_POLY1305_SEAL = 194, F_AEAD_CTX_OPEN = 185, F_AEAD_CTX_SEAL = 186,
  F_EVP_AEAD_CTX_INIT = 180,
  R_BAD_DECRYPT = 100, R_BAD_KEY_LENGTH = 137, R_BUFFER_TOO_SMALL = 155, R_IV_TOO_LARGE = 102,
  R_OUTPUT_ALIASES_INPUT = 172, R_TAG_TOO_LARGE = 171, R_TOO_LARGE = 164,
  R_UNSUPPORTED_KEY_SIZE = 108,
};

static void evp_err(int func, int reason) {
  if (ERR_put_error) ERR_put_error(ERR_LIB_EVP_, func, reason, __FILE__, __LINE__);
}

struct evp_aead_st {
  unsigned char key_len, nonce_len, overhead, max_tag_len;
  int kind;
};

static const evp_aead_st k_aes128 = {16, 12, 16, 16, TLSGPU_AES_128_GCM};
static const evp_aead_st k_aes256 = {32, 12, 16, 16, TLSGPU_AES_256_GCM};
static const evp_aead_st k_cc = {32, 12, 16, 16, TLSGPU_CHACHA20_POLY1305};
static const evp_aead_st k_cc_old = {32, 8, 16, 16, TLSGPU_CHACHA20_POLY1305_OLD};

extern "C" const EVP_AEAD* EVP_aead_aes_128_gcm(void) { return &k_aes128; }
extern "C" const EVP_AEAD* EVP_aead_aes_256_gcm(void) { return &k_aes256; }
extern "C" const EVP_AEAD* EVP_aead_chacha20_poly1305(void) { return &k_cc; }
extern "C" const EVP_AEAD* EVP_aead_chacha20_poly1305_old(void) { return &k_cc_old; }
extern "C" size_t EVP_AEAD_key_length(const EVP_AEAD* a) { return a->key_len; }
extern "C" size_t EVP_AEAD_nonce_length(const EVP_AEAD* a) { return a->nonce_len; }
extern "C" size_t EVP_AEAD_max_overhead(const EVP_AEAD* a) { return a->overhead; }
extern "C" size_t EVP_AEAD_max_tag_len(const EVP_AEAD* a) { return a->max_tag_len; }

// Process-wide engines of the per-call path, one per GPU the EVP surface uses:
// TLSGPU_DEVICE=d pins it to device d; otherwise every visible GPU takes new
// contexts in turn (EVP_AEAD_CTX_init round-robin), so an unchanged server's
// connections spread over the node's GPUs — one SSL per thread
// in the reference's worker model, one context per connection direction.
static std::mutex g_mu;
static tlsgpu_engine* g_engines[kMaxEvpDevices] = {};
static std::atomic<uint32_t> g_evp_rr{0};
static std::atomic<uint64_t> g_evp_dev_calls[kMaxEvpDevices];  // per EVP device
static std::atomic<uint64_t> g_evp_dev_ctx[kMaxEvpDevices];

static const std::vector<int>& evp_devices_locked() {
  // device ordinals, filled once (a function-local static: the queue's
  // load-time constructor may ask before this unit's initialisers have run)
  static std::vector<int> g_evp_devices;
  if (g_evp_devices.empty()) {
    const char* d = getenv("TLSGPU_DEVICE");
    const char* list = getenv("TLSGPU_DEVICES");  // e.g. "0,1,2,3"; a device may repeat
    int count = 0;
    if (list && *list) {
      for (const char* c = list; *c && g_evp_devices.size() < (size_t)kMaxEvpDevices;) {
        char* end = nullptr;
        const long v = strtol(c, &end, 10);
        if (end == c) break;
        g_evp_devices.push_back((int)v);
        c = *end == ',' ? end + 1 : end;
      }
    }
    if (!g_evp_devices.empty()) {
    } else if (d && *d) {
      g_evp_devices.push_back(atoi(d));
    } else if (hipGetDeviceCount(&count) == hipSuccess && count > 0) {
      for (int i = 0; i < count && i < kMaxEvpDevices; i++) g_evp_devices.push_back(i);
    } else {
      g_evp_devices.push_back(0);
    }
  }
  return g_evp_devices;
}

// Engine of the k-th EVP device (created on first use), or nullptr.
tlsgpu_engine* tg::evp_engine(size_t k) {
  std::lock_guard<std::mutex> lk(g_mu);
  const auto& devs = evp_devices_locked();
  if (k >= devs.size()) return nullptr;
  if (!g_engines[k] && tlsgpu_engine_create(devs[k], &g_engines[k]) != TLSGPU_OK)
    g_engines[k] = nullptr;
  return g_engines[k];
}

size_t tg::evp_device_count() {
  std::lock_guard<std::mutex> lk(g_mu);
  return evp_devices_locked().size();
}

// The next device index for a new context (round-robin over the EVP devices).
size_t tg::evp_pick() { return g_evp_rr.fetch_add(1) % evp_device_count(); }

constexpr size_t kImageBytes = sizeof(DevSession) + sizeof(DevGcmTables);
constexpr size_t kImageSlab = 32;
static_assert(kImageBytes % 256 == 0, "session images stay 256-B aligned in a slab");
PinnedPool tg::g_images{kImageBytes, kImageBytes * kImageSlab, true};
PinnedPool tg::g_stage_chunks{kStageChunk, kStageSlab, false};

bool PinnedPool::take(int dev, uint8_t** h, uint8_t** d) {
  if (dev < 0 || dev >= kMaxDev) return false;
  auto& p = per_dev[dev];
  {
    std::lock_guard<std::mutex> lk(p.mu);
    if (!p.free.empty()) {
      *h = p.free.back().first;
      *d = p.free.back().second;
      p.free.pop_back();
      return true;
    }
  }
  // none free: one pinned slab (one hipHostMalloc per slab / chunk takers)
  uint8_t *hs = nullptr, *ds = nullptr;
  if ((keys && hipSetDevice(dev) != hipSuccess) ||
      hipHostMalloc((void**)&hs, slab, hipHostMallocDefault) != hipSuccess)
    return false;
  if (hipHostGetDevicePointer((void**)&ds, hs, 0) != hipSuccess) {
    ds = nullptr;
    if (keys) {
      (void)hipHostFree(hs);
      return false;
    }
  }
  if (keys) memset(hs, 0, slab);
  p.slabs.fetch_add(1, std::memory_order_relaxed);
  {
    std::lock_guard<std::mutex> lk(p.mu);
    for (size_t i = 1; i < slab / chunk; i++)
      p.free.emplace_back(hs + i * chunk, ds ? ds + i * chunk : nullptr);
  }
  *h = hs;
  *d = ds;
  return true;
}
void PinnedPool::give(int dev, uint8_t* h, uint8_t* d) {
  if (keys) explicit_bzero(h, chunk);
  std::lock_guard<std::mutex> lk(per_dev[dev].mu);
  per_dev[dev].free.emplace_back(h, d);
}

// EVP context storage without a device allocation per context (connection
// churn): contexts outside the coalescing queue take a slot of
// per-device slab tables of kSlabSessions sessions, grown on demand; the slot
// is scrubbed on cleanup and reused.
constexpr uint32_t kSlabSessions = 1024;
struct EvpSlab {
  std::mutex mu;
  std::vector<tlsgpu_sessions*> chunks;
  std::vector<std::pair<tlsgpu_sessions*, uint32_t>> free;
};
static EvpSlab g_slabs[kMaxEvpDevices];

static bool slab_take(size_t dk, tlsgpu_engine* e, tlsgpu_sessions** t, uint32_t* slot) {
  EvpSlab& sl = g_slabs[dk];
  std::lock_guard<std::mutex> lk(sl.mu);
  if (sl.free.empty()) {
    tlsgpu_sessions* c = nullptr;
    if (tlsgpu_sessions_create(e, kSlabSessions, &c) != TLSGPU_OK) return false;
    sl.chunks.push_back(c);
    for (uint32_t i = kSlabSessions; i-- > 0;) sl.free.emplace_back(c, i);
  }
  *t = sl.free.back().first;
  *slot = sl.free.back().second;
  sl.free.pop_back();
  return true;
}

void tg::slab_give(size_t dk, tlsgpu_sessions* t, uint32_t slot) {
  EvpSlab& sl = g_slabs[dk];
  std::lock_guard<std::mutex> lk(sl.mu);
  sl.free.emplace_back(t, slot);
}

// Give a context's session slot back to its queue pool or slab.
static void release_slot(AeadState* st) {
  if (st->batcher) evp_queue_give_session(st->batcher, st->slot);
  else slab_give(st->evp_dev, st->sess, st->slot);
}

// Per-thread staging for one call: pinned host + device buffer and a stream
// (calls on one ctx may run concurrently from several threads,
// evp.h:1273-1274).  Layout [RawJob | nonce | ad | in | status | out], so one
// H2D covers the job up to its preset status and one D2H status and output.
// Threads share kCallStreams streams per process (more streams than the
// hardware queues, GPU_MAX_HW_QUEUES = 4, cost 3x in call rate at 64 threads:
// tools/hip_latency); each thread waits on its own event, i.e. on its own
// work and what was queued before it on that stream.
constexpr int kCallStreams = 4;
static hipStream_t g_call_streams[kMaxDev][kCallStreams];
static std::once_flag g_call_streams_once[kMaxDev];
static bool g_call_streams_ok[kMaxDev];
static std::atomic<uint32_t> g_call_thread_seq{0};

bool Staging::ensure(int dev, size_t bytes, bool dev_buf) {
  if (dev < 0 || dev >= kMaxDev || hipSetDevice(dev) != hipSuccess) return false;
  if (!stream) {
    std::call_once(g_call_streams_once[dev], [dev] {
      bool ok = true;
      for (hipStream_t& cs : g_call_streams[dev])
        ok &= hipStreamCreateWithFlags(&cs, hipStreamNonBlocking) == hipSuccess;
      g_call_streams_ok[dev] = ok;
    });
    if (!g_call_streams_ok[dev] ||
        hipEventCreateWithFlags(&done, hipEventDisableTiming) != hipSuccess)
      return false;
    stream = g_call_streams[dev][g_call_thread_seq.fetch_add(1) % kCallStreams];
  }
  device = dev;
  if (cap < bytes) {
    release_host();  // this thread's calls are synchronous: nothing in flight
    if (bytes <= kStageChunk) {
      if (!g_stage_chunks.take(dev, &h_buf, &h_dev)) return false;
      cap = kStageChunk;
    } else {
      const size_t want = (bytes + kStageChunk - 1) & ~(kStageChunk - 1);
      if (hipHostMalloc((void**)&h_buf, want, hipHostMallocDefault) != hipSuccess) {
        h_buf = nullptr;
        return false;
      }
      if (hipHostGetDevicePointer((void**)&h_dev, h_buf, 0) != hipSuccess) h_dev = nullptr;
      cap = want;
    }
  }
  if (dev_buf && dcap < bytes) {
    if (d_buf) (void)hipFree(d_buf);
    d_buf = nullptr;
    dcap = 0;
    const size_t want = (bytes + kStageChunk - 1) & ~(kStageChunk - 1);
    if (hipMalloc(&d_buf, want) != hipSuccess) {
      d_buf = nullptr;
      return false;
    }
    dcap = want;
  }
  return true;
}

// The event of a slot (created on first use).
static hipEvent_t slot_event(tlsgpu_sessions* t, uint32_t slot) {
  std::lock_guard<std::mutex> lk(t->mu);
  if (t->slot_ev.size() < t->capacity) t->slot_ev.resize(t->capacity, nullptr);
  hipEvent_t& ev = t->slot_ev[slot];
  if (!ev && hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) ev = nullptr;
  return ev;
}

// One session install for an EVP context on the calling thread's call stream,
// asynchronous (round 3): the parameters travel as a kernel argument (no
// staging copy to wait for), the install is ordered after the slot's previous
// scrub by the slot's event and records it again when done; the context's
// first call waits for that event on the device (gpu_call_impl).  A
// connection's key install at ChangeCipherSpec (t1_enc.c:444-495) then costs
// no device round trip of its own.
// Round 5 (hygiene): the image is built on the
// calling thread (session_host.cpp: key schedule, H, the GHASH power tables —
// the ~25 µs of one wave install_session_arg spent) into a pinned key area,
// and one short kernel copies it into the slot: no key material in kernel
// arguments, and the area is zeroed once its copy has finished
// (sweep_key_areas after the thread's next synchronised call, or when the
// area is reused).  TLSGPU_EVP_DEVICE_INSTALL=1 keeps the device install.
// A host without AES-NI or PCLMUL builds no host image (session_host.cpp: no
// table-driven key schedule on the CPU) and takes the device install too.
static const bool g_device_install = env_on("TLSGPU_EVP_DEVICE_INSTALL") || !host_crypto_ok();

static int install_one(tlsgpu_sessions* t, uint32_t slot, const tlsgpu_session_params& p,
                       hipEvent_t* installed) {
  if (!valid_params(p) || slot >= t->capacity) return fail(TLSGPU_EINVAL, "bad session");
  Staging* stg = stage_for(t->eng->device);
  if (!stg || !stg->ensure(t->eng->device, 16)) return fail(TLSGPU_ENOMEM, "staging");
  const hipEvent_t ev = slot_event(t, slot);  // on the slot's device (ensure set it)
  if (!ev) return fail(TLSGPU_EHIP, "slot event");
  bool ok;
  if (g_device_install) {
    ok = hipStreamWaitEvent(stg->stream, ev, 0) == hipSuccess &&
         launch_session_install_arg(t->d_sess, t->d_gcm, p, slot, stg->stream) == 0 &&
         hipEventRecord(ev, stg->stream) == hipSuccess;
  } else {
    Staging::KeyArea* ka = stg->take_key_area();
    if (!ka) return fail(TLSGPU_ENOMEM, "key area");
    auto* img_s = reinterpret_cast<DevSession*>(ka->h);
    auto* img_t = reinterpret_cast<DevGcmTables*>(ka->h + sizeof(DevSession));
    const bool tables = host_session_image(p, img_s, img_t);
    ka->dirty = true;
    ok = hipStreamWaitEvent(stg->stream, ev, 0) == hipSuccess &&
         launch_upload_session(ka->dev, t->d_sess + slot, t->d_gcm + slot,
                               tables ? kGcmTableUploadBytes : 0u, stg->stream) == 0 &&
         hipEventRecord(ka->ev, stg->stream) == hipSuccess &&
         hipEventRecord(ev, stg->stream) == hipSuccess;
  }
  if (!ok) return fail(TLSGPU_EHIP, "session install: %s", hipGetErrorString(hipGetLastError()));
  *installed = ev;
  std::lock_guard<std::mutex> lk(t->mu);
  t->kinds[slot] = p.aead;
  t->tag_lens[slot] = (uint8_t)(p.tag_len ? p.tag_len : 16);
  t->have[p.aead] = true;
  return TLSGPU_OK;
}

// Zero a session slot's key material on the calling thread's stream without
// waiting: ordered after the slot's install by the slot's event, which then
// orders the slot's next install after the scrub.
static void scrub_slot(tlsgpu_sessions* t, uint32_t slot) {
  Staging* stg = stage_for(t->eng->device);
  const bool staged = stg && stg->ensure(t->eng->device, 16);
  const hipEvent_t ev = staged ? slot_event(t, slot) : nullptr;
  // after the slot's install (a context cleaned up before any call, from
  // another thread, may still have its install queued on another stream)
  if (ev && hipStreamWaitEvent(stg->stream, ev, 0) == hipSuccess &&
      launch_scrub_session(t->d_sess + slot, t->d_gcm + slot, stg->stream) == 0 &&
      hipEventRecord(ev, stg->stream) == hipSuccess) {
    stg->sweep_key_areas();
    return;
  }
  (void)hipSetDevice(t->eng->device);  // fall back to the synchronous form
  (void)hipDeviceSynchronize();
  (void)hipMemset(t->d_sess + slot, 0, sizeof(DevSession));
  (void)hipMemset(t->d_gcm + slot, 0, sizeof(DevGcmTables));
}

// A context whose calls can take the doorbell defers its install to its first
// call (TLSGPU_EVP_DEFERRED_INSTALL=0: never).
static const bool g_deferred_install = env_not_off("TLSGPU_EVP_DEFERRED_INSTALL");
static bool deferred_install_ok(int kind) {
  return g_deferred_install && !g_device_install && evp_zerocopy() && doorbell_enabled() &&
         (kind == TLSGPU_AES_128_GCM || kind == TLSGPU_AES_256_GCM ||
          kind == TLSGPU_CHACHA20_POLY1305 || kind == TLSGPU_CHACHA20_POLY1305_OLD);
}

static int defer_install(AeadState* st, const tlsgpu_session_params& p) {
  tlsgpu_sessions* t = st->sess;
  if (!valid_params(p) || st->slot >= t->capacity) return fail(TLSGPU_EINVAL, "bad session");
  if (hipSetDevice(t->eng->device) != hipSuccess) return fail(TLSGPU_EHIP, "set device");
  st->slot_ev = slot_event(t, st->slot);  // its previous owner's scrub, if launched
  if (!st->slot_ev) return fail(TLSGPU_EHIP, "slot event");
  if (!g_images.take(t->eng->device, &st->img_h, &st->img_d)) return fail(TLSGPU_ENOMEM, "session image");
  // compact (round 6): the doorbell install reads m[8] = H^e of each Shoup
  // table and expands the rest on the device; a launched first call
  // completes the image on the host before its upload
  st->img_tables = host_session_image(p, reinterpret_cast<DevSession*>(st->img_h),
                                      reinterpret_cast<DevGcmTables*>(st->img_h + sizeof(DevSession)),
                                      kGcmTableUploadBytes > offsetof(DevGcmTables, bsrk), true);
  st->img_compact = st->img_tables;
  st->installed = st->slot_ev;
  st->install_pending.store(false, std::memory_order_release);  // nothing queued
  st->image.store(1, std::memory_order_release);
  std::lock_guard<std::mutex> lk(t->mu);
  t->kinds[st->slot] = p.aead;
  t->tag_lens[st->slot] = (uint8_t)(p.tag_len ? p.tag_len : 16);
  t->have[p.aead] = true;
  return TLSGPU_OK;
}

extern "C" int EVP_AEAD_CTX_init(EVP_AEAD_CTX* ctx, const EVP_AEAD* aead, const unsigned char* key,
                                 size_t key_len, size_t tag_len, ENGINE* impl) {
  (void)impl;
  ctx->aead = aead;
  ctx->aead_state = nullptr;
  if (key_len != aead->key_len) {  // evp_aead.c:55-58
    evp_err(F_EVP_AEAD_CTX_INIT, R_UNSUPPORTED_KEY_SIZE);
    return 0;
  }
  bool gcm = aead->kind == TLSGPU_AES_128_GCM || aead->kind == TLSGPU_AES_256_GCM;
  if (tag_len == EVP_AEAD_DEFAULT_TAG_LENGTH) tag_len = 16;
  if (tag_len > 16) {  // e_aes.c:1388-1391, e_chacha20poly1305.c:62-65
    evp_err(gcm ? F_AEAD_AES_GCM_INIT : F_AEAD_CHACHA20_POLY1305_INIT,
            gcm ? R_TAG_TOO_LARGE : R_TOO_LARGE);
    return 0;
  }
  const size_t dk = evp_pick();  // this context's GPU (round-robin over the EVP devices)
  tlsgpu_engine* e = evp_engine(dk);
  if (!e) return 0;
  auto* st = new (std::nothrow) AeadState();
  if (!st) return 0;
  st->kind = aead->kind;
  static std::atomic<uint32_t> g_key_ids{0};
  do st->key_id = g_key_ids.fetch_add(1, std::memory_order_relaxed) + 1;
  while (st->key_id == 0);  // 0 means "no key" to the server's table cache
  st->tag_len = (unsigned)tag_len;
  st->evp_dev = (uint32_t)dk;
  st->batcher = evp_queue_take_session(dk, &st->sess, &st->slot);
  if (!st->batcher) evp_sweep_scrubs_for(dk);  // answered cleanup scrubs: slots back first
  if (!st->batcher && !slab_take(dk, e, &st->sess, &st->slot)) {
    delete st;
    return 0;
  }
  tlsgpu_session_params p;
  memset(&p, 0, sizeof(p));
  p.aead = aead->kind;
  p.key_len = (uint32_t)key_len;
  memcpy(p.key, key, key_len);
  p.tag_len = (uint32_t)tag_len;
  p.version = 0x0303;
  // deferred (round 5) where the first call can take the doorbell: nothing is
  // launched here, the first call installs the host-built image; otherwise on
  // this thread's call stream, not waited for: installs of concurrent threads
  // overlap, and the context's first call is ordered after it
  const int rc = (!st->batcher && deferred_install_ok(aead->kind)) ? defer_install(st, p)
                                                                   : install_one(st->sess, st->slot, p, &st->installed);
  memset(&p, 0, sizeof(p));
  if (rc != TLSGPU_OK) {
    if (st->img_h) g_images.give(st->sess->eng->device, st->img_h, st->img_d);
    release_slot(st);
    delete st;
    return 0;
  }
  g_evp_dev_ctx[dk].fetch_add(1, std::memory_order_relaxed);
  ctx->aead_state = st;
  return 1;
}

static const bool g_async_scrub = env_not_off("TLSGPU_EVP_ASYNC_SCRUB");
extern "C" void EVP_AEAD_CTX_cleanup(EVP_AEAD_CTX* ctx) {
  if (ctx->aead == nullptr) return;
  auto* st = (AeadState*)ctx->aead_state;
  if (st) {
    const int img = st->image.load(std::memory_order_acquire);
    if (img == kImagePoisoned) {
      // an install job that never answered may still copy the image into the
      // slot: leak both (never reused, as stg->abandon() leaks staging) —
      // no scrub either, its synchronous fallback would wait on that device
      delete st;
      ctx->aead_state = nullptr;
      ctx->aead = nullptr;
      return;
    }
    if (img == 1) {
      // deferred and never called: no key material reached the device
      g_images.give(st->sess->eng->device, st->img_h, st->img_d);
    } else if (g_async_scrub && doorbell_scrub_async(st)) {
      // posted: the slot goes back once the server has answered (sweep_scrubs)
      delete st;
      ctx->aead_state = nullptr;
      ctx->aead = nullptr;
      return;
    } else if (!doorbell_scrub(st)) {
      // scrub the device key material before the slot is reused
      // (explicit_bzero analogue, e_aes.c:1415-1422), on this thread's stream
      scrub_slot(st->sess, st->slot);
    }
    release_slot(st);
    delete st;
  }
  ctx->aead_state = nullptr;
  ctx->aead = nullptr;
}

// Test support (include/tlsgpu.h): where a live EVP context's key material
// sits, and the bytes of a session slot once every queued install / scrub of
// that slot has finished — so a test can check that EVP_AEAD_CTX_cleanup's
// asynchronous scrub really zeroes the device copy (e_aes.c:1415-1422).
extern "C" int tlsgpu_evp_context_slot(const EVP_AEAD_CTX* ctx, tlsgpu_sessions** sessions,
                                       uint32_t* slot) {
  const auto* st = ctx ? (const AeadState*)ctx->aead_state : nullptr;
  if (!st || !sessions || !slot) return fail(TLSGPU_EINVAL, "no live EVP context");
  *sessions = st->sess;
  *slot = st->slot;
  return TLSGPU_OK;
}

extern "C" int tlsgpu_sessions_debug_read(tlsgpu_sessions* t, uint32_t slot, uint8_t* out,
                                          size_t n) {
  if (!t || !out || slot >= t->capacity || n > sizeof(DevSession) + sizeof(DevGcmTables))
    return fail(TLSGPU_EINVAL, "bad slot read");
  evp_wait_scrub_of(t, slot);  // an asynchronous cleanup scrub of this slot (round 6)
  HIPCHK(hipSetDevice(t->eng->device));
  if (const hipEvent_t ev = slot_event(t, slot)) HIPCHK(hipEventSynchronize(ev));
  const size_t a = std::min(n, sizeof(DevSession));
  HIPCHK(hipMemcpy(out, t->d_sess + slot, a, hipMemcpyDeviceToHost));
  if (n > a) HIPCHK(hipMemcpy(out + a, t->d_gcm + slot, n - a, hipMemcpyDeviceToHost));
  return TLSGPU_OK;
}

static int check_alias(const unsigned char* in, size_t in_len, const unsigned char* out) {
  if (out <= in) return 1;
  if (in + in_len <= out) return 1;
  return 0;
}

// EVP calls whose cipher work ran on the GPU (tlsgpu_evp_call_stats), and per
// EVP device (tlsgpu_evp_device_stats).
static std::atomic<uint64_t> g_evp_calls[2];  // [0] open, [1] seal

extern "C" int tlsgpu_evp_call_stats(uint64_t* seal_calls, uint64_t* open_calls) {
  if (seal_calls) *seal_calls = g_evp_calls[1].load();
  if (open_calls) *open_calls = g_evp_calls[0].load();
  return TLSGPU_OK;
}

extern "C" int tlsgpu_evp_device_stats(uint32_t k, int* device, uint64_t* contexts,
                                       uint64_t* calls) {
  if (k >= evp_device_count()) return fail(TLSGPU_ERANGE, "EVP device %u of %zu", k,
                                           evp_device_count());
  if (device) {
    std::lock_guard<std::mutex> lk(g_mu);
    *device = evp_devices_locked()[k];
  }
  if (contexts) *contexts = g_evp_dev_ctx[k].load();
  if (calls) *calls = g_evp_dev_calls[k].load();
  return TLSGPU_OK;
}

extern "C" uint32_t tlsgpu_evp_device_count(void) { return (uint32_t)evp_device_count(); }

// Test hook (TLSGPU_TEST_FAIL_INSTALLS=k): the first k calls that claim a
// deferred install fail before posting it (waiters must re-claim).
static std::atomic<int> g_test_fail_installs{[] {
  const char* v = getenv("TLSGPU_TEST_FAIL_INSTALLS");
  return v ? atoi(v) : 0;
}()};

// Wait for a per-call event: blocking (hipEventSynchronize), or with
// TLSGPU_EVP_SPIN=1 by polling hipEventQuery.  The probe had a host spin on
// the kernel's own completion word 5-6 µs faster than the blocking wait
// (tools/doorbell_probe.hip: 9.6 vs 15.4 µs for a 1,400-B job), but polling
// the event measured no better in the library (profiles/r04h_doorbell_bench:
// 36.1 vs 37.6 K calls/s at 1 thread, 42.0 vs 45.2 K at 64) and burns a core
// per waiting thread, so the blocking wait stays the default.
static const bool g_evp_spin = env_on("TLSGPU_EVP_SPIN");
static bool event_spin(hipEvent_t ev) {
  if (!g_evp_spin) return hipEventSynchronize(ev) == hipSuccess;
  for (uint64_t spins = 1;; spins++) {
    const hipError_t q = hipEventQuery(ev);
    if (q == hipSuccess) return true;
    if (q != hipErrorNotReady) return false;
    __builtin_ia32_pause();
    if ((spins & 255) == 0 && spins > 4096) sched_yield();  // a long job: let others run
  }
}

// The steps of one EVP call on the calling thread's staging (gpu_call_impl).
namespace {
struct CallArgs {  // EVP_AEAD_CTX_seal / _open's arguments
  const AeadState* st;
  bool seal;
  unsigned char* out;
  size_t *out_len, max_out_len;
  const unsigned char *nonce, *in, *ad;
  size_t nonce_len, in_len, ad_len;
};
// The call's job in the staging buffer: [RawJob | nonce | ad | in | status | out]
struct CallJob {
  Staging* stg;
  uint8_t *h, *d;  // the buffer as the host / the device addresses it
  bool zc;
  size_t o_status, o_out;
};

// a deferred install (EVP_AEAD_CTX_init, round 5): one caller installs the
// image with its call, concurrent first callers wait for it; a failed call
// leaves the image waiting (1) for the next caller — a waiter that sees it
// back at 1 claims it itself.  Once the image's address has
// reached the device (a posted doorbell job, a queued upload) a failure
// poisons the context instead (3, kImagePoisoned): the job may still run, so
// the image buffer and the slot are never handed to anyone else, and every
// later call fails (a doorbell timeout).
struct InstallClaim {
  const AeadState* st;
  bool active = false;
  bool posted = false;  // the device may read the image from now on
  ~InstallClaim() {
    if (active) st->image.store(posted ? kImagePoisoned : 1, std::memory_order_release);
  }
  void done() {  // on the device: the image buffer goes back, zeroed
    active = false;
    st->image.store(0, std::memory_order_release);
    g_images.give(st->sess->eng->device, st->img_h, st->img_d);
  }
};

// Claim the context's deferred install, or wait for the caller that holds it.
// false: the call fails.
bool claim_install(const AeadState* st, InstallClaim& claim) {
  if (st->image.load(std::memory_order_acquire) == 0) return true;
  for (uint64_t spins = 1;; spins++) {
    int expect = 1;
    if (st->image.compare_exchange_strong(expect, 2, std::memory_order_acq_rel)) {
      claim.active = true;
      // the slot's previous owner's scrub, if it went through a stream
      if (hipEventQuery(st->slot_ev) != hipSuccess &&
          hipEventSynchronize(st->slot_ev) != hipSuccess)
        return false;
      if (g_test_fail_installs.load(std::memory_order_relaxed) > 0 &&
          g_test_fail_installs.fetch_sub(1) > 0) {  // test hook: the claimer fails
        usleep(20000);  // with the other first callers waiting on it
        return false;
      }
      return true;
    }
    if (expect == 0) return true;               // installed by the caller that claimed it
    if (expect == kImagePoisoned) return false;
    // 2: another caller is installing right now
    __builtin_ia32_pause();
    if ((spins & 255) == 0) sched_yield();
    if (spins > (1ull << 34)) return false;
  }
}

// Lay the job out in this thread's staging and fill it.
bool stage_job(const CallArgs& c, CallJob& jb) {
  const AeadState* st = c.st;
  auto al = [](size_t v) { return (v + 15) & ~(size_t)15; };
  const size_t out_bytes = c.seal ? c.in_len + st->tag_len : std::max(c.max_out_len, c.in_len);
  const size_t o_nonce = al(sizeof(RawJob)), o_ad = o_nonce + al(c.nonce_len);
  const size_t o_in = o_ad + al(c.ad_len), o_status = o_in + al(c.in_len);
  const size_t o_out = o_status + 16, total = o_out + al(out_bytes + 1);
  tlsgpu_engine* e = st->sess->eng;
  Staging* stg = stage_for(e->device);
  if (!stg || !stg->ensure(e->device, total)) return false;
  // zero-copy (round 3, default): the kernel reads the job from and writes its
  // status and output to the pinned staging buffer itself — no H2D / D2H
  // launches around a one-record batch; TLSGPU_EVP_ZEROCOPY=0 stages through HBM
  const bool zc = evp_zerocopy() && stg->h_dev;
  if (!zc && !stg->ensure(e->device, total, true)) return false;
  uint8_t* d = zc ? stg->h_dev : stg->d_buf;
  uint8_t* h = stg->h_buf;
  hipStream_t s = stg->stream;
  if (st->install_pending.load(std::memory_order_acquire) &&
      hipStreamWaitEvent(s, st->installed, 0) != hipSuccess)
    return false;
  RawJob* j = reinterpret_cast<RawJob*>(h);
  j->in = (uint64_t)(d + o_in);
  j->out = (uint64_t)(d + o_out);
  j->nonce = (uint64_t)(d + o_nonce);
  j->aad = (uint64_t)(d + o_ad);
  j->in_len = (uint32_t)c.in_len;
  j->nonce_len = (uint32_t)c.nonce_len;
  j->aad_len = (uint32_t)c.ad_len;
  j->session = st->slot;
  j->max_out = c.max_out_len;
  if (c.nonce_len) memcpy(h + o_nonce, c.nonce, c.nonce_len);
  if (c.ad_len) memcpy(h + o_ad, c.ad, c.ad_len);
  if (c.in_len) memcpy(h + o_in, c.in, c.in_len);
  // a job the kernel rejects keeps this status (never a stale one)
  *reinterpret_cast<int32_t*>(h + o_status) = TLSGPU_REC_PUBLIC_INVALID;
  if (!zc && hipMemcpyAsync(d, h, o_status + 4, hipMemcpyHostToDevice, s) != hipSuccess)
    return false;
  jb = {stg, h, d, zc, o_status, o_out};
  return true;
}

// doorbell (zero-copy AES-GCM and ChaCha20-Poly1305 calls): post the job to a
// resident server workgroup instead of launching; the staging buffer is the
// job's memory.  1: served; 0: not posted, or never to be served (shutdown) —
// take the launched path; -1: failure.
int post_job(const CallArgs& c, const CallJob& jb, InstallClaim& claim) {
  const AeadState* st = c.st;
  EvpServer* sv = evp_server(st->evp_dev, st->sess->eng);
  uint32_t* seq = nullptr;
  DoorbellSlot* slot = sv ? thread_slot(sv, st->evp_dev, &seq) : nullptr;
  // a context's first call, its key install still queued, takes the
  // launched path (ordered after the install on the device, no host
  // wait): waiting for the install here halved connection churn at 16
  // threads (profiles/r04l_doorbell_bench.jsonl: 17.7 vs 43.7 K/s)
  if (!slot || st->install_pending.load(std::memory_order_acquire)) return 0;
  // the job travels in the slot (one wave load brings it to the server),
  // nonce and AAD inline when they fit
  // (an installing call carries the image's address in `inl` instead)
  const bool inl = !claim.active && c.nonce_len + c.ad_len <= kDoorbellInline;
  const uint32_t kop = st->kind == TLSGPU_AES_128_GCM   ? 10u
                       : st->kind == TLSGPU_AES_256_GCM ? 14u
                       : st->kind == TLSGPU_CHACHA20_POLY1305 ? 20u
                                                              : 21u;  // draft ChaCha
  doorbell_fill(slot, st,
                (uint32_t)(c.seal ? 1 : 0) | (kop << 8) | (inl ? 1u << 16 : 0u) |
                    (claim.active ? kDoorbellOpInstall : 0u) |
                    (claim.active && st->img_tables ? kDoorbellOpInstallTables : 0u),
                jb.d + jb.o_status);
  memcpy(&slot->job, jb.h, sizeof(RawJob));
  if (inl) {
    if (c.nonce_len) memcpy(slot->inl, c.nonce, c.nonce_len);
    if (c.ad_len) memcpy(slot->inl + c.nonce_len, c.ad, c.ad_len);
  } else if (claim.active) {
    const uint64_t img = (uint64_t)st->img_d;
    memcpy(slot->inl, &img, sizeof(img));
  }
  uint64_t t0 = 0;
  const int pr = doorbell_post_wait(sv, slot, seq, st->evp_dev, jb.stg, &t0);
  if (pr == -2) claim.posted = true;  // unanswered: the job may still copy the image
  if (pr <= 0) return pr < 0 ? -1 : 0;
  if (claim.active) claim.done();
  doorbell_served(sv, slot, t0);
  return 1;
}

// The launched path: one raw kernel on the thread's call stream, waited for.
bool launch_job(const CallArgs& c, const CallJob& jb, InstallClaim& claim) {
  const AeadState* st = c.st;
  Staging* stg = jb.stg;
  hipStream_t s = stg->stream;
  BatchArgs a = {};
  a.sessions = st->sess->d_sess;
  a.gcm_tables = st->sess->d_gcm;
  a.descs = jb.d;
  a.n = 1;
  a.records_per_group = 1;
  a.status = reinterpret_cast<int32_t*>(jb.d + jb.o_status);
  a.n_sessions = st->sess->capacity;
  // a deferred install on the launched path: one upload kernel ahead of the job
  if (claim.active) {
    if (hipStreamWaitEvent(s, st->slot_ev, 0) != hipSuccess) return false;
    if (st->img_compact)  // the upload copies whole Shoup tables
      host_image_complete(reinterpret_cast<DevGcmTables*>(st->img_h + sizeof(DevSession)));
    claim.posted = true;  // queued from here on, whatever fails after it
    if (launch_upload_session(st->img_d, st->sess->d_sess + st->slot, st->sess->d_gcm + st->slot,
                              st->img_tables ? kGcmTableUploadBytes : 0u, s) != 0)
      return false;
  }
  const bool gcm = st->kind == TLSGPU_AES_128_GCM || st->kind == TLSGPU_AES_256_GCM;
  int rc = gcm ? launch_gcm(a, c.seal, true, st->kind == TLSGPU_AES_128_GCM ? 10 : 14, 1, s)
               : launch_chacha(a, c.seal, true, true, true, s);
  if (rc) return false;
  // success writes at most in_len + tag (seal) / in_len - tag (open) bytes
  const size_t back = c.seal ? c.in_len + st->tag_len : std::min(c.max_out_len, c.in_len);
  if ((!jb.zc && hipMemcpyAsync(jb.h + jb.o_status, jb.d + jb.o_status,
                                jb.o_out - jb.o_status + back, hipMemcpyDeviceToHost,
                                s) != hipSuccess) ||
      hipEventRecord(stg->done, s) != hipSuccess || !event_spin(stg->done))
    return false;
  st->install_pending.store(false, std::memory_order_release);  // done before this call's work
  if (claim.active) claim.done();
  if (stg->any_dirty_key_area()) stg->sweep_key_areas();  // this context's image, copied by now
  return true;
}

// The job's status, and its output to the caller's buffer.
int finish_call(const CallArgs& c, const CallJob& jb) {
  const int32_t status = *reinterpret_cast<const int32_t*>(jb.h + jb.o_status);
  if (status < 0) {  // the kernel's zero-fill of max_out_len bytes (evp_aead.c:137-143)
    if (c.max_out_len) memset(c.out, 0, c.max_out_len);
    return 0;
  }
  if (status) memcpy(c.out, jb.h + jb.o_out, (size_t)status);
  *c.out_len = (size_t)status;
  return 1;
}
}  // namespace

static int gpu_call_impl(const AeadState* st, bool seal, unsigned char* out, size_t* out_len,
                         size_t max_out_len, const unsigned char* nonce, size_t nonce_len,
                         const unsigned char* in, size_t in_len, const unsigned char* ad,
                         size_t ad_len) {
  // the context's key install (EVP_AEAD_CTX_init does not wait for it)
  const bool wait_install = st->install_pending.load(std::memory_order_acquire);
  if (st->batcher) {  // pooled context: join the coalescing queue (large jobs run alone)
    if (wait_install) {
      if (hipEventSynchronize(st->installed) != hipSuccess) return -1;
      st->install_pending.store(false, std::memory_order_release);
    }
    int r = evp_queue_call(st->batcher, st, seal, out, out_len, max_out_len, nonce, nonce_len,
                           in, in_len, ad, ad_len);
    if (r != -2) return r;
  }
  const CallArgs c = {st, seal, out, out_len, max_out_len, nonce, in, ad, nonce_len, in_len, ad_len};
  InstallClaim claim{st};
  CallJob jb;
  if (!claim_install(st, claim) || !stage_job(c, jb)) return -1;
  const int posted = jb.zc ? post_job(c, jb, claim) : 0;
  if (posted < 0 || (posted == 0 && !launch_job(c, jb, claim))) return -1;
  return finish_call(c, jb);
}

// One EVP call on the GPU: 1 = success, 0 = authentication failure / rejected
// by the kernel (output zero-filled), -1 = runtime failure.
static int gpu_call(const AeadState* st, bool seal, unsigned char* out, size_t* out_len,
                    size_t max_out_len, const unsigned char* nonce, size_t nonce_len,
                    const unsigned char* in, size_t in_len, const unsigned char* ad,
                    size_t ad_len) {
  int r = gpu_call_impl(st, seal, out, out_len, max_out_len, nonce, nonce_len, in, in_len, ad,
                        ad_len);
  if (r >= 0) {
    g_evp_calls[seal ? 1 : 0].fetch_add(1, std::memory_order_relaxed);
    g_evp_dev_calls[st->evp_dev].fetch_add(1, std::memory_order_relaxed);
  }
  return r;
}

extern "C" int EVP_AEAD_CTX_seal(const EVP_AEAD_CTX* ctx, unsigned char* out, size_t* out_len,
                                 size_t max_out_len, const unsigned char* nonce, size_t nonce_len,
                                 const unsigned char* in, size_t in_len, const unsigned char* ad,
                                 size_t ad_len) {
  const AeadState* st = (const AeadState*)ctx->aead_state;
  size_t possible_out_len = in_len + ctx->aead->overhead;
  bool gcm = ctx->aead->kind == TLSGPU_AES_128_GCM || ctx->aead->kind == TLSGPU_AES_256_GCM;
  int r;
  if (possible_out_len < in_len) {  // evp_aead.c:96-100
    evp_err(F_AEAD_CTX_SEAL, R_TOO_LARGE);
    goto error;
  }
  if (!check_alias(in, in_len, out)) {
    evp_err(F_AEAD_CTX_SEAL, R_OUTPUT_ALIASES_INPUT);
    goto error;
  }
  if (!st) goto error;
  if (gcm) {
    if (max_out_len < in_len + st->tag_len) {  // e_aes.c:1434-1437
      evp_err(F_AEAD_AES_GCM_SEAL, R_BUFFER_TOO_SMALL);
      goto error;
    }
    if (in_len > TLSGPU_MAX_RECORD * 64ull || ad_len > TLSGPU_MAX_RECORD * 64ull) goto error;
  } else {
    if ((uint64_t)in_len >= (1ull << 32) * 64 - 64) {  // e_chacha20poly1305.c:144-147
      evp_err(F_AEAD_CHACHA20_POLY1305_SEAL, R_TOO_LARGE);
      goto error;
    }
    if (max_out_len < in_len + st->tag_len) {
      evp_err(F_AEAD_CHACHA20_POLY1305_SEAL, R_BUFFER_TOO_SMALL);
      goto error;
    }
    if (nonce_len != ctx->aead->nonce_len) {
      evp_err(F_AEAD_CHACHA20_POLY1305_SEAL, R_IV_TOO_LARGE);
      goto error;
    }
  }
  r = gpu_call(st, true, out, out_len, max_out_len, nonce, nonce_len, in, in_len, ad, ad_len);
  if (r == 1) return 1;
error:
  memset(out, 0, max_out_len);  // evp_aead.c:113-118
  *out_len = 0;
  return 0;
}

extern "C" int EVP_AEAD_CTX_open(const EVP_AEAD_CTX* ctx, unsigned char* out, size_t* out_len,
                                 size_t max_out_len, const unsigned char* nonce, size_t nonce_len,
                                 const unsigned char* in, size_t in_len, const unsigned char* ad,
                                 size_t ad_len) {
  const AeadState* st = (const AeadState*)ctx->aead_state;
  bool gcm = ctx->aead->kind == TLSGPU_AES_128_GCM || ctx->aead->kind == TLSGPU_AES_256_GCM;
  int r;
  if (!check_alias(in, in_len, out)) {
    evp_err(F_AEAD_CTX_OPEN, R_OUTPUT_ALIASES_INPUT);
    goto error;
  }
  if (!st) goto error;
  if (gcm) {
    if (in_len < st->tag_len) {  // e_aes.c:1473-1476
      evp_err(F_AEAD_AES_GCM_OPEN, R_BAD_DECRYPT);
      goto error;
    }
    if (max_out_len < in_len - st->tag_len) {
      evp_err(F_AEAD_AES_GCM_OPEN, R_BUFFER_TOO_SMALL);
      goto error;
    }
    if (in_len > TLSGPU_MAX_RECORD * 64ull || ad_len > TLSGPU_MAX_RECORD * 64ull) goto error;
  } else {
    if (in_len < st->tag_len) {  // e_chacha20poly1305.c:223-226
      evp_err(F_AEAD_CHACHA20_POLY1305_OPEN, R_BAD_DECRYPT);
      goto error;
    }
    if ((uint64_t)in_len >= (1ull << 32) * 64 - 64) {
      evp_err(F_AEAD_CHACHA20_POLY1305_OPEN, R_TOO_LARGE);
      goto error;
    }
    if (nonce_len != ctx->aead->nonce_len) {
      evp_err(F_AEAD_CHACHA20_POLY1305_OPEN, R_IV_TOO_LARGE);
      goto error;
    }
    if (max_out_len < in_len - st->tag_len) {
      evp_err(F_AEAD_CHACHA20_POLY1305_OPEN, R_BUFFER_TOO_SMALL);
      goto error;
    }
  }
  r = gpu_call(st, false, out, out_len, max_out_len, nonce, nonce_len, in, in_len, ad, ad_len);
  if (r == 1) return 1;
  evp_err(gcm ? F_AEAD_AES_GCM_OPEN : F_AEAD_CHACHA20_POLY1305_OPEN, R_BAD_DECRYPT);
error:
  memset(out, 0, max_out_len);  // evp_aead.c:137-143
  *out_len = 0;
  return 0;
}
