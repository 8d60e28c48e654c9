// evp_internal.h — what the EVP units (evp_*.cpp) share: the context state, the
// pinned pools, per-thread staging and each unit's few entry points.  Never
// included by a .hip file.
#pragma once
#include "host_internal.h"

namespace tg {

constexpr int kMaxEvpDevices = 16;
constexpr int kMaxDev = 64;  // device ordinals a thread may stage for

struct EvpBatcher;  // evp_queue.cpp
struct EvpServer;   // evp_doorbell.cpp
constexpr int kImagePoisoned = 3;
struct AeadState {
  tlsgpu_sessions* sess;  // the device table holding the context's session
  uint32_t slot;          // session id in sess
  int kind;
  unsigned tag_len;
  EvpBatcher* batcher;    // the queue of the context's device (pooled contexts), or null
  uint32_t evp_dev;       // index of the context's device among the EVP devices
  hipEvent_t installed;   // the slot's event, recorded after the context's key install
  uint32_t key_id = 0;    // unique per install (doorbell server's LDS table cache)
  mutable std::atomic<bool> install_pending{true};  // no call has waited for it yet
  // Deferred install (round 5): the session image built on the host at init
  // (session_host.cpp) in a pinned image buffer, installed by the context's
  // first call — posted with the doorbell job, or one upload kernel ahead of a
  // launched job — so EVP_AEAD_CTX_init launches nothing.  0: on the device
  // (or no image), 1: image waiting, 2: a call is installing it,
  // kImagePoisoned: an install job went unanswered (image and slot leaked)
  mutable std::atomic<int> image{0};
  uint8_t* img_h = nullptr;  // pinned image (host / device views)
  uint8_t* img_d = nullptr;
  bool img_tables = false;   // the image has GCM tables
  bool img_compact = false;  // ... only m[8] = H^e of each Shoup table (round 6)
  hipEvent_t slot_ev = nullptr;  // the slot's event: its previous owner's scrub
};

// A pool of pinned chunks: per device a free list of (host, device view) pairs,
// refilled by one hipHostMalloc slab of `slab` bytes carved into `chunk`-byte
// chunks and held for the process.  Chunks go back without a HIP call.
// `keys` (chunks hold key material): take sets the device and fails without a
// device view, a new slab is zeroed, and give zeroes the chunk.
struct PinnedPool {
  const size_t chunk, slab;
  const bool keys;
  struct {
    std::mutex mu;
    std::vector<std::pair<uint8_t*, uint8_t*>> free;  // (host, device view)
    std::atomic<uint64_t> slabs{0};
  } per_dev[kMaxDev];
  bool take(int dev, uint8_t** h, uint8_t** d);
  void give(int dev, uint8_t* h, uint8_t* d);
};
// Pinned image buffers of deferred installs and key areas (kImageBytes each, 32
// per slab), reused, zeroed on return.
extern PinnedPool g_images;
// Pinned staging chunks (round 6): a thread's
// per-call staging is one kStageChunk of pinned host memory carved from
// kStageSlab-byte slabs (one hipHostMalloc per 32 threads), enough for any TLS
// record job ([RawJob | nonce | ad | 16 KiB + 2 KiB in | status | out] <=
// 40 KiB); a thread that makes a larger EVP call grows to its own allocation.
// Chunks go back to the free list without a HIP call (a thread's exit makes
// none), so the pinned bytes are bounded by the peak number
// of calling threads x 64 KiB.  No device buffer unless a path needs one (the
// zero-copy per-call path, the default, reads and writes the pinned chunk).
constexpr size_t kStageChunk = 64u << 10;
constexpr size_t kStageSlab = 2u << 20;
extern PinnedPool g_stage_chunks;

// One per (thread, device): buffers, stream and event belong to that device.
struct Staging {
  int device = -1;
  hipStream_t stream = nullptr;
  hipEvent_t done = nullptr;
  uint8_t* d_buf = nullptr;  // device buffer (only the staged, non-zero-copy paths)
  uint8_t* h_buf = nullptr;
  uint8_t* h_dev = nullptr;  // h_buf as the device addresses it (zero-copy calls)
  size_t cap = 0;            // bytes of h_buf (kStageChunk: a pooled chunk)
  size_t dcap = 0;           // bytes of d_buf
  // key areas (round 5; round 6: buffers from the shared pinned image pool,
  // not per thread): install_one builds the slot's image here
  // (session_host.cpp) and one kernel copies it into the slot; `dirty` until
  // the copy is known done (its event), then zeroed and given back to the pool
  // (explicit_bzero analogue, g_images.give)
  struct KeyArea {
    uint8_t* h = nullptr;
    uint8_t* dev = nullptr;
    hipEvent_t ev = nullptr;
    bool dirty = false;
  };
  static constexpr int kKeyAreas = 4;
  KeyArea keys[kKeyAreas];
  uint32_t key_next = 0;
  void give_key_area(KeyArea& k) {
    g_images.give(device, k.h, k.dev);  // zeroes it
    k.h = k.dev = nullptr;
    k.dirty = false;
  }
  // the next key area (waiting for and zeroing its previous image if needed)
  KeyArea* take_key_area() {
    KeyArea& k = keys[key_next++ % kKeyAreas];
    if (!k.ev && hipEventCreateWithFlags(&k.ev, hipEventDisableTiming) != hipSuccess) {
      k.ev = nullptr;
      return nullptr;
    }
    if (k.dirty) {
      if (hipEventSynchronize(k.ev) != hipSuccess) return nullptr;
      give_key_area(k);
    }
    if (!g_images.take(device, &k.h, &k.dev)) return nullptr;
    return &k;
  }
  // zero and give back every key area whose copy has finished (no wait)
  void sweep_key_areas() {
    for (KeyArea& k : keys)
      if (k.dirty && hipEventQuery(k.ev) == hipSuccess) give_key_area(k);
  }
  bool any_dirty_key_area() const {
    for (const KeyArea& k : keys)
      if (k.dirty) return true;
    return false;
  }
  ~Staging() {
    if (device >= 0) (void)hipSetDevice(device);  // the buffers' and the event's device
    if (d_buf) (void)hipFree(d_buf);
    release_host();
    if (done) (void)hipEventDestroy(done);
  }
  void release_host() {
    if (h_buf && cap == kStageChunk) g_stage_chunks.give(device, h_buf, h_dev);
    else if (h_buf) (void)hipHostFree(h_buf);
    h_buf = h_dev = nullptr;
    cap = 0;
  }
  // A job that may still run on the device owns the buffers (a doorbell post
  // nobody answered): forget them without freeing, the next ensure allocates.
  void abandon() {
    d_buf = h_buf = h_dev = nullptr;
    cap = dcap = 0;
  }
  // `bytes` of pinned staging (and of device staging when `dev_buf`) on `dev`
  bool ensure(int dev, size_t bytes, bool dev_buf = false);  // evp_aead.cpp
};

// TLSGPU_EVP_ZEROCOPY=0: stage EVP jobs through HBM.  A function-local static:
// the queue's load-time constructor asks before other units' initialisers run.
inline bool evp_zerocopy() {
  static const bool on = env_not_off("TLSGPU_EVP_ZEROCOPY");
  return on;
}

// evp_aead.cpp
tlsgpu_engine* evp_engine(size_t k);
size_t evp_device_count();
size_t evp_pick();
void slab_give(size_t dk, tlsgpu_sessions* t, uint32_t slot);

// evp_doorbell.cpp (the switch and the shutdown state are read on every call)
extern unsigned g_doorbell_groups;        // 0: off
extern std::atomic<int> g_evp_shutdown;   // 0 running, 1 stopping, 2 drained
inline bool doorbell_enabled() {
  return g_doorbell_groups != 0 && g_evp_shutdown.load(std::memory_order_acquire) == 0;
}
Staging* stage_for(int dev);
EvpServer* evp_server(size_t k, tlsgpu_engine* e);
DoorbellSlot* thread_slot(EvpServer* sv, size_t k, uint32_t** seq);
void doorbell_fill(DoorbellSlot* slot, const AeadState* st, uint32_t op, const void* d_status);
int doorbell_post_wait(EvpServer* sv, DoorbellSlot* slot, uint32_t* seq, size_t k, Staging* stg,
                       uint64_t* t0_out);
void doorbell_served(EvpServer* sv, const DoorbellSlot* slot, uint64_t t0);
bool doorbell_scrub(const AeadState* st);
bool doorbell_scrub_async(const AeadState* st);
void evp_sweep_scrubs_for(size_t dk);
void evp_wait_scrub_of(const tlsgpu_sessions* t, uint32_t slot);

// evp_queue.cpp
EvpBatcher* evp_queue_take_session(size_t dk, tlsgpu_sessions** sess, uint32_t* slot);
void evp_queue_give_session(EvpBatcher* b, uint32_t slot);
int evp_queue_call(EvpBatcher* b, const AeadState* st, bool seal, unsigned char* out,
                   size_t* out_len, size_t max_out_len, const unsigned char* nonce,
                   size_t nonce_len, const unsigned char* in, size_t in_len,
                   const unsigned char* ad, size_t ad_len);

}  // namespace tg
