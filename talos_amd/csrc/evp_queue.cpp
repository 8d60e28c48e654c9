// evp_queue.cpp — the EVP coalescing queue: EvpSlot, EvpBatcher with its
// dispatcher and completer threads, the pooled contexts' sessions,
// evp_queue_call, tlsgpu_evp_set_batching and tlsgpu_evp_batch_stats.
#include <climits>
#include <condition_variable>
#include <deque>
#include <linux/futex.h>
#include <sys/syscall.h>
#include <thread>
#include <unistd.h>

#include "evp_internal.h"

using namespace tg;

// EVP coalescing queue (TaLoS make_asynchronous_ecall,
// src/talos/enclaveshim/enclaveshim_ecalls.c:457-610, in GPU form).
//
// With batching on (tlsgpu_evp_set_batching or TLSGPU_EVP_BATCH_US > 0),
// EVP_AEAD_CTX_init installs the key into a slot of one shared device session
// pool, and every EVP_AEAD_CTX_seal/open joins the batch being built and
// blocks until it completes.  Batches live in a ring of kEvpSlots staging
// slots (pinned host + device, one HIP stream each):
//   caller      reserves a descriptor and byte ranges in the building slot
//               (under the lock), copies its nonce / AD / input into the
//               pinned slot itself (outside the lock, in parallel with the
//               other callers), then sleeps on the slot's futex word;
//   dispatcher  closes the building slot when the GPU is idle, the slot is
//               full, or the window since its first job has passed; waits for
//               the slot's writers, then issues one H2D, one raw batch per
//               direction, one D2H and an event on the slot's stream;
//   completer   waits on the events in order and wakes each slot's callers
//               with ONE futex wake; every caller copies its own output out,
//               and the last one returns the slot to the ring.
// So at most kEvpSlots-1 batches are in flight while the next one fills, no
// per-job work runs on the dispatcher, and results are the per-call path's,
// bit for bit (same raw kernels).
constexpr uint32_t kEvpSlots = 3;
constexpr uint32_t kEvpMaxJobs = 1024;
constexpr size_t kEvpDescBytes = sizeof(RawJob) * kEvpMaxJobs;
constexpr size_t kEvpInBytes = 8u << 20, kEvpOutBytes = 8u << 20;
constexpr size_t kEvpStatusOff = kEvpDescBytes + kEvpInBytes;   // int32 x kEvpMaxJobs
constexpr size_t kEvpOutOff = kEvpStatusOff + 4 * kEvpMaxJobs;
constexpr size_t kEvpSlotBytes = kEvpOutOff + kEvpOutBytes;

struct EvpSlot {
  uint8_t* h = nullptr;  // pinned: [RawJob x kEvpMaxJobs | inputs | status | outputs]
  uint8_t* d = nullptr;  // device, same layout (zero-copy: h as the device addresses it)
  bool zc = false;       // zero-copy: no device copy of the slot, no H2D / D2H
  hipStream_t stream = nullptr;
  hipEvent_t done = nullptr;
  // built under EvpBatcher::mu: seal descriptors from the front, open ones
  // from the back, so each direction is one contiguous raw batch
  uint32_t nseal = 0, nopen = 0;
  unsigned kinds_seal = 0, kinds_open = 0;  // AEAD kinds present (run_batch masks)
  size_t in_used = 0, out_used = 0;
  std::chrono::steady_clock::time_point first, submitted_at;
  std::atomic<uint32_t> writers{0};  // callers still copying in
  std::atomic<uint32_t> readers{0};  // callers still copying out
  std::atomic<uint32_t> gen{0};      // bumped on completion (futex word)
  bool ok = false;
  uint32_t jobs() const { return nseal + nopen; }
};

struct tg::EvpBatcher {
  std::mutex mu;
  std::condition_variable cv_disp, cv_comp, cv_slot;
  EvpSlot slots[kEvpSlots];
  EvpSlot* building = nullptr;  // the slot callers join (nullptr: all busy)
  std::vector<EvpSlot*> free_ring;
  std::deque<EvpSlot*> submitted;
  uint32_t inflight = 0;
  bool full = false;  // a caller found the building slot full
  std::thread disp, comp;
  unsigned window_us = 0, max_jobs = kEvpMaxJobs;
  tlsgpu_sessions* pool = nullptr;
  std::vector<int> free_sessions;
  uint64_t batches = 0, jobs_done = 0;
  // TLSGPU_EVP_STATS=1: nanoseconds summed over batches (printed at exit)
  uint64_t ns_wait = 0, ns_writers = 0, ns_submit = 0, ns_gpu = 0;
  void dispatch_loop();
  void complete_loop();
  void submit(EvpSlot* s);
  bool submit_work(EvpSlot* s);
  void release(EvpSlot* s);
};
// one coalescing queue per EVP device (index as evp_engine); g_batcher_on once
// tlsgpu_evp_set_batching has created them
static EvpBatcher* g_batchers[kMaxEvpDevices] = {};
static std::mutex g_batcher_mu;
static bool g_batcher_on = false;

static inline void futex_wait(std::atomic<uint32_t>* w, uint32_t v) {
  syscall(SYS_futex, reinterpret_cast<uint32_t*>(w), FUTEX_WAIT_PRIVATE, v, nullptr, nullptr, 0);
}
static inline void futex_wake_all(std::atomic<uint32_t>* w) {
  syscall(SYS_futex, reinterpret_cast<uint32_t*>(w), FUTEX_WAKE_PRIVATE, INT_MAX, nullptr, nullptr,
          0);
}

// A session of device dk's queue pool for a new context (its table and slot),
// or nullptr: no queue, or none free.
EvpBatcher* tg::evp_queue_take_session(size_t dk, tlsgpu_sessions** sess, uint32_t* slot) {
  std::lock_guard<std::mutex> lk(g_batcher_mu);
  // a queue counts only once tlsgpu_evp_set_batching has published every
  // device's (a partial setup that failed leaves g_batcher_on false)
  EvpBatcher* b = g_batcher_on ? g_batchers[dk] : nullptr;
  if (!b || b->free_sessions.empty()) return nullptr;
  *slot = (uint32_t)b->free_sessions.back();
  b->free_sessions.pop_back();
  *sess = b->pool;
  return b;
}
void tg::evp_queue_give_session(EvpBatcher* b, uint32_t slot) {
  std::lock_guard<std::mutex> lk(g_batcher_mu);
  b->free_sessions.push_back((int)slot);
}

// ---------------------------------------------------------------------------
// EVP coalescing queue: callers, dispatcher, completer

// 1 / 0 / -1 as gpu_call; -2: the job is too large for a staging slot (the
// caller runs it on its own staging instead).
int tg::evp_queue_call(EvpBatcher* b, const AeadState* st, bool seal, unsigned char* out,
                       size_t* out_len, size_t max_out_len, const unsigned char* nonce,
                       size_t nonce_len, const unsigned char* in, size_t in_len,
                       const unsigned char* ad, size_t ad_len) {
  auto al = [](size_t v) { return (v + 15) & ~(size_t)15; };
  const size_t need_in = al(nonce_len) + al(ad_len) + al(in_len);
  const size_t out_bytes = seal ? in_len + st->tag_len : std::max(max_out_len, in_len);
  const size_t need_out = al(out_bytes + 1);
  if (need_in > kEvpInBytes / 4 || need_out > kEvpOutBytes / 4) return -2;
  std::unique_lock<std::mutex> lk(b->mu);
  EvpSlot* s;
  for (;;) {
    s = b->building;
    if (s && s->jobs() < b->max_jobs && s->in_used + need_in <= kEvpInBytes &&
        s->out_used + need_out <= kEvpOutBytes)
      break;
    if (s && !b->full) {  // no room: have it dispatched now
      b->full = true;
      b->cv_disp.notify_one();
    }
    b->cv_slot.wait(lk);
  }
  const bool first = s->jobs() == 0;
  const uint32_t idx = seal ? s->nseal++ : kEvpMaxJobs - 1 - s->nopen++;
  (seal ? s->kinds_seal : s->kinds_open) |= 1u << st->kind;
  const size_t io = kEvpDescBytes + s->in_used, oo = kEvpOutOff + s->out_used;
  s->in_used += need_in;
  s->out_used += need_out;
  s->writers.fetch_add(1, std::memory_order_relaxed);
  const uint32_t gen = s->gen.load(std::memory_order_relaxed);
  if (first) {
    s->first = std::chrono::steady_clock::now();
    b->cv_disp.notify_one();
  }
  lk.unlock();
  RawJob* rj = reinterpret_cast<RawJob*>(s->h) + idx;
  size_t o = io;
  rj->nonce = (uint64_t)(s->d + o);
  if (nonce_len) memcpy(s->h + o, nonce, nonce_len);
  o += al(nonce_len);
  rj->aad = (uint64_t)(s->d + o);
  if (ad_len) memcpy(s->h + o, ad, ad_len);
  o += al(ad_len);
  rj->in = (uint64_t)(s->d + o);
  if (in_len) memcpy(s->h + o, in, in_len);
  rj->out = (uint64_t)(s->d + oo);
  rj->in_len = (uint32_t)in_len;
  rj->nonce_len = (uint32_t)nonce_len;
  rj->aad_len = (uint32_t)ad_len;
  rj->session = st->slot;
  rj->max_out = max_out_len;
  s->writers.fetch_sub(1, std::memory_order_release);
  while (s->gen.load(std::memory_order_acquire) == gen) futex_wait(&s->gen, gen);
  int r;
  if (!s->ok) {
    r = -1;
  } else {
    const int32_t status = reinterpret_cast<const int32_t*>(s->h + kEvpStatusOff)[idx];
    if (status < 0) {  // the kernel's zero-fill (evp_aead.c:137-143)
      if (max_out_len) memset(out, 0, max_out_len);
      r = 0;
    } else {
      if (status) memcpy(out, s->h + oo, (size_t)status);
      *out_len = (size_t)status;
      r = 1;
    }
  }
  if (s->readers.fetch_sub(1, std::memory_order_acq_rel) == 1) b->release(s);
  return r;
}

// The last reader hands the slot back: it becomes the building slot if there
// is none, else waits in the ring.
void EvpBatcher::release(EvpSlot* s) {
  std::lock_guard<std::mutex> lk(mu);
  s->nseal = s->nopen = 0;
  s->kinds_seal = s->kinds_open = 0;
  s->in_used = s->out_used = 0;
  if (!building) {
    building = s;
    full = false;
    cv_slot.notify_all();
  } else {
    free_ring.push_back(s);
  }
}

void EvpBatcher::dispatch_loop() {
  std::unique_lock<std::mutex> lk(mu);
  for (;;) {
    cv_disp.wait(lk, [&] { return building && building->jobs() > 0; });
    // batching policy: go now when the GPU is idle or the slot is full,
    // else when the window since the slot's first job has passed
    const auto deadline = building->first + std::chrono::microseconds(window_us);
    cv_disp.wait_until(lk, deadline, [&] { return inflight == 0 || full; });
    EvpSlot* s = building;
    full = false;
    const auto t_close = std::chrono::steady_clock::now();
    ns_wait += std::chrono::duration_cast<std::chrono::nanoseconds>(t_close - s->first).count();
    if (free_ring.empty()) {
      building = nullptr;
    } else {
      building = free_ring.back();
      free_ring.pop_back();
      cv_slot.notify_all();
    }
    inflight++;
    s->readers.store(s->jobs(), std::memory_order_relaxed);
    lk.unlock();
    while (s->writers.load(std::memory_order_acquire)) std::this_thread::yield();
    const auto t_sub = std::chrono::steady_clock::now();
    submit(s);
    s->submitted_at = std::chrono::steady_clock::now();
    lk.lock();
    ns_writers += std::chrono::duration_cast<std::chrono::nanoseconds>(t_sub - t_close).count();
    ns_submit +=
        std::chrono::duration_cast<std::chrono::nanoseconds>(s->submitted_at - t_sub).count();
    submitted.push_back(s);
    cv_comp.notify_one();
  }
}

void EvpBatcher::submit(EvpSlot* s) {
  s->ok = false;
  if (hipSetDevice(pool->eng->device) != hipSuccess) return;
  if (!submit_work(s)) {
    // part of the batch may already be queued: let it drain before the slot's
    // pinned and device buffers go back to the ring for the next batch
    (void)hipStreamSynchronize(s->stream);
    return;
  }
  s->ok = true;
}

bool EvpBatcher::submit_work(EvpSlot* s) {
  const uint32_t ns = s->nseal, no = s->nopen;
  int32_t* d_status = reinterpret_cast<int32_t*>(s->d + kEvpStatusOff);
  const RawJob* d_desc = reinterpret_cast<const RawJob*>(s->d);
  if (!s->zc && hipMemcpyAsync(s->d, s->h, kEvpDescBytes + s->in_used, hipMemcpyHostToDevice,
                               s->stream) != hipSuccess)
    return false;
  if (ns && run_batch(pool, d_desc, ns, nullptr, nullptr, d_status, s->stream, true, true,
                     nullptr, s->kinds_seal) != TLSGPU_OK)
    return false;
  if (no && run_batch(pool, d_desc + (kEvpMaxJobs - no), no, nullptr, nullptr,
                      d_status + (kEvpMaxJobs - no), s->stream, false, true, nullptr,
                      s->kinds_open) != TLSGPU_OK)
    return false;
  return (s->zc || hipMemcpyAsync(s->h + kEvpStatusOff, s->d + kEvpStatusOff,
                                  kEvpOutOff - kEvpStatusOff + s->out_used,
                                  hipMemcpyDeviceToHost, s->stream) == hipSuccess) &&
         hipEventRecord(s->done, s->stream) == hipSuccess;
}

void EvpBatcher::complete_loop() {
  std::unique_lock<std::mutex> lk(mu);
  for (;;) {
    cv_comp.wait(lk, [&] { return !submitted.empty(); });
    EvpSlot* s = submitted.front();
    submitted.pop_front();
    lk.unlock();
    if (s->ok && hipEventSynchronize(s->done) != hipSuccess) {
      s->ok = false;
      (void)hipStreamSynchronize(s->stream);  // nothing of the slot may still run
    }
    const uint64_t gpu_ns = std::chrono::duration_cast<std::chrono::nanoseconds>(
                                std::chrono::steady_clock::now() - s->submitted_at)
                                .count();
    const uint32_t n = s->jobs();
    s->gen.fetch_add(1, std::memory_order_release);
    futex_wake_all(&s->gen);
    lk.lock();
    batches++;
    jobs_done += n;
    ns_gpu += gpu_ns;
    inflight--;
    cv_disp.notify_one();
  }
}

// One device's queue: pool table, kEvpSlots staging slots, dispatcher and
// completer threads (they live as long as the process).  nullptr on failure.
static EvpBatcher* make_batcher(tlsgpu_engine* e, unsigned window_us, unsigned max_jobs,
                                uint32_t cap) {
  auto* b = new (std::nothrow) EvpBatcher();
  if (!b) {
    fail(TLSGPU_ENOMEM, "batcher");
    return nullptr;
  }
  b->window_us = window_us;
  b->max_jobs = max_jobs ? std::min(max_jobs, kEvpMaxJobs) : kEvpMaxJobs;
  if (tlsgpu_sessions_create(e, cap, &b->pool) != TLSGPU_OK) {
    delete b;
    return nullptr;
  }
  bool ok = hipSetDevice(e->device) == hipSuccess;
  for (EvpSlot& s : b->slots) {
    ok = ok && hipHostMalloc((void**)&s.h, kEvpSlotBytes, hipHostMallocDefault) == hipSuccess;
    // zero-copy (TLSGPU_EVP_ZEROCOPY, default on): the batch kernels read the
    // jobs from and write statuses and outputs to the pinned slot directly
    s.zc = ok && evp_zerocopy() && hipHostGetDevicePointer((void**)&s.d, s.h, 0) == hipSuccess;
    if (!s.zc) s.d = nullptr;
    ok = ok && (s.zc || hipMalloc((void**)&s.d, kEvpSlotBytes) == hipSuccess) &&
         hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking) == hipSuccess &&
         hipEventCreateWithFlags(&s.done, hipEventDisableTiming) == hipSuccess;
  }
  if (!ok) {  // never started: nothing queued on its streams
    fail(TLSGPU_EHIP, "EVP queue staging on device %d", e->device);
    for (EvpSlot& s : b->slots) {
      if (s.h) (void)hipHostFree(s.h);
      if (s.d && !s.zc) (void)hipFree(s.d);
    }
    tlsgpu_sessions_destroy(b->pool);
    delete b;
    return nullptr;
  }
  b->building = &b->slots[0];
  for (uint32_t i = kEvpSlots - 1; i >= 1; i--) b->free_ring.push_back(&b->slots[i]);
  for (int i = (int)cap - 1; i >= 0; i--) b->free_sessions.push_back(i);
  b->disp = std::thread([b] { b->dispatch_loop(); });
  b->comp = std::thread([b] { b->complete_loop(); });
  return b;
}

extern "C" int tlsgpu_evp_set_batching(unsigned window_us, unsigned max_jobs,
                                       unsigned pool_sessions) {
  std::lock_guard<std::mutex> lk(g_batcher_mu);
  if (g_batcher_on) {  // already running: adjust the window / batch size only
    for (EvpBatcher* b : g_batchers) {
      if (!b) continue;
      std::lock_guard<std::mutex> lk2(b->mu);
      b->window_us = window_us;
      if (max_jobs) b->max_jobs = std::min(max_jobs, kEvpMaxJobs);
    }
    return TLSGPU_OK;
  }
  if (window_us == 0 && max_jobs == 0) return TLSGPU_OK;  // stays off
  // one queue per EVP device: contexts initialised afterwards take a pool slot
  // on the device evp_pick gives them
  const uint32_t cap = pool_sessions ? pool_sessions : 1024;
  const size_t ndev = evp_device_count();
  // All devices or none: a queue built before a later device failed stays in
  // g_batchers unused (g_batcher_on stays false, so no context takes its pool
  // slots) and a retry reuses it instead of building a second one over it —
  // its dispatcher and completer threads never outlive their queue's pointer.
  for (size_t k = 0; k < ndev; k++) {
    if (g_batchers[k]) {
      std::lock_guard<std::mutex> lk2(g_batchers[k]->mu);
      g_batchers[k]->window_us = window_us;
      if (max_jobs) g_batchers[k]->max_jobs = std::min(max_jobs, kEvpMaxJobs);
      continue;
    }
    tlsgpu_engine* e = evp_engine(k);
    if (!e) return fail(TLSGPU_EHIP, "no GPU engine for EVP device %zu", k);
    EvpBatcher* b = make_batcher(e, window_us, max_jobs, cap);
    if (!b) return TLSGPU_EHIP;
    g_batchers[k] = b;
  }
  g_batcher_on = true;
  if (getenv("TLSGPU_EVP_STATS")) {
    atexit([] {
      uint64_t nb = 0, nj = 0, w = 0, wr = 0, sb = 0, gp = 0;
      for (EvpBatcher* q : g_batchers) {
        if (!q) continue;
        std::lock_guard<std::mutex> lk3(q->mu);
        nb += q->batches;
        nj += q->jobs_done;
        w += q->ns_wait;
        wr += q->ns_writers;
        sb += q->ns_submit;
        gp += q->ns_gpu;
      }
      const double d = nb ? (double)nb : 1.0;
      fprintf(stderr,
              "{\"evp_queue\": {\"devices\": %zu, \"batches\": %llu, \"jobs\": %llu, "
              "\"jobs_per_batch\": %.2f, \"us_first_to_close\": %.1f, \"us_writers\": %.1f, "
              "\"us_submit\": %.1f, \"us_submit_to_done\": %.1f}}\n",
              evp_device_count(), (unsigned long long)nb, (unsigned long long)nj, nj / d,
              w / d / 1e3, wr / d / 1e3, sb / d / 1e3, gp / d / 1e3);
    });
  }
  return TLSGPU_OK;
}

extern "C" int tlsgpu_evp_batch_stats(uint64_t* batches, uint64_t* jobs) {
  std::lock_guard<std::mutex> lk(g_batcher_mu);
  uint64_t nb = 0, nj = 0;
  for (EvpBatcher* b : g_batchers) {
    if (!b) continue;
    std::lock_guard<std::mutex> lk2(b->mu);
    nb += b->batches;
    nj += b->jobs_done;
  }
  if (batches) *batches = nb;
  if (jobs) *jobs = nj;
  return TLSGPU_OK;
}

// TLSGPU_EVP_BATCH_US=<window> turns the queue on at load time for unchanged
// applications (LD_PRELOAD); TLSGPU_EVP_POOL sets the pooled context count.
__attribute__((constructor)) static void evp_batching_from_env() {
  const char* w = getenv("TLSGPU_EVP_BATCH_US");
  if (!w || !*w) return;
  const char* p = getenv("TLSGPU_EVP_POOL");
  tlsgpu_evp_set_batching((unsigned)strtoul(w, nullptr, 10), 0,
                          p ? (unsigned)strtoul(p, nullptr, 10) : 0);
}
