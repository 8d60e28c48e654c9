// evp_doorbell.cpp — host side of the doorbell server (evp_server.hip):
// EvpServer and its launches, the threads' doorbell slots, post and wait,
// scrubs through the server, the trace, the shutdown contract with its exit
// hooks and crash trace.  Both thread-locals of the per-call path live here,
// the staging set (t_stages) before the doorbell slots (t_slots): at thread
// exit the slots go first, then the staging, whichever was touched first.
#include <csignal>
#include <execinfo.h>
#include <sched.h>
#include <sys/syscall.h>
#include <unistd.h>

#include "evp_internal.h"

using namespace tg;

// ---------------------------------------------------------------------------
// Doorbell server (round 4, evp_server.hip): per-call AES-GCM and RFC 7539
// ChaCha20-Poly1305 jobs without a kernel launch.  TLSGPU_EVP_DOORBELL=<G> (or tlsgpu_evp_set_doorbell) keeps G
// server workgroups resident per EVP device while calls arrive; a calling
// thread owns one slot of kSlotsPerGroup * G (slot k -> workgroup k % G), posts
// its job number there and spins on the answer.  An instance lives `lifetime`
// (TLSGPU_EVP_DOORBELL_MS, default 5 ms) and is relaunched by the first post
// after half of that has passed, on the same stream: a job is only posted
// while an instance that still polls for at least half a lifetime is queued or
// running, so every posted job is served, and a process that stops calling
// leaves nothing spinning.  AES-GCM, RFC 7539 and (round 5) draft ChaCha20-
// Poly1305 jobs; pooled (queued) contexts keep the launched path; a context's first call carries its
// deferred install (the host-built image, defer_install) and its cleanup posts
// a scrub job; a short GCM job's input is staged into LDS by the server's idle
// waves.  On by default (round 5, kDoorbellDefaultGroups).
// The lifetime is short on purpose: this box runs at most GPU_MAX_HW_QUEUES = 4
// hardware queues per process, so with more streams than that (engine + 4 call
// streams + server) the server's queue is shared, and a kernel launched on a
// stream that shares it waits until the running instance exits
// (tools/doorbell_probe.hip: 2.7 s behind a 3 s instance with 8 other streams).
// 5 ms bounds that wait; relaunching every 2.5 ms under load costs one launch.
constexpr uint32_t kSlotsPerGroup = 8;
struct tg::EvpServer {
  int device = -1;
  uint32_t groups = 0, nslots = 0;
  uint64_t lifetime_ns = 0;
  DoorbellSlot* slots = nullptr;  // pinned host
  DoorbellSlot* d_slots = nullptr;
  uint32_t* stop = nullptr;       // pinned host word
  uint32_t* d_stop = nullptr;
  hipStream_t stream = nullptr;
  std::mutex mu;
  std::atomic<uint64_t> deadline_ns{0};  // post only before this (host clock), else relaunch
  uint64_t end_ns = 0;                   // when the last queued instance stops polling, at the
                                         // earliest (host clock; under mu)
  std::vector<uint32_t> free_slots;
  std::atomic<uint64_t> jobs{0}, launches{0};
  // threads holding a slot, and 1 + the highest slot ever handed out: an
  // instance is launched with as many workgroups as there are calling
  // threads (at most `groups`), and enough that its 64 polling lanes per
  // workgroup cover every slot in use
  std::atomic<uint32_t> active{0}, hi_slot{0};
  std::atomic<uint32_t> covered{0};  // slots the last launched instance polls (64 per workgroup)
  std::atomic<uint32_t> last_launched_g{0};  // workgroups of the last launched instance
  uint32_t launch_seq = 0, last_g = 0;  // the last launched instance (under mu)
  // every launched instance whose workgroups have not all been seen leaving:
  // (launch number, workgroups), oldest first (under mu; pruned at each launch)
  std::vector<std::pair<uint32_t, uint32_t>> outstanding;
  // TLSGPU_EVP_DOORBELL_TRACE=1: per-slot device timestamps (pinned) and their
  // sums, printed at exit: pick -> slot loaded -> job done -> released (ticks
  // of 10 ns), and the caller's post -> done-seen wall time (ns)
  uint64_t* d_scrubs = nullptr;  // HBM: the scrub ring (ServerArgs::scrubs)
  // asynchronous cleanup scrubs (round 6): a status word per doorbell slot
  // (pinned) and the scrubs posted but not yet seen done, whose session slots
  // go back to their slab only then
  int32_t* scrub_status = nullptr;
  int32_t* d_scrub_status = nullptr;
  struct PendingScrub {
    tlsgpu_sessions* sess;
    uint32_t slot;
    size_t evp_dev;
    DoorbellSlot* ds;
    uint32_t post;
    uint64_t t0;
  };
  std::mutex pend_mu;
  std::vector<PendingScrub> pending;
  std::atomic<uint32_t> npending{0};  // pending.size(), read without the lock
  uint64_t* trace = nullptr;
  uint64_t* d_trace = nullptr;
  std::atomic<uint64_t> tr_n{0}, tr_load{0}, tr_job{0}, tr_rel{0}, tr_host_ns{0};
  std::atomic<uint64_t> tr_marks_n{0}, tr_phase[8] = {};  // GCM jobs: loaded -> mark 0 .. 6 -> done
  std::atomic<uint64_t> tr_last[4] = {};  // since loaded: wave 0 blocks / shoup, last wave blocks / shoup
  std::atomic<uint64_t> tr_inst_n{0}, tr_inst[2] = {};  // install jobs: loaded -> image read -> tables built
  void account_trace(const DoorbellSlot* slot, uint64_t t0);
};
static EvpServer* g_servers[kMaxEvpDevices] = {};
// the servers whose setup succeeded, read without the lock on every call (a
// process-wide mutex per call cost 16 calling threads more than the call)
static std::atomic<EvpServer*> g_ready_servers[kMaxEvpDevices] = {};
constexpr uint32_t kExitedWord = 32;  // exit marks after the stop word (256 workgroups max)
static std::mutex g_server_mu;
// On by default (round 5), G = 64: TLSGPU_EVP_DOORBELL=0 or
// tlsgpu_evp_set_doorbell(0, 0) turns it off.  The round-4 exit SIGSEGV is
// explained and removed (thread-exit destructors made HIP
// calls; the shutdown contract below drains every instance).  Design grounds:
// the EVP surface's users are per-call callers (an unchanged libssl under
// LD_PRELOAD), for whom the doorbell is 1.5-6x the launched path and makes
// init / cleanup launch-free; a process that never calls EVP never creates a
// server; an instance holds only as many CUs as calling threads (<= G), and
// only while calls arrive plus one lifetime (5 ms).
constexpr unsigned kDoorbellDefaultGroups = 64;
unsigned tg::g_doorbell_groups = (unsigned)env_uint("TLSGPU_EVP_DOORBELL", kDoorbellDefaultGroups, 10);
static unsigned g_doorbell_ms = [] {
  const char* v = getenv("TLSGPU_EVP_DOORBELL_MS");
  const unsigned ms = v && *v ? (unsigned)strtoul(v, nullptr, 10) : 5u;
  return ms ? ms : 5u;
}();

// A waiting caller spins this long before it starts yielding the core
// (TLSGPU_EVP_DOORBELL_YIELD_US, default 100): with more calling threads than
// cores, spinners keep the threads that would post from running.
static const uint64_t g_doorbell_yield_ns = env_uint("TLSGPU_EVP_DOORBELL_YIELD_US", 100, 10) * 1000ull;

// Test hook (tests/test_evp_doorbell.py): sleep this long between a call's
// server_ensure and its post, as a caller descheduled there would.
static const unsigned g_test_post_delay_us =
    (unsigned)env_uint("TLSGPU_TEST_DOORBELL_POST_DELAY_US", 0, 10);

static const bool g_doorbell_trace = env_on("TLSGPU_EVP_DOORBELL_TRACE");

// ---------------------------------------------------------------------------
// Shutdown contract (round 5).
// A server instance reads and writes pinned host memory (its slots, the stop
// page, the callers' staging) for as long as it runs, and instances queue on
// the server's stream (and on whatever shares its hardware queue).  Before
// the HIP runtime tears down — it frees every pinned allocation — every
// instance ever launched must have left.  tlsgpu_evp_shutdown():
//   1. no new instance and no new post from here on (g_evp_shutdown);
//   2. the stop word of every server: a running instance leaves within 16
//      polls or after the job it is on, a queued one at its first instruction;
//   3. waits for EVERY outstanding instance's exit marks (not only the last
//      one's), reading pinned memory only — no HIP call — with no silent cap:
//      a note on stderr after 1 s, TLSGPU_ETIMEOUT after TLSGPU_EVP_SHUTDOWN_MS
//      (default 60,000);
//   4. callers still spinning on a post see the drain and take the launched
//      path for that call if no instance served it.
// It runs at the earliest point of process exit (a thread-local guard of the
// main thread: thread-local destructors of the exiting thread run before any
// atexit or static destructor, so before the runtime's), again from an atexit
// handler (exit from another thread) and from the library destructor
// (dlclose); it is idempotent.  At exit a drain that timed out ends the
// process with _exit(70) before the runtime's teardown can free memory a
// still-running instance uses.
std::atomic<int> tg::g_evp_shutdown{0};  // 0 running, 1 stopping, 2 drained
static std::mutex g_shutdown_mu;
static const uint64_t g_shutdown_cap_ns = [] {
  const char* v = getenv("TLSGPU_EVP_SHUTDOWN_MS");
  const uint64_t ms = v && *v ? strtoull(v, nullptr, 10) : 60000ull;
  return (ms ? ms : 60000ull) * 1000000ull;
}();
static const bool g_shutdown_verbose = env_on("TLSGPU_EVP_SHUTDOWN_VERBOSE");

// Every workgroup of instance `seq` (g workgroups) has left.  A workgroup
// stores its instance's launch number into exited[b] as its last act;
// instances of one server run one after another on its stream, so a mark
// >= seq (wrapping compare) means workgroup b of this instance or of a later
// one — which only started after this one ended — has left.
static bool instance_left(const EvpServer* sv, uint32_t seq, uint32_t g) {
  for (uint32_t b = 0; b < g; b++)
    if ((int32_t)(__atomic_load_n(sv->stop + kExitedWord + b, __ATOMIC_ACQUIRE) - seq) < 0)
      return false;
  return true;
}

// Which exit hook is running (TLSGPU_CRASH_TRACE names it in a fault report):
// 0 running, 1 the main thread's exit guard, 2 atexit, 3 library destructor.
static volatile sig_atomic_t g_exit_phase = 0;

static void print_doorbell_trace() {
  for (EvpServer* sv : g_servers) {
    const uint64_t n = sv ? sv->tr_n.load() : 0;
    if (!n) continue;
    fprintf(stderr,
            "{\"doorbell_trace\": {\"jobs\": %llu, \"us_slot_load\": %.2f, \"us_job\": %.2f, "
            "\"us_release\": %.2f, \"us_host_round_trip\": %.2f}}\n",
            (unsigned long long)n, sv->tr_load.load() * 0.01 / n, sv->tr_job.load() * 0.01 / n,
            sv->tr_rel.load() * 0.01 / n, sv->tr_host_ns.load() * 1e-3 / n);
    const uint64_t m = sv->tr_marks_n.load();
    if (m) {  // gcm_raw.h TG_JOB_MARK phases
      static const char* names[8] = {"tables+barrier", "parse", "ctr_setup", "blocks",
                                     "close+shoup", "reduce+barrier", "ek0_aes", "tag"};
      fprintf(stderr, "{\"doorbell_gcm_phases_us\": {\"jobs\": %llu", (unsigned long long)m);
      for (int i = 0; i < 8; i++) fprintf(stderr, ", \"%s\": %.2f", names[i], sv->tr_phase[i].load() * 0.01 / m);
      fprintf(stderr, ", \"since_loaded_us\": {\"wave0_blocks\": %.2f, \"wave0_shoup\": %.2f, "
                      "\"last_wave_blocks\": %.2f, \"last_wave_shoup\": %.2f}}}\n",
              sv->tr_last[0].load() * 0.01 / m, sv->tr_last[1].load() * 0.01 / m,
              sv->tr_last[2].load() * 0.01 / m, sv->tr_last[3].load() * 0.01 / m);
      if (const uint64_t ni = sv->tr_inst_n.load())
        fprintf(stderr, "{\"doorbell_install_us\": {\"jobs\": %llu, \"image_read\": %.2f, "
                        "\"tables_built\": %.2f}}\n", (unsigned long long)ni,
                sv->tr_inst[0].load() * 0.01 / ni, sv->tr_inst[1].load() * 0.01 / ni);
    }
  }
}

// A served job's device timestamps (TLSGPU_EVP_DOORBELL_TRACE) into the sums
// print_doorbell_trace prints; t0: the caller's post (host clock).
void EvpServer::account_trace(const DoorbellSlot* slot, uint64_t t0) {
  const uint64_t* tr = trace + kTraceWords * (size_t)(slot - slots);
  tr_n.fetch_add(1, std::memory_order_relaxed);
  tr_load.fetch_add(tr[1] - tr[0], std::memory_order_relaxed);
  tr_job.fetch_add(tr[9] - tr[1], std::memory_order_relaxed);
  tr_rel.fetch_add(tr[10] - tr[9], std::memory_order_relaxed);
  tr_host_ns.fetch_add(mono_ns() - t0, std::memory_order_relaxed);
  bool all = true;
  for (int i = 2; i < 9; i++) all = all && tr[i] >= tr[i - 1];
  if (all && tr[9] >= tr[8]) {
    tr_marks_n.fetch_add(1, std::memory_order_relaxed);
    for (int i = 0; i < 8; i++)
      tr_phase[i].fetch_add(tr[i + 2] - tr[i + 1], std::memory_order_relaxed);
    const uint64_t lw_b = tr[11] >= tr[1] ? tr[11] - tr[1] : 0, lw_s = tr[12] >= tr[1] ? tr[12] - tr[1] : 0;
    tr_last[0].fetch_add(tr[5] - tr[1], std::memory_order_relaxed);
    tr_last[1].fetch_add(tr[6] - tr[1], std::memory_order_relaxed);
    tr_last[2].fetch_add(lw_b, std::memory_order_relaxed);
    tr_last[3].fetch_add(lw_s, std::memory_order_relaxed);
    if (tr[13] >= tr[1] && tr[14] >= tr[13] && tr[13] != 0) {  // an install job (round 6)
      tr_inst_n.fetch_add(1, std::memory_order_relaxed);
      tr_inst[0].fetch_add(tr[13] - tr[1], std::memory_order_relaxed);
      tr_inst[1].fetch_add(tr[14] - tr[13], std::memory_order_relaxed);
    }
  }
}

// Launch an instance if the one queued last may stop polling within half a
// lifetime.  Returns false if the launch failed.
static bool server_ensure(EvpServer* sv) {
  const uint64_t now = mono_ns();
  if (now < sv->deadline_ns.load(std::memory_order_acquire)) return true;  // no lock per call
  std::lock_guard<std::mutex> lk(sv->mu);
  if (now < sv->deadline_ns.load(std::memory_order_relaxed)) return true;
  // the shutdown contract copies `outstanding` under this lock: nothing is
  // launched after it
  if (g_evp_shutdown.load(std::memory_order_acquire) != 0) return false;
  if (hipSetDevice(sv->device) != hipSuccess) return false;
  // forget instances that have left (the list stays a few entries long)
  sv->outstanding.erase(std::remove_if(sv->outstanding.begin(), sv->outstanding.end(),
                                       [sv](const std::pair<uint32_t, uint32_t>& i) {
                                         return instance_left(sv, i.first, i.second);
                                       }),
                        sv->outstanding.end());
  ServerArgs a;
  a.slots = sv->d_slots;
  // poll the slots handed out so far, rounded up to 16 (so that a burst of new
  // threads forces few relaunches): every poll is a PCIe read, and at 64
  // threads polling all 8 G slots was 8x the reads the calls needed
  const uint32_t hi = std::max(1u, sv->hi_slot.load(std::memory_order_acquire));
  a.nslots = std::min(sv->nslots, (hi + 15) & ~15u);
  a.stop = sv->d_stop;
  a.lifetime = sv->lifetime_ns / 10;  // 100 MHz realtime ticks
  a.trace = reinterpret_cast<unsigned long long*>(sv->d_trace);
  a.scrubs = reinterpret_cast<unsigned long long*>(sv->d_scrubs);
  a.exited = sv->d_stop + kExitedWord;
  a.seq = sv->launch_seq + 1;
  const uint32_t cover = (hi + kWave - 1) / kWave;
  const uint32_t g = std::min(sv->groups, std::max({1u, sv->active.load(std::memory_order_acquire), cover}));
  if (launch_evp_server(a, (int)g, sv->stream) != 0) return false;
  sv->launch_seq = a.seq;
  sv->last_g = g;
  sv->outstanding.emplace_back(a.seq, g);
  sv->covered.store(std::min(g * (uint32_t)kWave, a.nslots), std::memory_order_release);
  sv->last_launched_g.store(g, std::memory_order_release);
  // instances on one stream run one after another: this one starts when the
  // one queued before it ends (never before now) and polls for a lifetime
  // from then; post to it until half of that is left.  (Counting from the
  // launch instead queued a new instance every half lifetime behind ones
  // that each ran a whole lifetime: the queue grew without bound.)
  sv->end_ns = std::max(now, sv->end_ns) + sv->lifetime_ns;
  sv->deadline_ns.store(sv->end_ns - sv->lifetime_ns / 2, std::memory_order_release);
  sv->launches.fetch_add(1, std::memory_order_relaxed);
  return true;
}

constexpr uint32_t kScrubSweepBatch = 32;  // pending scrubs before an init sweeps
// Give back the session slots whose cleanup scrub has been answered; wait up to
// `wait_ns` for the others (relaunching the server when an instance left before
// picking a post up).  With `only`, just the entries of that (table, slot).
static void sweep_scrubs(EvpServer* sv, uint64_t wait_ns, const tlsgpu_sessions* only_t = nullptr,
                         uint32_t only_slot = 0) {
  const uint64_t t0 = mono_ns();
  for (;;) {
    bool left = false, overdue = false;
    {
      // no wait asked: another thread's sweep does the work (init and cleanup
      // of many threads must not queue on this lock)
      std::unique_lock<std::mutex> lk(sv->pend_mu, std::defer_lock);
      if (wait_ns == 0) {
        if (!lk.try_lock()) return;
      } else {
        lk.lock();
      }
      auto& v = sv->pending;
      for (size_t i = 0; i < v.size();) {
        const auto& e = v[i];
        if ((int32_t)(__atomic_load_n(&e.ds->done, __ATOMIC_ACQUIRE) - e.post) >= 0) {
          slab_give(e.evp_dev, e.sess, e.slot);
          v[i] = v.back();
          v.pop_back();
          sv->npending.fetch_sub(1, std::memory_order_relaxed);
          continue;
        }
        if (!only_t || (e.sess == only_t && e.slot == only_slot)) left = true;
        if (mono_ns() - e.t0 > 2000000ull) overdue = true;  // 2 ms: look at the server
        i++;
      }
    }
    // (no launch from an exit hook: HIP calls there race the runtime's teardown)
    if (overdue && g_evp_shutdown.load(std::memory_order_acquire) == 0 && g_exit_phase == 0)
      (void)server_ensure(sv);
    if (!left || mono_ns() - t0 >= wait_ns) return;
    __builtin_ia32_pause();
    sched_yield();
  }
}

extern "C" int tlsgpu_evp_shutdown(void) {
  std::lock_guard<std::mutex> lk(g_shutdown_mu);
  if (g_evp_shutdown.load(std::memory_order_acquire) == 2) return TLSGPU_OK;
  // cleanup scrubs still in flight are answered before the servers stop (up
  // to 2 s each server; they take microseconds)
  if (g_evp_shutdown.load(std::memory_order_acquire) == 0)
    for (EvpServer* sv : g_servers)
      if (sv && sv->slots && sv->npending.load(std::memory_order_relaxed) != 0)
        sweep_scrubs(sv, 2000000000ull);
  g_evp_shutdown.store(1, std::memory_order_seq_cst);
  for (EvpServer* sv : g_servers)
    if (sv && sv->stop) __atomic_store_n(sv->stop, 1u, __ATOMIC_SEQ_CST);
  const uint64_t t0 = mono_ns();
  bool noted = false;
  uint32_t waited = 0;
  for (EvpServer* sv : g_servers) {
    if (!sv || !sv->stop) continue;
    std::vector<std::pair<uint32_t, uint32_t>> pend;
    {
      // server_ensure checks g_evp_shutdown under this lock: no instance is
      // launched after this copy
      std::lock_guard<std::mutex> lk2(sv->mu);
      pend = sv->outstanding;
    }
    for (const auto& inst : pend) {
      waited++;
      while (!instance_left(sv, inst.first, inst.second)) {
        __builtin_ia32_pause();
        const uint64_t t = mono_ns() - t0;
        if (!noted && t > 1000000000ull) {
          fprintf(stderr,
                  "tlsgpu: waiting for doorbell server instance %u (%u workgroups) on device %d "
                  "to leave\n",
                  inst.first, inst.second, sv->device);
          noted = true;
        }
        if (t > g_shutdown_cap_ns)
          return fail(TLSGPU_ETIMEOUT,
                      "doorbell server instance %u on device %d still running after %llu ms",
                      inst.first, sv->device, (unsigned long long)(g_shutdown_cap_ns / 1000000));
      }
    }
    std::lock_guard<std::mutex> lk2(sv->mu);
    sv->outstanding.clear();
  }
  g_evp_shutdown.store(2, std::memory_order_release);
  if (g_shutdown_verbose)
    fprintf(stderr, "{\"evp_shutdown\": {\"instances_waited\": %u, \"ms\": %.3f}}\n", waited,
            (mono_ns() - t0) * 1e-6);
  print_doorbell_trace();
  return TLSGPU_OK;
}

// TLSGPU_CRASH_TRACE=1: a fatal signal prints the exit phase and a native
// backtrace before the default action (Python's faulthandler, when enabled
// after the library loaded, chains to this handler after its own dump).
// Async-signal-safe: fixed strings and a hand-rolled integer
// formatter through write(2); backtrace() was called once at install, so the
// unwinder (libgcc) is loaded before any fault and the handler does not
// dlopen or malloc.
static void write_str(const char* p) { (void)!write(2, p, strlen(p)); }
static void write_int(long v) {
  char d[24];
  int i = (int)sizeof d;
  const bool neg = v < 0;
  unsigned long u = neg ? 0ul - (unsigned long)v : (unsigned long)v;
  do {
    d[--i] = (char)('0' + u % 10);
    u /= 10;
  } while (u && i > 1);
  if (neg) d[--i] = '-';
  (void)!write(2, d + i, sizeof d - (size_t)i);
}
static void crash_report(int sig) {
  write_str("tlsgpu: fatal signal ");
  write_int(sig);
  write_str(" in exit phase ");
  write_int((long)g_exit_phase);
  write_str(" (0 running, 1 main-thread exit guard, 2 atexit, 3 library destructor)\n");
  void* fr[64];
  backtrace_symbols_fd(fr, backtrace(fr, 64), 2);
  signal(sig, SIG_DFL);
  raise(sig);
}
__attribute__((constructor)) static void install_crash_report() {
  if (!env_on("TLSGPU_CRASH_TRACE")) return;
  void* warm[2];
  (void)backtrace(warm, 2);  // loads the unwinder now, not inside the handler
  struct sigaction sa;
  memset(&sa, 0, sizeof sa);
  sa.sa_handler = crash_report;
  sa.sa_flags = SA_RESETHAND;
  for (int sig : {SIGSEGV, SIGBUS, SIGABRT, SIGILL, SIGFPE}) sigaction(sig, &sa, nullptr);
}

static void evp_shutdown_at_exit() {
  bool any = false;
  for (EvpServer* sv : g_servers) any = any || (sv && sv->stop);
  if (!any || tlsgpu_evp_shutdown() == TLSGPU_OK) return;
  fprintf(stderr, "tlsgpu: %s; leaving before the runtime's teardown (exit status 70)\n",
          tlsgpu_last_error());
  fflush(stderr);
  _exit(70);
}

// The main thread's own staging set is destroyed among its thread-local
// destructors at exit(), before the guard (constructed at load, so destroyed
// later): drain there first.
static void evp_shutdown_main_thread_exit() {
  if ((pid_t)syscall(SYS_gettid) != getpid()) return;
  g_exit_phase = 1;
  evp_shutdown_at_exit();
}

// Staging of exited threads, per device, for the next thread (round 5): a
// thread's exit makes no HIP call — hipFree / hipHostFree would synchronise
// the device, i.e. wait behind doorbell server instances that other threads
// keep relaunching, and at process exit they ran before the servers were
// stopped.  The buffers live until the runtime's teardown.
static std::mutex g_stage_pool_mu;
static std::vector<Staging*> g_stage_pool[kMaxDev];
struct StagingSet {
  Staging* by_dev[kMaxDev] = {};
  ~StagingSet() {
    // the main thread's staging goes at exit(): stop and drain the doorbell
    // servers first (shutdown contract)
    evp_shutdown_main_thread_exit();
    std::lock_guard<std::mutex> lk(g_stage_pool_mu);
    for (int d = 0; d < kMaxDev; d++)
      if (by_dev[d]) g_stage_pool[d].push_back(by_dev[d]);
  }
};
static thread_local StagingSet t_stages;

// This thread's staging for device `dev` (nullptr on a bad ordinal / no memory).
Staging* tg::stage_for(int dev) {
  if (dev < 0 || dev >= kMaxDev) return nullptr;
  Staging*& st = t_stages.by_dev[dev];
  if (!st) {
    std::lock_guard<std::mutex> lk(g_stage_pool_mu);
    if (!g_stage_pool[dev].empty()) {
      st = g_stage_pool[dev].back();
      g_stage_pool[dev].pop_back();
    }
  }
  // an exited thread's installs may have left images in its key areas
  // (ADVICE r05): zero the ones whose copies are done before reuse
  if (st && st->any_dirty_key_area()) st->sweep_key_areas();
  if (!st) st = new (std::nothrow) Staging();
  return st;
}

// The main thread's exit guard: armed by the library constructor when it runs
// on the main thread (LD_PRELOAD, or a dlopen from the main thread), so its
// destructor runs among the main thread's thread-local destructors, first
// thing in exit().
namespace {
struct MainExitGuard {
  ~MainExitGuard() {
    g_exit_phase = 1;
    evp_shutdown_at_exit();
  }
};
}  // namespace
__attribute__((constructor)) static void arm_main_exit_guard() {
  if ((pid_t)syscall(SYS_gettid) != getpid()) return;
  static thread_local MainExitGuard guard;
  (void)&guard;
}
__attribute__((destructor)) static void evp_shutdown_at_unload() {
  g_exit_phase = 3;
  evp_shutdown_at_exit();
}
static void evp_shutdown_atexit() {
  g_exit_phase = 2;
  evp_shutdown_at_exit();
}

// The server of EVP device k (created on first use when the doorbell is on).
EvpServer* tg::evp_server(size_t k, tlsgpu_engine* e) {
  if (!g_doorbell_groups || k >= (size_t)kMaxEvpDevices ||
      g_evp_shutdown.load(std::memory_order_acquire) != 0)
    return nullptr;
  if (EvpServer* ready = g_ready_servers[k].load(std::memory_order_acquire)) return ready;
  std::lock_guard<std::mutex> lk(g_server_mu);
  if (g_servers[k]) return g_servers[k]->slots ? g_servers[k] : nullptr;
  auto* sv = new (std::nothrow) EvpServer();
  if (!sv) return nullptr;
  g_servers[k] = sv;  // a failed setup stays registered (slots == nullptr): not retried
  sv->device = e->device;
  sv->groups = std::min(g_doorbell_groups, 256u);
  sv->nslots = sv->groups * kSlotsPerGroup;
  sv->lifetime_ns = (uint64_t)g_doorbell_ms * 1000000ull;
  DoorbellSlot* h = nullptr;
  uint32_t* stop = nullptr;
  if (hipSetDevice(e->device) != hipSuccess ||
      hipHostMalloc((void**)&h, sizeof(DoorbellSlot) * sv->nslots, hipHostMallocDefault) !=
          hipSuccess)
    return nullptr;
  memset(h, 0, sizeof(DoorbellSlot) * sv->nslots);
  // one pinned page: [0] the stop word, [kExitedWord + b] workgroup b's exit mark
  if (hipHostMalloc((void**)&stop, 4096, hipHostMallocDefault) != hipSuccess ||
      hipHostGetDevicePointer((void**)&sv->d_slots, h, 0) != hipSuccess ||
      hipHostGetDevicePointer((void**)&sv->d_stop, stop, 0) != hipSuccess ||
      hipStreamCreateWithFlags(&sv->stream, hipStreamNonBlocking) != hipSuccess ||
      hipMalloc((void**)&sv->d_scrubs, 8 * (kScrubRing + 2)) != hipSuccess ||
      hipMemset(sv->d_scrubs, 0, 8 * (kScrubRing + 2)) != hipSuccess) {
    (void)hipHostFree(h);
    if (stop) (void)hipHostFree(stop);
    return nullptr;
  }
  if (hipHostMalloc((void**)&sv->scrub_status, 4 * sv->nslots, hipHostMallocDefault) != hipSuccess ||
      hipHostGetDevicePointer((void**)&sv->d_scrub_status, sv->scrub_status, 0) != hipSuccess)
    sv->scrub_status = sv->d_scrub_status = nullptr;  // cleanup scrubs stay synchronous
  if (g_doorbell_trace &&
      (hipHostMalloc((void**)&sv->trace, 8 * kTraceWords * sv->nslots, hipHostMallocDefault) !=
           hipSuccess ||
       hipHostGetDevicePointer((void**)&sv->d_trace, sv->trace, 0) != hipSuccess))
    sv->trace = sv->d_trace = nullptr;
  memset(stop, 0, 4096);
  sv->stop = stop;
  for (uint32_t i = sv->nslots; i-- > 0;) sv->free_slots.push_back(i);
  sv->slots = h;
  static std::once_flag once;
  std::call_once(once, [] { atexit(evp_shutdown_atexit); });
  g_ready_servers[k].store(sv, std::memory_order_release);
  return sv;
}

// The calling thread's slot on a server (assigned on first use, given back
// when the thread exits); -1 when all are taken.
struct ThreadSlots {
  int slot[kMaxEvpDevices];
  uint32_t seq[kMaxEvpDevices];
  // a second slot for the thread's asynchronous cleanup scrubs (round 6): the
  // scrub runs while the thread's next call uses its own slot
  int scrub[kMaxEvpDevices];
  uint32_t scrub_seq[kMaxEvpDevices];
  ThreadSlots() {
    for (int& x : slot) x = -2;  // not asked yet
    for (int& x : scrub) x = -2;
  }
  ~ThreadSlots() {
    for (int k = 0; k < kMaxEvpDevices; k++) {
      if (!g_servers[k]) continue;
      std::lock_guard<std::mutex> lk(g_servers[k]->mu);
      if (slot[k] >= 0) {
        g_servers[k]->free_slots.push_back((uint32_t)slot[k]);
        g_servers[k]->active.fetch_sub(1, std::memory_order_release);
      }
      // a scrub slot with its last post still unanswered is not handed on
      // (its next owner would number from `done`): kept out of use
      if (scrub[k] >= 0) {
        g_servers[k]->active.fetch_sub(1, std::memory_order_release);
        if (__atomic_load_n(&g_servers[k]->slots[scrub[k]].done, __ATOMIC_ACQUIRE) == scrub_seq[k])
          g_servers[k]->free_slots.push_back((uint32_t)scrub[k]);
      }
    }
  }
};
static thread_local ThreadSlots t_slots;

DoorbellSlot* tg::thread_slot(EvpServer* sv, size_t k, uint32_t** seq) {
  int& s = t_slots.slot[k];
  if (s == -2) {
    std::lock_guard<std::mutex> lk(sv->mu);
    if (sv->free_slots.empty()) {
      s = -1;
    } else {
      s = (int)sv->free_slots.back();
      sv->free_slots.pop_back();
      sv->active.fetch_add(1, std::memory_order_release);
      if ((uint32_t)s + 1 > sv->hi_slot.load(std::memory_order_relaxed))
        sv->hi_slot.store((uint32_t)s + 1, std::memory_order_release);
      // a slot the queued instance does not poll: relaunch wider before the
      // first post (the caller's server_ensure follows)
      if ((uint32_t)s >= sv->covered.load(std::memory_order_acquire))
        sv->deadline_ns.store(0, std::memory_order_release);
      // continue the slot's numbering (an earlier thread may have used it)
      t_slots.seq[k] = __atomic_load_n(&sv->slots[s].done, __ATOMIC_ACQUIRE);
    }
  }
  if (s < 0) return nullptr;
  *seq = &t_slots.seq[k];
  return &sv->slots[s];
}

// The calling thread's scrub slot on a server (round 6; nullptr when none is
// free).  Its numbering continues from the slot's `done`, which equals its
// `post`: a slot is only ever handed on with no post outstanding.
static DoorbellSlot* thread_scrub_slot(EvpServer* sv, size_t k, uint32_t** seq) {
  int& s = t_slots.scrub[k];
  if (s == -2) {
    std::lock_guard<std::mutex> lk(sv->mu);
    if (sv->free_slots.empty()) {
      s = -1;
    } else {
      s = (int)sv->free_slots.back();
      sv->free_slots.pop_back();
      // counted as a caller: an instance then has a workgroup for it beside
      // the thread's own slot's (slot m is served by workgroup m mod G), so
      // the scrub runs while the thread's next call is served
      sv->active.fetch_add(1, std::memory_order_release);
      if ((uint32_t)s + 1 > sv->hi_slot.load(std::memory_order_relaxed))
        sv->hi_slot.store((uint32_t)s + 1, std::memory_order_release);
      if ((uint32_t)s >= sv->covered.load(std::memory_order_acquire) ||
          sv->active.load(std::memory_order_relaxed) > sv->last_launched_g.load(std::memory_order_relaxed))
        sv->deadline_ns.store(0, std::memory_order_release);
      t_slots.scrub_seq[k] = __atomic_load_n(&sv->slots[s].done, __ATOMIC_ACQUIRE);
    }
  }
  if (s < 0) return nullptr;
  *seq = &t_slots.scrub_seq[k];
  return &sv->slots[s];
}

// The part of a posted slot that says whose job it is and where its status
// goes (the caller writes the job itself, then posts).
void tg::doorbell_fill(DoorbellSlot* slot, const AeadState* st, uint32_t op, const void* d_status) {
  slot->op = op;
  slot->n_sessions = st->sess->capacity;
  slot->status = (uint64_t)d_status;
  slot->sessions = (uint64_t)st->sess->d_sess;
  slot->gcm_tables = (uint64_t)st->sess->d_gcm;
  slot->key_id = st->key_id;
}

void tg::doorbell_served(EvpServer* sv, const DoorbellSlot* slot, uint64_t t0) {
  sv->jobs.fetch_add(1, std::memory_order_relaxed);
  if (sv->trace) sv->account_trace(slot, t0);
}

// EVP_AEAD_CTX_cleanup's scrub posted without waiting (round 6, VERDICT r05
// next-round 6: one-thread connection setup): the job goes to the thread's
// scrub slot and the session slot stays out of the free list until the server
// has answered, so no new context can install into it first.  false: not
// posted (no server / scrub slot, or the previous scrub on it still running
// after 10 s) — the caller scrubs synchronously.
bool tg::doorbell_scrub_async(const AeadState* st) {
  if (st->batcher || !evp_zerocopy() || !doorbell_enabled() ||
      st->install_pending.load(std::memory_order_acquire))
    return false;
  tlsgpu_engine* e = st->sess->eng;
  EvpServer* sv = evp_server(st->evp_dev, e);
  if (!sv || !sv->scrub_status) return false;
  uint32_t* seq = nullptr;
  DoorbellSlot* ds = thread_scrub_slot(sv, st->evp_dev, &seq);
  if (!ds) return false;
  const uint64_t t0 = mono_ns();
  for (uint64_t spins = 1; __atomic_load_n(&ds->done, __ATOMIC_ACQUIRE) != *seq; spins++) {
    // the previous scrub on this slot (normally answered long ago)
    if (mono_ns() - t0 > 10000000000ull) return false;
    __builtin_ia32_pause();
    if ((spins & 255) == 0) {
      sweep_scrubs(sv, 0);  // relaunches the server if an instance left before picking it up
      sched_yield();
    }
  }
  if (!server_ensure(sv)) return false;
  const uint32_t idx = (uint32_t)(ds - sv->slots);
  sv->scrub_status[idx] = -1;
  doorbell_fill(ds, st, kDoorbellOpScrub << 8, sv->d_scrub_status + idx);
  memset(&ds->job, 0, sizeof(RawJob));
  ds->job.session = st->slot;
  const uint32_t n = ++*seq;
  {
    std::lock_guard<std::mutex> lk(sv->pend_mu);
    sv->pending.push_back({st->sess, st->slot, st->evp_dev, ds, n, mono_ns()});
    sv->npending.fetch_add(1, std::memory_order_relaxed);
  }
  __atomic_store_n(&ds->post, n, __ATOMIC_RELEASE);
  sv->jobs.fetch_add(1, std::memory_order_relaxed);
  return true;
}

// EVP_AEAD_CTX_init's look at device dk's answered scrubs (their slots back to
// the slab before it takes one); tlsgpu_sessions_debug_read's wait for a slot.
void tg::evp_sweep_scrubs_for(size_t dk) {
  if (dk >= (size_t)kMaxEvpDevices) return;
  EvpServer* sv = g_ready_servers[dk].load(std::memory_order_acquire);
  // answered scrubs' slots go back in batches: a sweep per init cost 16
  // calling threads ~10 us of lock hand-offs each (profiles/r06f_evp_churn)
  if (sv && sv->npending.load(std::memory_order_relaxed) >= kScrubSweepBatch) sweep_scrubs(sv, 0);
}
void tg::evp_wait_scrub_of(const tlsgpu_sessions* t, uint32_t slot) {
  for (size_t k = 0; k < (size_t)kMaxEvpDevices; k++) {
    EvpServer* sv = g_ready_servers[k].load(std::memory_order_acquire);
    if (sv && sv->npending.load(std::memory_order_relaxed) != 0)
      sweep_scrubs(sv, 10000000000ull, t, slot);
  }
}

extern "C" int tlsgpu_evp_set_doorbell(unsigned groups, unsigned lifetime_ms) {
  std::lock_guard<std::mutex> lk(g_server_mu);
  for (EvpServer* sv : g_servers)
    if (sv) return fail(TLSGPU_EINVAL, "the doorbell server is already set up");
  g_doorbell_groups = groups;
  if (lifetime_ms) g_doorbell_ms = lifetime_ms;
  return TLSGPU_OK;
}

extern "C" int tlsgpu_evp_doorbell_warm(void) {
  if (!g_doorbell_groups || g_evp_shutdown.load(std::memory_order_acquire) != 0) return TLSGPU_OK;
  for (size_t k = 0; k < evp_device_count() && k < (size_t)kMaxEvpDevices; k++) {
    tlsgpu_engine* e = evp_engine(k);
    EvpServer* sv = e ? evp_server(k, e) : nullptr;
    if (sv && !server_ensure(sv) && g_evp_shutdown.load() == 0)
      return fail(TLSGPU_EHIP, "doorbell server launch on EVP device %zu", k);
  }
  return TLSGPU_OK;
}

extern "C" int tlsgpu_evp_doorbell_stats(uint64_t* jobs, uint64_t* launches) {
  uint64_t j = 0, l = 0;
  for (EvpServer* sv : g_servers)
    if (sv) {
      j += sv->jobs.load();
      l += sv->launches.load();
    }
  if (jobs) *jobs = j;
  if (launches) *launches = l;
  return TLSGPU_OK;
}

extern "C" int tlsgpu_evp_doorbell_scrub_stats(uint64_t* scrubs, uint64_t* flushes) {
  uint64_t n = 0, f = 0;
  for (EvpServer* sv : g_servers)
    if (sv && sv->d_scrubs) {
      uint64_t w[2] = {0, 0};
      if (hipSetDevice(sv->device) != hipSuccess ||
          hipMemcpy(&w[0], sv->d_scrubs, 8, hipMemcpyDeviceToHost) != hipSuccess ||
          hipMemcpy(&w[1], sv->d_scrubs + 1 + kScrubRing, 8, hipMemcpyDeviceToHost) != hipSuccess)
        return fail(TLSGPU_EHIP, "scrub stats");
      n += w[0];
      f += w[1];
    }
  if (scrubs) *scrubs = n;
  if (flushes) *flushes = f;
  return TLSGPU_OK;
}

// Post the job written into `slot` (the caller's doorbell slot on server sv,
// EVP device k) and wait for its answer.  1: served; 0: not served and never
// will be (shutdown) — take the launched path; -1: failure, nothing posted
// (launch failed); -2: posted but no answer in 10 s (the job may still run:
// the slot is retired and the staging abandoned).
int tg::doorbell_post_wait(EvpServer* sv, DoorbellSlot* slot, uint32_t* seq, size_t k, Staging* stg,
                           uint64_t* t0_out) {
  if (!server_ensure(sv)) {
    if (g_evp_shutdown.load(std::memory_order_acquire) == 0) return -1;  // launch failed
    return 0;  // shutting down: nothing was posted
  }
  const uint32_t n = ++*seq;
  const uint64_t t0 = mono_ns();
  *t0_out = t0;
  if (g_test_post_delay_us) usleep(g_test_post_delay_us);  // test hook: a descheduled caller
  __atomic_store_n(&slot->post, n, __ATOMIC_RELEASE);
  for (uint64_t spins = 1; __atomic_load_n(&slot->done, __ATOMIC_ACQUIRE) != n; spins++) {
    __builtin_ia32_pause();
    if ((spins & 127) == 0) {
      // the instance the post was meant for may have left before the post
      // landed (this thread descheduled between server_ensure and the store
      // for more than half a lifetime): past the deadline, relaunch — the new
      // instance picks the post up
      const int sd = g_evp_shutdown.load(std::memory_order_acquire);
      if (sd == 0 && !server_ensure(sv) && g_evp_shutdown.load() == 0) return -1;
      if (sd == 2) {  // drained: no instance will ever serve it
        if (__atomic_load_n(&slot->done, __ATOMIC_ACQUIRE) == n) return 1;
        t_slots.slot[k] = -1;  // this thread posts no more
        return 0;
      }
      const uint64_t waited = mono_ns() - t0;
      if (waited > 10000000000ull) {  // 10 s: the device is gone
        // the post stays outstanding: retire the slot (never handed out
        // again) and leave the staging buffer to the job that may still run
        // (never freed, never reused)
        t_slots.slot[k] = -1;
        stg->abandon();
        return -2;
      }
      if (waited > g_doorbell_yield_ns) sched_yield();  // let other callers post
    }
  }
  return 1;
}

// EVP_AEAD_CTX_cleanup through the doorbell (round 5): a scrub job zeroes the
// slot on the device and the serving workgroup's LDS copies of this key,
// synchronously — no launch; the other server workgroups zero theirs when
// they next look at the scrub ring (round 6, evp_server.hip: before their
// next job, or within 16 idle polls).  false: no server / slot for this thread (the caller scrubs on a
// stream instead).
bool tg::doorbell_scrub(const AeadState* st) {
  if (st->batcher || !evp_zerocopy() || !doorbell_enabled() ||
      st->install_pending.load(std::memory_order_acquire))
    return false;
  tlsgpu_engine* e = st->sess->eng;
  EvpServer* sv = evp_server(st->evp_dev, e);
  uint32_t* seq = nullptr;
  DoorbellSlot* slot = sv ? thread_slot(sv, st->evp_dev, &seq) : nullptr;
  Staging* stg = slot ? stage_for(e->device) : nullptr;
  if (!stg || !stg->ensure(e->device, 64) || !stg->h_dev) return false;
  int32_t* status = reinterpret_cast<int32_t*>(stg->h_buf);
  *status = -1;
  doorbell_fill(slot, st, kDoorbellOpScrub << 8, stg->h_dev);
  memset(&slot->job, 0, sizeof(RawJob));
  slot->job.session = st->slot;
  uint64_t t0 = 0;
  return doorbell_post_wait(sv, slot, seq, st->evp_dev, stg, &t0) == 1 &&
         __atomic_load_n(status, __ATOMIC_ACQUIRE) == 0;
}

