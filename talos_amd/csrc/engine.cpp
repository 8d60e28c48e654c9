// engine.cpp — the batch C ABI of libtlsgpu.so (include/tlsgpu.h): error
// reporting, engines and session tables, GCM kernel selection and the tuning
// knobs, run_batch with tlsgpu_open_batch / tlsgpu_seal_batch, and the thin
// device helper API.  The other host units: host_paths.cpp (host-resident and
// wire paths), evp_aead.cpp, evp_doorbell.cpp, evp_queue.cpp, evp_cipher.cpp
// (the drop-in EVP surfaces), group.cpp, session_host.cpp, talos_hooks.cpp.
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

// Scratch of at least `bytes` for stream s (enlarging waits for the stream's
// earlier work, which may still read the old buffer).
// TLSGPU_PRE_POOL=1 (diagnostic): take the scratch from the stream-ordered
// pool instead, as round 1 first did; tools/pool_probe.hip and DESIGN.md §4.1
// explain why that is wrong on MI355X.
static const bool g_pre_pool = [] {
  const char* v = getenv("TLSGPU_PRE_POOL");
  return v && *v == '1';
}();

static void* pre_scratch(tlsgpu_engine* e, hipStream_t s, size_t bytes) {
  std::lock_guard<std::mutex> g(e->pre_mu);
  PreScratch* ps = nullptr;
  for (auto& kv : e->pre)
    if (kv.first == s) ps = &kv.second;
  if (!ps) {
    e->pre.emplace_back(s, PreScratch{});
    ps = &e->pre.back().second;
  }
  if (ps->cap < bytes) {
    if (ps->ptr) {
      if (hipStreamSynchronize(s) != hipSuccess) return nullptr;
      (void)hipFree(ps->ptr);
      ps->ptr = nullptr;
      ps->cap = 0;
    }
    const size_t cap = std::max(bytes, (size_t)1 << 20);
    if (hipMalloc(&ps->ptr, cap) != hipSuccess) return nullptr;
    ps->cap = cap;
  }
  return ps->ptr;
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
    t->have[params[i].aead] = true;
  }
  return TLSGPU_OK;
}

static int initial_gcm_impl() {
  const char* v = getenv("TLSGPU_GCM_IMPL");
  if (v && strcmp(v, "ttable") == 0) return TLSGPU_GCM_TTABLE;
  if (v && strcmp(v, "bitslice") == 0) return TLSGPU_GCM_BITSLICE;
  if (v && strcmp(v, "hybrid") == 0) return TLSGPU_GCM_HYBRID;
  if (v && strcmp(v, "fused") == 0) return TLSGPU_GCM_FUSED;
  if (v && strcmp(v, "queue") == 0) return TLSGPU_GCM_QUEUE;
  if (v && strcmp(v, "split") == 0) return TLSGPU_GCM_SPLIT;
  return TLSGPU_GCM_AUTO;
}
// The bitsliced / hybrid / fused GCM variants measured slower than the queue
// kernel; they are compiled only with `make EXPERIMENTAL=1`
// (-DTG_EXPERIMENTAL).  Without it, selecting them fails and the default stays.
#ifdef TG_EXPERIMENTAL
static constexpr bool kExperimental = true;
#else
static constexpr bool kExperimental = false;
#endif
static bool impl_built(int impl) {
  return impl == TLSGPU_GCM_QUEUE || impl == TLSGPU_GCM_TTABLE || impl == TLSGPU_GCM_SPLIT ||
         impl == TLSGPU_GCM_AUTO || kExperimental;
}
static std::atomic<int> g_gcm_impl{impl_built(initial_gcm_impl()) ? initial_gcm_impl()
                                                                 : (int)TLSGPU_GCM_AUTO};

extern "C" int tlsgpu_set_gcm_impl(int impl) {
  if (impl < TLSGPU_GCM_BITSLICE || impl > TLSGPU_GCM_AUTO)
    return fail(TLSGPU_EINVAL, "unknown gcm impl %d", impl);
  if (!impl_built(impl))
    return fail(TLSGPU_EINVAL, "gcm impl %d not built (make EXPERIMENTAL=1)", impl);
  g_gcm_impl.store(impl);
  return TLSGPU_OK;
}
extern "C" int tlsgpu_get_gcm_impl(void) { return g_gcm_impl.load(); }

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

// TLSGPU_WG_PER_CU (A/B): workgroups per CU.  Only one 16-wave workgroup fits
// a CU at a time (LDS), so k > 1 gives each CU k ranges in turn, handed out by
// the dispatcher as CUs free up: a CU that runs fast takes more of them.
static uint32_t wg_per_cu() {
  static const uint32_t v = [] {
    const char* e = getenv("TLSGPU_WG_PER_CU");
    const long k = e ? strtol(e, nullptr, 10) : 1;
    return (uint32_t)(k < 1 ? 1 : (k > 4 ? 4 : k));
  }();
  return v;
}
static int groups_for(const tlsgpu_engine* e, uint32_t n, uint32_t* per_group) {
  // one persistent 16-wave workgroup per CU, contiguous record ranges
  uint32_t groups = (uint32_t)e->num_cus * wg_per_cu();
  uint32_t min_per = 16;
  if ((uint64_t)groups * min_per > n) groups = (n + min_per - 1) / min_per;
  if (groups == 0) groups = 1;
  *per_group = (n + groups - 1) / groups;
  groups = (n + *per_group - 1) / *per_group;
  return (int)groups;
}

static uint32_t initial_bs_reserve() {
  const char* v = getenv("TLSGPU_BS_RESERVE");
  long r = v ? strtol(v, nullptr, 10) : 12;
  return (uint32_t)(r < 2 ? 2 : r);
}
static uint32_t g_bs_reserve = initial_bs_reserve();
// Diagnostic phase timing of the hybrid kernel (TLSGPU_PHASE_STATS=1): 32
// counters in device memory, read with tlsgpu_debug_phase_stats.
static unsigned long long* g_phase_stats = nullptr;
static int g_phase_stats_dev = -1;
extern "C" int tlsgpu_debug_phase_stats(tlsgpu_engine* e, unsigned long long* out32, int reset) {
  if (!e) return fail(TLSGPU_EINVAL, "null engine");
  HIPCHK(hipSetDevice(e->device));
  if (!g_phase_stats) {
    if (!env_on("TLSGPU_PHASE_STATS")) return fail(TLSGPU_EINVAL, "TLSGPU_PHASE_STATS not set");
    HIPCHK(hipMalloc((void**)&g_phase_stats, 64 * sizeof(unsigned long long)));
    HIPCHK(hipMemset(g_phase_stats, 0, 64 * sizeof(unsigned long long)));
    g_phase_stats_dev = e->device;
  }
  HIPCHK(hipDeviceSynchronize());
  if (out32) HIPCHK(hipMemcpy(out32, g_phase_stats, 32 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  if (reset) HIPCHK(hipMemset(g_phase_stats, 0, 64 * sizeof(unsigned long long)));
  return TLSGPU_OK;
}

// Diagnostic per-workgroup timing of the queue kernel (TLSGPU_WG_TIMES=1):
// {start, end, rlo, rhi} of each workgroup of the last queue launch, read with
// tlsgpu_debug_wg_times (s_memrealtime ticks, 100 MHz).
static unsigned long long* g_wg_times = nullptr;
static int g_wg_times_dev = -1;  // the first engine's device only
static unsigned long long* wg_times_for(const tlsgpu_engine* e) {
  static const bool on = env_on("TLSGPU_WG_TIMES");
  if (!on) return nullptr;
  static std::mutex mu;
  std::lock_guard<std::mutex> lk(mu);
  if (!g_wg_times && hipMalloc((void**)&g_wg_times, 4 * 1024 * sizeof(unsigned long long)) == hipSuccess) {
    (void)hipMemset(g_wg_times, 0, 4 * 1024 * sizeof(unsigned long long));
    g_wg_times_dev = e->device;
  }
  return e->device == g_wg_times_dev ? g_wg_times : nullptr;
}
extern "C" int tlsgpu_debug_wg_times(tlsgpu_engine* e, unsigned long long* out, unsigned groups) {
  if (!e || !out || groups > 1024) return fail(TLSGPU_EINVAL, "bad arguments");
  if (!g_wg_times) return fail(TLSGPU_EINVAL, "TLSGPU_WG_TIMES not set");
  HIPCHK(hipSetDevice(e->device));
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(out, g_wg_times, 4 * (size_t)groups * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  return TLSGPU_OK;
}

// Hybrid-kernel experiment flags (TLSGPU_HY_FLAGS, tlsgpu_internal.h).  Bit 2
// parks the waves of gcm_hy_kernel that are not bitsliced-pair waves, bit 4 the
// bitsliced-pair waves.  A setting that parks every wave of the kernel that
// runs leaves every record of the batch unprocessed: round 2's
// gpurun_out/b16ab2 ("workload seal failed for 65536 records") ran the queue
// kernel, whose waves (T-table and packed-bitsliced role alike, BSW = 0) all
// obey bit 2.  Refused here: the park bits are dropped with a warning.
static uint32_t sane_hy_flags(uint32_t f, int impl) {
  const uint32_t parks = impl == TLSGPU_GCM_HYBRID ? 6u : impl == TLSGPU_GCM_BITSLICE ? 4u : 2u;
  if ((f & parks) == parks) {
    static std::once_flag warned;
    std::call_once(warned, [f] {
      fprintf(stderr, "libtlsgpu: TLSGPU_HY_FLAGS=%#x would park every wave; ignoring the "
                      "park bits\n", f);
    });
    return f & ~6u;
  }
  return f;
}
static uint32_t g_hy_flags = (uint32_t)env_uint("TLSGPU_HY_FLAGS", 0, 0) & 15u;

// Queue kernel: records with n >= this take the packed bitsliced path
// (gcm_bs16.h); 0 = T-table only.  Env TLSGPU_BS16_MIN.
static uint32_t g_bs16_min = (uint32_t)env_uint("TLSGPU_BS16_MIN", 0, 0);

// Queue kernel: short-record packs (gcm_pack).  Env TLSGPU_PACK=0 turns them
// off, =1 keeps them on even when the caller hints NO_SHORT_RECORDS; unset
// (-1): on unless hinted off.
static int g_pack = []() {
  const char* v = getenv("TLSGPU_PACK");
  return v && *v ? (int)strtol(v, nullptr, 0) : -1;
}();

// Per-wave-session kernel (gcm_pw.hip): env TLSGPU_PWS=0 never, 1 always,
// unset = automatic (short session runs, tlsgpu_internal.h pws_selected).
static uint32_t g_pws = []() {
  const char* v = getenv("TLSGPU_PWS");
  if (!v || !*v) return 0u;
  return *v == '0' ? 1u : 2u;
}();

static const bool g_fused = env_not_off("TLSGPU_FUSED");
// Work-balanced ranges for the fused kernel (round 5, TLSGPU_BALANCE): 0 off
// (the default), 1 the pack variant (mixed record lengths), 2 always.  Equal
// record counts per workgroup leave the Zipf workload's slowest CU with 16 %
// more bytes than the mean, but a cut inside a session run costs both of its
// workgroups a table build, a plan and a run-end wait, and config D measured
// no faster with equal-work cuts.
static const uint32_t g_balance = (uint32_t)env_uint("TLSGPU_BALANCE", 0, 10);
// Whole-piece balance (round 5, TLSGPU_PIECES): 0 off, 1 the pack variant
// (mixed record lengths; the default), 2 always — each workgroup takes whole
// pieces (a session run inside one count range) from a list sorted by work,
// in snake order (gcm_queue.hip piece_sort_kernel), instead of its count
// range: config D +1.4 % same-box, B (uniform records) −1 % (the two plan
// launches), DESIGN.md §4.1c.
static const uint32_t g_pieces = (uint32_t)env_uint("TLSGPU_PIECES", 1, 10);
// ... and how near a session-run boundary a cut snaps to it, in 1/1024 of a
// workgroup's share of the work (TLSGPU_BALANCE_SNAP; 0: exact cuts)
static const uint32_t g_balance_snap = (uint32_t)env_uint("TLSGPU_BALANCE_SNAP", 0, 10);

int tg::run_batch(tlsgpu_sessions* t, const void* d_descs, uint32_t n, const uint8_t* d_in,
                  uint8_t* d_out, int32_t* d_status, hipStream_t s, bool seal, bool raw,
                  const Bounds* bounds, unsigned kinds, unsigned hints, tlsgpu_record* type_out) {
  if (hints == ~0u) hints = t->hints.load(std::memory_order_relaxed);
  bool have[kKinds];
  for (int k = 0; k < kKinds; k++) have[k] = t->have[k] && ((kinds >> k) & 1u);
  BatchArgs a = {};
  a.sessions = t->d_sess;
  a.gcm_tables = t->d_gcm;
  a.descs = d_descs;
  a.n = n;
  a.in = d_in;
  a.out = d_out;
  a.status = d_status;
  a.n_sessions = t->capacity;
  a.bs_reserve = g_bs_reserve;

  a.dbg = g_phase_stats;
  a.wg_times = wg_times_for(t->eng);
  // a TLS 1.3 table (its sessions are all TLS 1.3): the kernels compiled for
  // that record layout, T-table record paths only (the packed bitsliced role
  // and the experimental kernels know the TLS 1.2 layout alone)
  const bool t13 = !raw && t->generation == 13;
  a.tls13 = t13 ? 1u : 0u;  // the launchers forward to the TLS 1.3 kernels and the unpad pass
  a.type_out = t13 && !seal ? type_out : nullptr;
  a.bs16_min = t13 ? 0u : g_bs16_min;
  // batch-shape hints rule out the kernels the device would not select
  // (tlsgpu_sessions_hint); the TLSGPU_PACK / TLSGPU_PWS overrides win
  a.pack = g_pack >= 0 ? (uint32_t)g_pack : (hints & TLSGPU_HINT_NO_SHORT_RECORDS) ? 0u : 1u;
  a.pws = (g_pws == 0 && (hints & TLSGPU_HINT_SESSION_RUNS)) ? 1u : g_pws;
  int groups = groups_for(t->eng, n, &a.records_per_group);
  int sel_impl = g_gcm_impl.load();
  if (t13 && (sel_impl == TLSGPU_GCM_HYBRID || sel_impl == TLSGPU_GCM_BITSLICE ||
                    sel_impl == TLSGPU_GCM_FUSED))
    sel_impl = TLSGPU_GCM_QUEUE;  // the experimental kernels: TLS 1.2 tables only
  // small TLS batches (at most two records per CU): one record per workgroup,
  // its blocks split over the 16 waves, instead of one wave per record
  // (measured crossover, 16 KiB records: split 47 vs 77 us at 512 records,
  // 93 vs 81 us at 1,024)
  const bool split = !raw && (sel_impl == TLSGPU_GCM_SPLIT ||
                              (sel_impl == TLSGPU_GCM_AUTO && n <= 2u * (uint32_t)t->eng->num_cus));
  if (raw || split) {
    // raw EVP jobs: latency, not throughput — one workgroup per job, so a
    // batch of jobs on different contexts runs side by side instead of one
    // session run (table rebuild) after another inside one workgroup
    a.records_per_group = 1;
    groups = (int)n;
  }
  const int impl = raw ? TLSGPU_GCM_TTABLE
                       : split ? TLSGPU_GCM_SPLIT
                       : sel_impl == TLSGPU_GCM_AUTO ? TLSGPU_GCM_QUEUE : sel_impl;
  a.hy_flags = sane_hy_flags(g_hy_flags, impl);
  const bool gcm_pre = impl != TLSGPU_GCM_TTABLE && impl != TLSGPU_GCM_SPLIT &&
                       (have[TLSGPU_AES_128_GCM] || have[TLSGPU_AES_256_GCM]);
  // Fused (round 5): one queue kernel is the batch's only kernel — one AES key
  // size installed, no ChaCha, the hints rule out the per-wave-session kernel,
  // and they decide the variant (TLSGPU_HINT_NO_SHORT_RECORDS: no-pack, else
  // the pack variant, which also runs long records) — so it checks bounds,
  // writes the initial statuses and computes the per-record constants of its
  // own records in its prologue: no check_record_bounds, no gcm_prep_kernel, no
  // checked-descriptor copy, no variant that exits at once (TLSGPU_FUSED=0
  // keeps the launch sequence with the device-side selection).
  const bool fused_gcm = g_fused && bounds && impl == TLSGPU_GCM_QUEUE && a.pws == 1 &&
                         (have[TLSGPU_AES_128_GCM] != have[TLSGPU_AES_256_GCM]) &&
                         !have[TLSGPU_CHACHA20_POLY1305] && !have[TLSGPU_CHACHA20_POLY1305_OLD] &&
                         !have[TLSGPU_CHACHA20_POLY1305_TLS13];
  // ... and the same for a batch of RFC 7539 ChaCha sessions only, or of a TLS 1.3
  // table whose only kind is the TLS 1.3 ChaCha one: the staged ChaCha kernel
  // checks bounds and writes the statuses of the records it does not run itself
  // (chacha_kernels.hip cc_tls_wave).  have_cc: the staged kernel's suite, RFC 7905
  // or, in a TLS 1.3 table, the TLS 1.3 kind
  const bool have_cc = t13 ? have[TLSGPU_CHACHA20_POLY1305_TLS13] : have[TLSGPU_CHACHA20_POLY1305];
  const bool fused_cc = g_fused && bounds && !raw && have_cc &&
                        !have[t13 ? TLSGPU_CHACHA20_POLY1305 : TLSGPU_CHACHA20_POLY1305_TLS13] &&
                        !have[TLSGPU_CHACHA20_POLY1305_OLD] && !have[TLSGPU_AES_128_GCM] &&
                        !have[TLSGPU_AES_256_GCM];
  const bool fused = fused_gcm || fused_cc;
  // per-stream scratch: [RecPre x n (queue kernels) | ctl_bytes control words |
  // checked descriptors x n].  Control words per key size k (0: AES-128, 1:
  // AES-256): selection words (kSelSlots x 64 B) at 1024 k, then one uint32
  // record counter per workgroup of the per-wave-session kernel at
  // 2048 + k * cnt_bytes, sized from the grid (any CU count).
  static_assert(kSelSlots * kSelWords * 4 <= 1024, "selection words exceed their slot");
  const size_t cnt_bytes = ((size_t)groups * 4 + 255) & ~(size_t)255;
  const size_t ctl_bytes = 2048 + 2 * cnt_bytes;
  const bool balance = fused_gcm && groups > 1 && groups <= 1024 &&
                       (g_balance >= 2 || (g_balance == 1 && a.pack != 0));
  const bool pieces = fused_gcm && !balance && groups > 1 && groups <= 1024 &&
                      (g_pieces >= 2 || (g_pieces == 1 && a.pack != 0));
  const size_t cut_bytes = balance  ? ((size_t)groups * 8 + 255) & ~(size_t)255
                           : pieces ? ((kPieceScratchBytes((uint32_t)groups) + 255) & ~(size_t)255) + 256
                                    : 0;
  const size_t pre_bytes =
      gcm_pre ? sizeof(RecPre) * (size_t)n + (fused ? cut_bytes : ctl_bytes) : 0;
  uint8_t* scratch = nullptr;
  uint8_t* pool_scratch = nullptr;
  if (pre_bytes || (bounds && !fused)) {
    const size_t sbytes = pre_bytes + (bounds && !fused ? sizeof(tlsgpu_record) * (size_t)n : 0);
    if (g_pre_pool) {  // diagnostic only (DESIGN.md §4.1 pool scratch): stream-ordered pool
      if (hipMallocAsync((void**)&scratch, sbytes, s) != hipSuccess) scratch = nullptr;
      pool_scratch = scratch;
    } else {
      scratch = (uint8_t*)pre_scratch(t->eng, s, sbytes);
    }
    if (!scratch) return fail(TLSGPU_ENOMEM, "batch scratch (%u records)", n);
  }
  RecPre* pre = nullptr;  // per-record constants of the queue kernels (per-stream scratch)
  uint8_t* ctl = nullptr;
  if (gcm_pre) {
    pre = reinterpret_cast<RecPre*>(scratch);
    ctl = fused ? nullptr : reinterpret_cast<uint8_t*>(pre + n);
  }
  uint8_t* const ctl_zero = impl == TLSGPU_GCM_QUEUE ? ctl : nullptr;
  if (fused) {
    a.fused = 1;
    a.in_bytes = bounds->in_bytes;
    a.out_bytes = bounds->out_bytes;
    if (balance) {  // each count range's work, then the kernel cuts at equal work
      auto* cw = reinterpret_cast<unsigned long long*>(pre + n);
      if (launch_range_work(a, groups, cw, s))
        return fail(TLSGPU_EHIP, "range work launch: %s", hipGetErrorString(hipGetLastError()));
      a.cut_work = cw;
      a.cut_snap = g_balance_snap;
    } else if (pieces) {  // whole pieces sorted by work
      uint8_t* ps = reinterpret_cast<uint8_t*>(pre + n);
      ps += (256 - ((uintptr_t)ps & 255)) & 255;
      if (launch_piece_plan(a, groups, ps, &a.pieces, &a.n_pieces, s))
        return fail(TLSGPU_EHIP, "piece plan launch: %s", hipGetErrorString(hipGetLastError()));
    }
  } else if (bounds) {
    // one setup launch: sanitized descriptors, every record's initial status
    // (records whose session is empty / invalid keep TLSGPU_REC_PUBLIC_INVALID)
    // and the zeroed control words
    auto* safe = reinterpret_cast<tlsgpu_record*>(scratch + pre_bytes);
    if (launch_check_bounds(reinterpret_cast<const tlsgpu_record*>(d_descs), safe, n, t->d_sess,
                            t->capacity, bounds->in_bytes, bounds->out_bytes, seal, d_status,
                            reinterpret_cast<uint32_t*>(ctl_zero),
                            ctl_zero ? (uint32_t)(ctl_bytes / 4) : 0u, s))
      return fail(TLSGPU_EHIP, "bounds launch: %s", hipGetErrorString(hipGetLastError()));
    a.descs = safe;
  } else {
    // records whose session is empty / invalid keep this status (raw EVP
    // jobs: the raw kernels write it themselves, so a queue batch launches no
    // fill kernel — round 2 measured ~18 K of them per queue run)
    if (!raw) HIPCHK(hipMemsetD32Async((hipDeviceptr_t)d_status, (int)TLSGPU_REC_PUBLIC_INVALID, n, s));
    if (ctl_zero) HIPCHK(hipMemsetAsync(ctl_zero, 0, ctl_bytes, s));
  }
  for (int rounds : {10, 14}) {
    if (!have[rounds == 10 ? TLSGPU_AES_128_GCM : TLSGPU_AES_256_GCM]) continue;
    // selection words and counters per key size: a short AES-128 record must
    // not send the AES-256 pass to the pack variant
    if (ctl && impl == TLSGPU_GCM_QUEUE) {
      const int k = rounds == 10 ? 0 : 1;
      a.sel = reinterpret_cast<uint32_t*>(ctl + 1024 * k);
      a.wg_next = reinterpret_cast<uint32_t*>(ctl + 2048 + cnt_bytes * k);
    }
    int rc;
    if (impl == TLSGPU_GCM_TTABLE) {
      rc = launch_gcm(a, seal, raw, rounds, groups, s);
    } else if (impl == TLSGPU_GCM_SPLIT) {
      rc = launch_gcm_split(a, seal, rounds, s);
    } else {
      rc = fused ? 0 : launch_gcm_prep(a, pre, seal, rounds, s);
      if (rc == 0) {
        if (impl == TLSGPU_GCM_QUEUE)
          rc = launch_gcm_queue(a, pre, seal, rounds, groups, s);
#ifdef TG_EXPERIMENTAL
        else if (impl == TLSGPU_GCM_FUSED)
          rc = (rounds == 10 ? launch_gcm_fused10 : launch_gcm_fused14)(a, pre, seal, groups, s);
        else
          rc = (rounds == 10 ? launch_gcm_hy10 : launch_gcm_hy14)(
              a, pre, seal, impl == TLSGPU_GCM_HYBRID ? 4 : 8, groups, s);
#else
        else
          rc = -1;
#endif
      }
    }
    if (rc) {
      return fail(TLSGPU_EHIP, "gcm-%d launch: %s", rounds == 10 ? 128 : 256,
                  hipGetErrorString(hipGetLastError()));
    }
  }
  // (a TLS 1.3 table: launch_chacha also runs the ChaCha sessions' unpad pass after an open)
  if ((have_cc || have[TLSGPU_CHACHA20_POLY1305_OLD]) &&
      launch_chacha(a, seal, raw, have_cc, have[TLSGPU_CHACHA20_POLY1305_OLD], s))
    return fail(TLSGPU_EHIP, "chacha launch: %s", hipGetErrorString(hipGetLastError()));
  if (pool_scratch) HIPCHK(hipFreeAsync(pool_scratch, s));
  return TLSGPU_OK;
}

extern "C" int tlsgpu_sessions_hint(tlsgpu_sessions* t, unsigned hints) {
  if (!t || (hints & ~(TLSGPU_HINT_NO_SHORT_RECORDS | TLSGPU_HINT_SESSION_RUNS)))
    return fail(TLSGPU_EINVAL, "bad arguments");
  t->hints.store(hints, std::memory_order_relaxed);
  return TLSGPU_OK;
}

extern "C" int tlsgpu_open_batch(tlsgpu_sessions* t, const tlsgpu_record* d_recs, uint32_t n,
                                 const uint8_t* d_in, size_t in_bytes, uint8_t* d_out,
                                 size_t out_bytes, int32_t* d_status, void* stream) {
  if (!t || (n && (!d_recs || !d_in || !d_out || !d_status)))
    return fail(TLSGPU_EINVAL, "bad arguments");
  if (n == 0) return TLSGPU_OK;
  HIPCHK(hipSetDevice(t->eng->device));
  const Bounds b = {in_bytes, out_bytes};
  return run_batch(t, d_recs, n, d_in, d_out, d_status,
                   stream ? (hipStream_t)stream : t->eng->stream, false, false, &b);
}

extern "C" int tlsgpu_seal_batch(tlsgpu_sessions* t, const tlsgpu_record* d_recs, uint32_t n,
                                 const uint8_t* d_in, size_t in_bytes, uint8_t* d_out,
                                 size_t out_bytes, int32_t* d_status, void* stream) {
  if (!t || (n && (!d_recs || !d_in || !d_out || !d_status)))
    return fail(TLSGPU_EINVAL, "bad arguments");
  if (n == 0) return TLSGPU_OK;
  HIPCHK(hipSetDevice(t->eng->device));
  const Bounds b = {in_bytes, out_bytes};
  return run_batch(t, d_recs, n, d_in, d_out, d_status,
                   stream ? (hipStream_t)stream : t->eng->stream, true, false, &b);
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
