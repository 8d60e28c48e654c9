// batch.cpp — batch dispatch: every path of the engine reaches the GPU through
// tg::run_batch (tlsgpu_open_batch / tlsgpu_seal_batch here, the host-resident
// and wire paths of host_paths.cpp, the group split, the EVP coalescing queue).
// In order: the batch knobs (one struct, read once), the GCM implementation
// switch, the two debug facilities that only fill BatchArgs, plan_batch (a pure
// function: what to launch and where everything lies in the scratch), run_batch
// (gets the scratch and issues the plan) and the two batch entry points.
// DESIGN.md §4.15; tests/test_batch_plan_trace.py pins every decision on a CPU.
#include "host_internal.h"

using namespace tg;

// ---------------------------------------------------------------------------
// The batch-path environment knobs, read once (ChaCha's own A/B switches:
// chacha_kernels.hip launch_chacha).
struct BatchKnobs {
  // TLSGPU_PRE_POOL=1 (diagnostic): take the scratch from the stream-ordered
  // pool instead of the per-stream grow-only buffer, as round 1 first did;
  // tools/pool_probe.hip and DESIGN.md §4.1 explain why that is wrong on MI355X.
  bool pre_pool = env_starts("TLSGPU_PRE_POOL", '1');
  // TLSGPU_WG_PER_CU (A/B): workgroups per CU, 1..4.  Only one 16-wave workgroup
  // fits a CU at a time (LDS), so k > 1 gives each CU k ranges in turn, handed
  // out by the dispatcher as CUs free up: a CU that runs fast takes more of them.
  uint32_t wg_per_cu =
      (uint32_t)std::clamp<int64_t>((int64_t)env_uint("TLSGPU_WG_PER_CU", 1, 10), 1, 4);
  // TLSGPU_BS_RESERVE: BatchArgs::bs_reserve (hybrid kernel), at least 2
  // (set and empty reads as 0, as it always has)
  uint32_t bs_reserve = (uint32_t)std::max<int64_t>(
      env_starts("TLSGPU_BS_RESERVE", '\0') ? 0 : (int64_t)env_uint("TLSGPU_BS_RESERVE", 12, 10), 2);
  // Hybrid-kernel experiment flags (TLSGPU_HY_FLAGS, tlsgpu_internal.h), before
  // sane_hy_flags below.
  uint32_t hy_flags = (uint32_t)env_uint("TLSGPU_HY_FLAGS", 0, 0) & 15u;
  // Queue kernel: records with n >= this take the packed bitsliced path
  // (gcm_bs16.h); 0 = T-table only.  Env TLSGPU_BS16_MIN.
  uint32_t bs16_min = (uint32_t)env_uint("TLSGPU_BS16_MIN", 0, 0);
  // Queue kernel: short-record packs (gcm_pack).  Env TLSGPU_PACK=0 turns them
  // off, =1 keeps them on even when the caller hints NO_SHORT_RECORDS; unset
  // (-1): on unless hinted off.
  int pack = (int)env_uint("TLSGPU_PACK", ~0ull, 0);
  // Per-wave-session kernel (gcm_pw.hip): env TLSGPU_PWS=0 never (1), anything
  // else always (2), unset (0) = automatic (short session runs,
  // tlsgpu_internal.h pws_selected).
  uint32_t pws = !env_not_off("TLSGPU_PWS") ? 1u : env_on("TLSGPU_PWS") ? 2u : 0u;
  // TLSGPU_FUSED=0 keeps the launch sequence with the device-side selection
  // instead of the fused single-kernel batches (plan_batch fused_gcm / fused_cc).
  bool fused = env_not_off("TLSGPU_FUSED");
  // TLSGPU_CHACHA_LEGACY=1 (launch_chacha): TLS 1.2 ChaCha batches run on the
  // per-lane kernel, which has no bounds rule and writes no initial statuses of
  // its own, so such a batch is never fused.
  bool cc_legacy = env_on("TLSGPU_CHACHA_LEGACY");
  // Work-balanced ranges for the fused kernel (round 5, TLSGPU_BALANCE): 0 off
  // (the default), 1 the pack variant (mixed record lengths), 2 always.  Equal
  // record counts per workgroup leave the Zipf workload's slowest CU with 16 %
  // more bytes than the mean, but a cut inside a session run costs both of its
  // workgroups a table build, a plan and a run-end wait, and config D measured
  // no faster with equal-work cuts.
  uint32_t balance = (uint32_t)env_uint("TLSGPU_BALANCE", 0, 10);
  // Whole-piece balance (round 5, TLSGPU_PIECES): 0 off, 1 the pack variant
  // (mixed record lengths; the default), 2 always — each workgroup takes whole
  // pieces (a session run inside one count range) from a list sorted by work,
  // in snake order (gcm_queue.hip piece_sort_kernel), instead of its count
  // range: config D +1.4 % same-box, B (uniform records) −1 % (the two plan
  // launches), DESIGN.md §4.1c.
  uint32_t pieces = (uint32_t)env_uint("TLSGPU_PIECES", 1, 10);
  // ... and how near a session-run boundary a cut snaps to it, in 1/1024 of a
  // workgroup's share of the work (TLSGPU_BALANCE_SNAP; 0: exact cuts)
  uint32_t balance_snap = (uint32_t)env_uint("TLSGPU_BALANCE_SNAP", 0, 10);
  // Diagnostic per-workgroup timing of the queue kernel (TLSGPU_WG_TIMES=1),
  // read with tlsgpu_debug_wg_times.
  bool wg_times = env_on("TLSGPU_WG_TIMES");
};
static const BatchKnobs& knobs() {
  static const BatchKnobs k{};
  return k;
}

// TLSGPU_HY_FLAGS bit 2 parks the waves of gcm_hy_kernel that are not
// bitsliced-pair waves, bit 4 the bitsliced-pair waves.  A setting that parks
// every wave of the kernel that runs leaves every record of the batch
// unprocessed: round 2's b16ab2 run ("workload seal failed for 65536
// records") ran the queue kernel, whose waves (T-table and packed-bitsliced
// role alike, BSW = 0) all obey bit 2.  Refused here: the park bits are dropped
// (run_batch warns once).
static uint32_t sane_hy_flags(uint32_t f, int impl) {
  const uint32_t parks = impl == TLSGPU_GCM_HYBRID ? 6u : impl == TLSGPU_GCM_BITSLICE ? 4u : 2u;
  return (f & parks) == parks ? f & ~6u : f;
}

// ---------------------------------------------------------------------------
// the GCM implementation switch: a runtime atomic seeded from TLSGPU_GCM_IMPL
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

extern "C" int tlsgpu_sessions_hint(tlsgpu_sessions* t, unsigned hints) {
  if (!t || (hints & ~(TLSGPU_HINT_NO_SHORT_RECORDS | TLSGPU_HINT_SESSION_RUNS)))
    return fail(TLSGPU_EINVAL, "bad arguments");
  t->hints.store(hints, std::memory_order_relaxed);
  return TLSGPU_OK;
}

// ---------------------------------------------------------------------------
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
  if (!knobs().wg_times) return nullptr;
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

// ---------------------------------------------------------------------------
// the plan

// Per-stream scratch of one batch: byte counts, and byte offsets from its base
// (256-B aligned: hipMalloc).  Two layouts:
//   launch sequence  [RecPre x n | control words | checked descriptors x n]
//   fused_gcm        [RecPre x n | cut work (balance) or piece plan (pieces)]
// RecPre and what follows it exist only when a queue-family kernel runs
// (gcm_pre), the checked descriptors only for a caller's batch (bounds) that is
// not fused; a fused ChaCha batch needs no scratch at all (total 0).
// Control words (ctl_bytes of them, zeroed by the setup launch), per key size
// k (0: AES-128, 1: AES-256): the selection words (kSelSlots x 64 B) at
// sel[k] = ctl + 1024 k, then one uint32 record counter per workgroup of the
// per-wave-session kernel at wg_next[k] = ctl + 2048 + k * cnt_bytes, sized
// from the grid (any CU count).  The cut work is one uint64 per workgroup right
// behind RecPre; the piece plan (kPieceScratchBytes) starts at the next 256-B
// boundary and its size carries 256 B of slack for that.
struct ScratchLayout {
  size_t total;           // 0: no scratch
  size_t pre;             // RecPre x n (always 0)
  size_t ctl, ctl_bytes;  // control words
  size_t cnt_bytes;       // ... their per-key-size counter block
  size_t sel[2], wg_next[2];
  size_t cut, cut_bytes;  // cut work or piece plan
  size_t safe;            // checked descriptors
};
static_assert(kSelSlots * kSelWords * 4 <= 1024, "selection words exceed their slot");

struct PlanInput {
  uint32_t n;
  int num_cus;
  bool have[kKinds];  // kind k is installed AND in the caller's kinds mask
  int generation;     // of the table: 12 / 13
  bool cc_padded;     // the table holds a TLS 1.3 ChaCha session with a padding block
  bool seal, raw;
  bool bounds;        // a caller's batch: {in_bytes, out_bytes} to check against
  uint64_t in_bytes, out_bytes;
  bool type_out;      // the caller gave writable descriptors for the inner types
  unsigned hints;     // resolved (the call's, else the table's)
  int impl;           // selected (g_gcm_impl)
  const BatchKnobs& knobs;
};

enum class Setup {
  kFused,        // the one kernel's own prologue (after the range-work / piece-plan launch)
  kCheckBounds,  // launch_check_bounds: checked descriptors, statuses, zeroed control words
  kMemset,       // the engine's own descriptors: status fill (not raw) + control-word memset
};

struct BatchPlan {
  // the implementation that runs the GCM records, and its grid
  int impl;  // TLSGPU_GCM_TTABLE / _SPLIT / _QUEUE, or an experimental one
  int groups;  // (args.records_per_group records each)
  // the GCM passes: per key size (0: AES-128, 1: AES-256), and whether they
  // are queue-family kernels that read RecPre (prep pass unless fused)
  bool pass[2];
  bool gcm_pre;
  bool use_ctl;  // the queue impl's control words: zeroed by the setup, sel / wg_next per pass
  // the ChaCha launch: the staged kernel's suite / the draft suite
  bool cc_rfc, cc_old;
  // the setup
  Setup setup;
  bool fused_gcm, fused_cc, balance, pieces;
  bool type_out;
  // the scalar BatchArgs fields, in place (n, records_per_group, tls13,
  // bs16_min, pack, pws, hy_flags, fused, in_bytes / out_bytes, bs_reserve; the
  // pointers are run_batch's), and cut_snap, which goes in after the range-work
  // launch
  BatchArgs args;
  uint32_t cut_snap;
  ScratchLayout layout;
};

static int groups_for(int num_cus, uint32_t wg_per_cu, uint32_t n, uint32_t* per_group) {
  // one persistent 16-wave workgroup per CU, contiguous record ranges
  uint32_t groups = (uint32_t)num_cus * wg_per_cu;
  uint32_t min_per = 16;
  if ((uint64_t)groups * min_per > n) groups = (n + min_per - 1) / min_per;
  if (groups == 0) groups = 1;
  *per_group = (n + groups - 1) / groups;
  groups = (n + *per_group - 1) / *per_group;
  return (int)groups;
}

static size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

// Everything run_batch decides.  Pure: no HIP call, no allocation, no global.
static BatchPlan plan_batch(const PlanInput& in) {
  const BatchKnobs& k = in.knobs;
  const bool* have = in.have;
  const bool aes128 = have[TLSGPU_AES_128_GCM], aes256 = have[TLSGPU_AES_256_GCM];
  BatchPlan p = {};
  p.args.n = in.n;
  // a TLS 1.3 table (its sessions are all TLS 1.3): the kernels compiled for
  // that record layout, T-table record paths only (the packed bitsliced role
  // and the experimental kernels know the TLS 1.2 layout alone)
  const bool t13 = !in.raw && in.generation == 13;
  p.args.tls13 = t13 ? 1u : 0u;  // the launchers forward to the TLS 1.3 kernels and the unpad pass
  p.type_out = t13 && !in.seal && in.type_out;
  p.args.cc_pad = t13 && in.seal && in.cc_padded ? 1u : 0u;  // launch_chacha: the PAD kernel
  p.args.bs16_min = t13 ? 0u : k.bs16_min;
  p.args.bs_reserve = k.bs_reserve;
  // batch-shape hints rule out the kernels the device would not select
  // (tlsgpu_sessions_hint); the TLSGPU_PACK / TLSGPU_PWS overrides win
  p.args.pack = k.pack >= 0 ? (uint32_t)k.pack : (in.hints & TLSGPU_HINT_NO_SHORT_RECORDS) ? 0u : 1u;
  p.args.pws = (k.pws == 0 && (in.hints & TLSGPU_HINT_SESSION_RUNS)) ? 1u : k.pws;

  // --- the implementation and its grid
  if (in.raw) {
    p.impl = TLSGPU_GCM_TTABLE;
  } else if (in.impl == TLSGPU_GCM_SPLIT ||
             (in.impl == TLSGPU_GCM_AUTO && in.n <= 2u * (uint32_t)in.num_cus)) {
    // small TLS batches (at most two records per CU): one record per workgroup,
    // its blocks split over the 16 waves, instead of one wave per record
    // (measured crossover, 16 KiB records: split 47 vs 77 us at 512 records,
    // 93 vs 81 us at 1,024)
    p.impl = TLSGPU_GCM_SPLIT;
  } else if (in.impl == TLSGPU_GCM_AUTO) {
    p.impl = TLSGPU_GCM_QUEUE;
  } else if (t13 && (in.impl == TLSGPU_GCM_HYBRID || in.impl == TLSGPU_GCM_BITSLICE ||
                     in.impl == TLSGPU_GCM_FUSED)) {
    p.impl = TLSGPU_GCM_QUEUE;  // the experimental kernels: TLS 1.2 tables only
  } else {
    p.impl = in.impl;
  }
  if (in.raw || p.impl == TLSGPU_GCM_SPLIT) {
    // raw EVP jobs: latency, not throughput — one workgroup per job, so a
    // batch of jobs on different contexts runs side by side instead of one
    // session run (table rebuild) after another inside one workgroup
    p.args.records_per_group = 1;
    p.groups = (int)in.n;
  } else {
    p.groups = groups_for(in.num_cus, k.wg_per_cu, in.n, &p.args.records_per_group);
  }
  p.args.hy_flags = sane_hy_flags(k.hy_flags, p.impl);

  // --- the launches
  p.pass[0] = aes128;
  p.pass[1] = aes256;
  p.gcm_pre = p.impl != TLSGPU_GCM_TTABLE && p.impl != TLSGPU_GCM_SPLIT && (aes128 || aes256);
  // the staged ChaCha kernel's suite: RFC 7905 or, in a TLS 1.3 table, the TLS 1.3 kind
  p.cc_rfc = have[t13 ? TLSGPU_CHACHA20_POLY1305_TLS13 : TLSGPU_CHACHA20_POLY1305];
  p.cc_old = have[TLSGPU_CHACHA20_POLY1305_OLD];
  const bool any_cc = have[TLSGPU_CHACHA20_POLY1305] || have[TLSGPU_CHACHA20_POLY1305_OLD] ||
                      have[TLSGPU_CHACHA20_POLY1305_TLS13];
  // Fused (round 5): one queue kernel is the batch's only kernel — one AES key
  // size installed, no ChaCha, the hints rule out the per-wave-session kernel,
  // and they decide the variant (TLSGPU_HINT_NO_SHORT_RECORDS: no-pack, else
  // the pack variant, which also runs long records) — so it checks bounds,
  // writes the initial statuses and computes the per-record constants of its
  // own records in its prologue: no check_record_bounds, no gcm_prep_kernel, no
  // checked-descriptor copy, no variant that exits at once.
  p.fused_gcm = k.fused && in.bounds && p.impl == TLSGPU_GCM_QUEUE && p.args.pws == 1 &&
                aes128 != aes256 && !any_cc;
  // ... and the same for a batch of RFC 7539 ChaCha sessions only, or of a TLS 1.3
  // table whose only kind is the TLS 1.3 ChaCha one: the staged ChaCha kernel
  // checks bounds and writes the statuses of the records it does not run itself
  // (chacha_kernels.hip cc_tls_wave).
  // Not under TLSGPU_CHACHA_LEGACY, whose per-lane kernel (TLS 1.2 only) checks nothing.
  p.fused_cc = k.fused && in.bounds && !in.raw && p.cc_rfc && !aes128 && !aes256 && !p.cc_old &&
               !have[t13 ? TLSGPU_CHACHA20_POLY1305 : TLSGPU_CHACHA20_POLY1305_TLS13] &&
               !(k.cc_legacy && !t13);
  const bool fused = p.fused_gcm || p.fused_cc;
  p.setup = fused ? Setup::kFused : in.bounds ? Setup::kCheckBounds : Setup::kMemset;
  p.args.fused = fused ? 1u : 0u;
  p.args.in_bytes = fused ? in.in_bytes : 0;
  p.args.out_bytes = fused ? in.out_bytes : 0;
  const bool cuttable = p.fused_gcm && p.groups > 1 && p.groups <= 1024;
  p.balance = cuttable && (k.balance >= 2 || (k.balance == 1 && p.args.pack != 0));
  p.pieces = cuttable && !p.balance && (k.pieces >= 2 || (k.pieces == 1 && p.args.pack != 0));
  p.cut_snap = p.balance ? k.balance_snap : 0u;
  p.use_ctl = p.gcm_pre && !fused && p.impl == TLSGPU_GCM_QUEUE;

  // --- the scratch (ScratchLayout above)
  ScratchLayout& L = p.layout;
  size_t end = 0;
  if (p.gcm_pre) {
    end = sizeof(RecPre) * (size_t)in.n;
    if (!fused) {
      L.cnt_bytes = align256((size_t)p.groups * 4);
      L.ctl = end;
      L.ctl_bytes = 2048 + 2 * L.cnt_bytes;
      for (int ks = 0; ks < 2; ks++) {
        L.sel[ks] = L.ctl + 1024 * (size_t)ks;
        L.wg_next[ks] = L.ctl + 2048 + L.cnt_bytes * (size_t)ks;
      }
      end += L.ctl_bytes;
    } else if (p.balance) {
      L.cut = end;
      L.cut_bytes = align256((size_t)p.groups * 8);
      end += L.cut_bytes;
    } else if (p.pieces) {
      L.cut = align256(end);
      L.cut_bytes = align256(kPieceScratchBytes((uint32_t)p.groups)) + 256;
      end += L.cut_bytes;
    }
  }
  if (in.bounds && !fused) {
    L.safe = end;
    end += sizeof(tlsgpu_record) * (size_t)in.n;
  }
  L.total = end;
  return p;
}

// ---------------------------------------------------------------------------
// the execution

// Scratch of at least `bytes` for stream s (enlarging waits for the stream's
// earlier work, which may still read the old buffer).
void* tg::pre_scratch(tlsgpu_engine* e, hipStream_t s, size_t bytes) {
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

// The batch's scratch: the stream's grow-only buffer, or (TLSGPU_PRE_POOL,
// diagnostic only, DESIGN.md §4.1 pool scratch) the stream-ordered pool, which
// the caller frees after the launches (*pool).
static uint8_t* batch_scratch(tlsgpu_engine* e, hipStream_t s, size_t bytes, bool from_pool,
                              uint8_t** pool) {
  if (!from_pool) return (uint8_t*)pre_scratch(e, s, bytes);
  if (hipMallocAsync((void**)pool, bytes, s) != hipSuccess) *pool = nullptr;
  return *pool;
}

static void warn_park_bits_dropped(uint32_t flags) {
  static std::once_flag warned;
  std::call_once(warned, [flags] {
    fprintf(stderr, "libtlsgpu: TLSGPU_HY_FLAGS=%#x would park every wave; ignoring the "
                    "park bits\n", flags);
  });
}

// The setup of the plan: what comes before the GCM passes.  Completes `a`
// (cut work / pieces, or the checked descriptors).  TLSGPU_OK or the failure.
static int launch_setup(const BatchPlan& p, BatchArgs& a, uint8_t* scratch, uint8_t* ctl,
                        const Bounds* bounds, bool seal, bool raw, hipStream_t s) {
  const ScratchLayout& L = p.layout;
  switch (p.setup) {
    case Setup::kFused:
      if (p.balance) {  // each count range's work, then the kernel cuts at equal work
        auto* cw = reinterpret_cast<unsigned long long*>(scratch + L.cut);
        if (launch_range_work(a, p.groups, cw, s))
          return fail(TLSGPU_EHIP, "range work launch: %s", hipGetErrorString(hipGetLastError()));
        a.cut_work = cw;
        a.cut_snap = p.cut_snap;
      } else if (p.pieces) {  // whole pieces sorted by work
        if (launch_piece_plan(a, p.groups, scratch + L.cut, &a.pieces, &a.n_pieces, s))
          return fail(TLSGPU_EHIP, "piece plan launch: %s", hipGetErrorString(hipGetLastError()));
      }
      break;
    case Setup::kCheckBounds: {
      // one setup launch: sanitized descriptors, every record's initial status
      // (records whose session is empty / invalid keep TLSGPU_REC_PUBLIC_INVALID)
      // and the zeroed control words
      auto* safe = reinterpret_cast<tlsgpu_record*>(scratch + L.safe);
      if (launch_check_bounds(reinterpret_cast<const tlsgpu_record*>(a.descs), safe, a.n,
                              a.sessions, a.n_sessions, bounds->in_bytes, bounds->out_bytes, seal,
                              a.status, reinterpret_cast<uint32_t*>(ctl),
                              ctl ? (uint32_t)(L.ctl_bytes / 4) : 0u, s))
        return fail(TLSGPU_EHIP, "bounds launch: %s", hipGetErrorString(hipGetLastError()));
      a.descs = safe;
      break;
    }
    case Setup::kMemset:
      // records whose session is empty / invalid keep this status (raw EVP
      // jobs: the raw kernels write it themselves, so a queue batch launches no
      // fill kernel — round 2 measured ~18 K of them per queue run)
      if (!raw)
        HIPCHK(hipMemsetD32Async((hipDeviceptr_t)a.status, (int)TLSGPU_REC_PUBLIC_INVALID, a.n, s));
      if (ctl) HIPCHK(hipMemsetAsync(ctl, 0, L.ctl_bytes, s));
      break;
  }
  return TLSGPU_OK;
}

// one key size's GCM pass of the plan's implementation
static int launch_gcm_pass(const BatchPlan& p, const BatchArgs& a, RecPre* pre, bool seal, bool raw,
                           int rounds, hipStream_t s) {
  if (p.impl == TLSGPU_GCM_TTABLE) return launch_gcm(a, seal, raw, rounds, p.groups, s);
  if (p.impl == TLSGPU_GCM_SPLIT) return launch_gcm_split(a, seal, rounds, s);
  if (!a.fused && launch_gcm_prep(a, pre, seal, rounds, s)) return -1;
  if (p.impl == TLSGPU_GCM_QUEUE) return launch_gcm_queue(a, pre, seal, rounds, p.groups, s);
#ifdef TG_EXPERIMENTAL
  if (p.impl == TLSGPU_GCM_FUSED)
    return (rounds == 10 ? launch_gcm_fused10 : launch_gcm_fused14)(a, pre, seal, p.groups, s);
  return (rounds == 10 ? launch_gcm_hy10 : launch_gcm_hy14)(
      a, pre, seal, p.impl == TLSGPU_GCM_HYBRID ? 4 : 8, p.groups, s);
#else
  return -1;
#endif
}

int tg::run_batch(tlsgpu_sessions* t, const void* d_descs, uint32_t n, const uint8_t* d_in,
                  uint8_t* d_out, int32_t* d_status, hipStream_t s, bool seal, bool raw,
                  const Bounds* bounds, unsigned kinds, unsigned hints, tlsgpu_record* type_out) {
  const BatchKnobs& k = knobs();
  PlanInput in = {n, t->eng->num_cus, {}, t->generation, t->cc_padded, seal, raw, bounds != nullptr,
                  bounds ? bounds->in_bytes : 0, bounds ? bounds->out_bytes : 0,
                  type_out != nullptr,
                  hints == ~0u ? t->hints.load(std::memory_order_relaxed) : hints,
                  g_gcm_impl.load(), k};
  for (int kind = 0; kind < kKinds; kind++) in.have[kind] = t->have[kind] && ((kinds >> kind) & 1u);
  const BatchPlan p = plan_batch(in);
  const ScratchLayout& L = p.layout;
  if (p.args.hy_flags != k.hy_flags) warn_park_bits_dropped(k.hy_flags);

  BatchArgs a = p.args;  // the plan's scalars; the pointers:
  a.sessions = t->d_sess;
  a.gcm_tables = t->d_gcm;
  a.descs = d_descs;
  a.in = d_in;
  a.out = d_out;
  a.status = d_status;
  a.n_sessions = t->capacity;
  a.dbg = g_phase_stats;
  a.wg_times = wg_times_for(t->eng);
  a.type_out = p.type_out ? type_out : nullptr;
  uint8_t* scratch = nullptr;
  uint8_t* pool_scratch = nullptr;
  if (L.total && !(scratch = batch_scratch(t->eng, s, L.total, k.pre_pool, &pool_scratch)))
    return fail(TLSGPU_ENOMEM, "batch scratch (%u records)", n);
  // per-record constants of the queue kernels, and the queue impl's control words
  RecPre* pre = p.gcm_pre ? reinterpret_cast<RecPre*>(scratch + L.pre) : nullptr;
  uint8_t* ctl = p.use_ctl ? scratch + L.ctl : nullptr;

  if (const int rc = launch_setup(p, a, scratch, ctl, bounds, seal, raw, s)) return rc;
  for (int ks = 0; ks < 2; ks++) {
    if (!p.pass[ks]) continue;
    // selection words and counters per key size: a short AES-128 record must
    // not send the AES-256 pass to the pack variant
    if (ctl) {
      a.sel = reinterpret_cast<uint32_t*>(scratch + L.sel[ks]);
      a.wg_next = reinterpret_cast<uint32_t*>(scratch + L.wg_next[ks]);
    }
    if (launch_gcm_pass(p, a, pre, seal, raw, ks == 0 ? 10 : 14, s))
      return fail(TLSGPU_EHIP, "gcm-%d launch: %s", ks == 0 ? 128 : 256,
                  hipGetErrorString(hipGetLastError()));
  }
  // (a TLS 1.3 table: launch_chacha also runs the ChaCha sessions' unpad pass after an open)
  if ((p.cc_rfc || p.cc_old) && launch_chacha(a, seal, raw, p.cc_rfc, p.cc_old, s))
    return fail(TLSGPU_EHIP, "chacha launch: %s", hipGetErrorString(hipGetLastError()));
  if (pool_scratch) HIPCHK(hipFreeAsync(pool_scratch, s));
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
