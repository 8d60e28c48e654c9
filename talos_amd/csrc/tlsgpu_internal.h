// tlsgpu_internal.h — layouts shared by the host units (the .cpp files) and the
// HIP kernels (gcm_kernels.hip, chacha_kernels.hip, session_kernels.hip,
// key_schedule.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstddef>

#include "../../include/tlsgpu.h"

namespace tg {

constexpr int kWave = 64;

// Device session header (one per session id, 1 KiB, in HBM).  Mirrors the
// per-direction state LibreSSL keeps in SSL_AEAD_CTX (ssl/ssl_locl.h:527-543)
// plus the expanded key material aead_aes_gcm_init / _chacha20_poly1305_init
// derive (e_aes.c:1372-1413, e_chacha20poly1305.c:52-79).
struct alignas(16) DevSession {
  uint32_t kind;              // enum tlsgpu_aead, 0 = empty slot
  uint32_t rounds;            // 10 / 14 (AES)
  uint32_t tag_len;           // 1..16
  uint32_t key_len;
  uint32_t fixed_nonce_len;   // 4 / 12 / 0
  uint32_t xor_fixed_nonce;   // ChaCha RFC 7905 (and the TLS 1.3 ChaCha kind: the same nonce)
  uint32_t nonce_in_record;   // GCM explicit nonce (TLS 1.2); 0 for a TLS 1.3 GCM session,
                              // which is how the GCM kernels tell the two apart (gcm_tls13)
  uint32_t version;           // TLS version for the AAD
  uint8_t fixed_nonce[16];
  uint32_t rk[60];            // AES round keys, little-endian column words
  uint8_t chacha_key[32];
  uint32_t h_le[4];           // H = E_K(0), little-endian words
  uint32_t rk_rot[60];        // rotr16(rk[i]): round keys pre-rotated for the
                              // xor3 + alignbit + xor3 column form
  uint32_t pad_mask;          // TLS 1.3 seal padding: block - 1 (a power of two), 0 = none;
                              // always 0 for a TLS 1.2 session (tls13_inner_len)
  uint32_t secret_len;        // 0: the slot holds no traffic secret (every install from a key);
                              // 32 / 48: secret[] is the TLS 1.3 traffic secret the slot's key
                              // and IV come from, and the length is its hash (SHA-256 / SHA-384:
                              // tlsgpu_sessions_install_secrets, tlsgpu_sessions_key_update)
  uint8_t secret[48];
  uint32_t reserved[98];
};
static_assert(sizeof(DevSession) == 1024, "DevSession layout");
static_assert(offsetof(DevSession, pad_mask) == 576 && offsetof(DevSession, secret_len) == 580 &&
                  offsetof(DevSession, secret) == 584 && offsetof(DevSession, reserved) == 632,
              "DevSession layout");

// "Is this session TLS 1.3?" (the RFC 8446 5.2-5.4 record layout): the ChaCha
// kind that exists in TLS 1.3 only, or a GCM session without an explicit nonce.
// Every kernel and host path that frames, bounds or unpads records asks here.
// (On the host, where only the table's generation is known, nonce_in_record is
// "the table is not TLS 1.3".)
__host__ __device__ __forceinline__ bool tls13_session(uint32_t kind, uint32_t nonce_in_record) {
  return kind == TLSGPU_CHACHA20_POLY1305_TLS13 ||
         ((kind == TLSGPU_AES_128_GCM || kind == TLSGPU_AES_256_GCM) && nonce_in_record == 0);
}
// Inner plaintext length of a TLS 1.3 seal of `len` content bytes (RFC 8446 5.4:
// content || type || zeros): len + 1 rounded up to the session's padding block,
// pad_mask = block - 1 (a power of two up to 16384) or 0.  A record beyond the
// protocol's 16384 bytes (the engine's wider TLSGPU_MAX_RECORD range) is never
// padded, so a padded inner plaintext is at most 16385 bytes.  The only place
// the rule is written: every kernel and host path that sizes, bounds or frames a
// TLS 1.3 seal asks here.
__host__ __device__ __forceinline__ uint32_t tls13_inner_len(uint32_t len, uint32_t pad_mask) {
  return len >= 16384u ? len + 1u : (len + 1u + pad_mask) & ~pad_mask;
}
// pad_mask of a session with params.pad_block = b: read for TLS 1.3 sessions
// only; a power of two from 2 to 16384 is the block, and everything else (0, 1,
// and what valid_params rejects at install) is no padding
__host__ __device__ __forceinline__ uint32_t tls13_pad_mask(uint32_t version, uint32_t pad_block) {
  const bool block = pad_block > 1u && pad_block <= 16384u && (pad_block & (pad_block - 1u)) == 0;
  return version == 0x0304u && block ? pad_block - 1u : 0u;
}
// number of AEAD kinds + 1: arrays indexed by enum tlsgpu_aead
constexpr int kKinds = TLSGPU_CHACHA20_POLY1305_TLS13 + 1;

// Per-session GHASH tables (GCM sessions only), 16-B aligned, in HBM.
//   basis[p]      = K * x^p, K = H^64, p = 0..127 (little-endian words); a
//                   workgroup expands these into the 64 KiB byte-position table
//                   T[j][b] = (b at byte j) * K in LDS.
//   shoup[e-1][v] = v * H^e for nibble v (Shoup 4-bit, gcm128.c:255-324
//                   layout: v's MSB is x^0), e = 1..65, big-endian words.
//   bsrk[r][8b+k] = 0 or ~0: bit k of byte b of round key r, the AddRoundKey
//                   masks of the bitsliced AES path (bs_aes.h), read by s_load.
constexpr int kPowMax = 65;
struct alignas(16) DevGcmTables {
  uint32_t basis[128][4];
  uint32_t shoup[kPowMax][16][4];
  uint32_t bsrk[15][128];
};
static_assert(sizeof(DevGcmTables) == 2048 + kPowMax * 256 + 15 * 512, "DevGcmTables layout");

// Raw AEAD job: one EVP_AEAD_CTX_seal/open call (arbitrary nonce / AAD), used
// by the per-call drop-in path.  Pointers are device pointers.
struct RawJob {
  uint64_t in, out, nonce, aad;
  uint32_t in_len;     // open: ct||tag length ; seal: plaintext length
  uint32_t nonce_len;
  uint32_t aad_len;
  uint32_t session;
  uint64_t max_out;    // bytes zero-filled on failure
};

// Streaming GCM state of one EVP_CIPHER context (GCM128_CONTEXT,
// crypto/modes/modes_lcl.h:79-95), in device memory; byte strings as
// big-endian words.  Operated on by gcm_stream.hip.
struct alignas(16) GcmStream {
  uint32_t Yi[4], EKi[4], EK0[4], Xi[4];
  uint64_t len_aad, len_data;
  uint32_t mres, ares;
  int32_t rc;       // result of the program's last step (gcm128.c return values;
                    // FINISH: 0 tag equal, 1 differs, -1 no tag)
  uint32_t reserved;
};
enum GcmOpKind : uint32_t {
  GCM_OP_SETIV = 0, GCM_OP_AAD = 1, GCM_OP_ENCRYPT = 2, GCM_OP_DECRYPT = 3, GCM_OP_FINISH = 4,
  GCM_OP_TAG = 5
};
struct GcmStreamOp {
  uint32_t kind;    // GcmOpKind
  uint32_t reserved;
  uint64_t len;
  uint64_t in, out; // device pointers
};

// Kernel launch parameters for the GCM / ChaCha batch kernels.
// Global-address-space views of generic pointers.  Record pointers reach the
// kernels through descriptors, structs and lane shuffles, where the compiler
// loses their address space and emits FLAT loads/stores; a FLAT op counts in
// lgkmcnt as well as vmcnt, so every LDS wait (s_waitcnt lgkmcnt) would also
// wait for the in-flight prefetch loads.  Going through an integer keeps them
// global_load / global_store.
template <class T>
__device__ __forceinline__ const __attribute__((address_space(1))) T* gld(const void* p) {
  return (const __attribute__((address_space(1))) T*)(uintptr_t)p;
}
template <class T>
__device__ __forceinline__ __attribute__((address_space(1))) T* gst(void* p) {
  return (__attribute__((address_space(1))) T*)(uintptr_t)p;
}

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
// 16 B through a global-address-space pointer (p 16-B aligned)
__device__ __forceinline__ uint4 gload16(const void* p) {
  const u32x4 v = *gld<u32x4>(p);
  return make_uint4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ void gstore16(void* p, uint4 v) {
  u32x4 w;
  w.x = v.x; w.y = v.y; w.z = v.z; w.w = v.w;
  *gst<u32x4>(p) = w;
}

// A full 16-B block at any byte address with dword loads: the dwords that hold
// its bytes (each contains at least one byte of the block, so none crosses the
// buffer's last page) funnel-shifted into place.  TLS wire fragments sit 5 B
// past their headers, so in-place opens of wire buffers take this path.
__device__ __forceinline__ void load16_any(const uint8_t* p, uint32_t v[4]) {
  const uintptr_t a = (uintptr_t)p;
  const uint32_t sh = (uint32_t)a & 3u;
  const auto q = gld<uint32_t>((const void*)(a & ~(uintptr_t)3));
  const uint32_t w0 = q[0], w1 = q[1], w2 = q[2], w3 = q[3];
  const uint32_t w4 = sh ? q[4] : 0u;
  v[0] = __builtin_amdgcn_alignbyte(w1, w0, sh);
  v[1] = __builtin_amdgcn_alignbyte(w2, w1, sh);
  v[2] = __builtin_amdgcn_alignbyte(w3, w2, sh);
  v[3] = __builtin_amdgcn_alignbyte(w4, w3, sh);
}

// The first nb (1..16) bytes of a block at any byte address, zero past them:
// dword loads only where a byte below nb lies (a record's last piece may end
// at its buffer's last page).
__device__ __forceinline__ void load16_upto(const uint8_t* p, uint32_t nb, uint32_t v[4]) {
  const uintptr_t a = (uintptr_t)p;
  const uint32_t sh = (uint32_t)a & 3u;
  const auto q = gld<uint32_t>((const void*)(a & ~(uintptr_t)3));
  const uint32_t nd = (sh + nb + 3) >> 2;  // dwords holding bytes [0, nb): 1..5
  const uint32_t w0 = q[0], w1 = nd > 1 ? q[1] : 0u, w2 = nd > 2 ? q[2] : 0u;
  const uint32_t w3 = nd > 3 ? q[3] : 0u, w4 = nd > 4 ? q[4] : 0u;
  v[0] = __builtin_amdgcn_alignbyte(w1, w0, sh);
  v[1] = __builtin_amdgcn_alignbyte(w2, w1, sh);
  v[2] = __builtin_amdgcn_alignbyte(w3, w2, sh);
  v[3] = __builtin_amdgcn_alignbyte(w4, w3, sh);
}

// The matching store: whole dwords inside the block, 1-2 byte/short stores at
// its two ends (never a read-modify-write of a neighbour's bytes).
__device__ __forceinline__ void store16_any(uint8_t* p, const uint32_t o[4]) {
  const uintptr_t a = (uintptr_t)p;
  const uint32_t sh = (uint32_t)a & 3u;
  if (sh == 0) {
    const auto q = gst<uint32_t>(p);
    q[0] = o[0]; q[1] = o[1]; q[2] = o[2]; q[3] = o[3];
    return;
  }
  const auto q = gst<uint32_t>((void*)(a - sh));  // q[1..3] lie inside the block
  const auto b = gst<uint8_t>(p);
  const auto h = gst<uint16_t>(p);  // used at even byte offsets only
  q[1] = __builtin_amdgcn_alignbyte(o[1], o[0], 4 - sh);
  q[2] = __builtin_amdgcn_alignbyte(o[2], o[1], 4 - sh);
  q[3] = __builtin_amdgcn_alignbyte(o[3], o[2], 4 - sh);
  if (sh == 1) {
    b[0] = (uint8_t)o[0];
    gst<uint16_t>(p + 1)[0] = (uint16_t)(o[0] >> 8);
    b[15] = (uint8_t)(o[3] >> 24);
  } else if (sh == 2) {
    h[0] = (uint16_t)o[0];
    h[7] = (uint16_t)(o[3] >> 16);
  } else {
    b[0] = (uint8_t)o[0];
    gst<uint16_t>(p + 13)[0] = (uint16_t)(o[3] >> 8);
    b[15] = (uint8_t)(o[3] >> 24);
  }
}

struct BatchArgs {
  const DevSession* sessions;
  const DevGcmTables* gcm_tables;   // indexed by session id
  const void* descs;                // tlsgpu_record[] or RawJob[]
  uint32_t n;
  uint32_t records_per_group;       // contiguous range per workgroup
  const uint8_t* in;
  uint8_t* out;
  int32_t* status;
  uint32_t n_sessions;              // descriptors naming a session >= this are invalid
  uint32_t bs_reserve;              // hybrid kernel: a bitsliced wave takes a record pair
                                    // only while >= this many records of the run are left
  uint32_t hy_flags;                // hybrid kernel experiments (env TLSGPU_HY_FLAGS):
                                    // 1 = no bitsliced pairs, 2 = T-table waves idle,
                                    // 4 = bitsliced waves idle
  unsigned long long* dbg;          // phase timing (PhaseClock), normally null
  uint32_t bs16_min;                // queue kernel: non-zero = the no-pack variant runs with
                                    // 4 packed bitsliced waves, which take records of n >= this
                                    // (<= 16384, 16-B aligned; gcm_queue_b16.hip); 0 = never
  uint32_t pack;                    // queue kernel: short records of one session share a
                                    // wave (gcm_pack); 0 = off
  uint32_t* sel;                    // queue impl: 4 selection words of this key size, filled
                                    // by the prep pass: [0] a record can be packed, [1] session
                                    // runs (records whose session differs from the previous
                                    // record's), [2] records.  The queue kernel's no-pack / pack
                                    // variants and the per-wave-session kernel all launch; the
                                    // ones the words do not select return (null: queue no-pack)
  uint32_t pws;                     // per-wave-session kernel: 0 auto (runs shorter than
                                    // kPwsRun records on average), 1 never, 2 always
  uint32_t* wg_next;                // per-wave-session kernel: one record counter per workgroup
  uint32_t fused;                   // queue no-pack kernel (round 5): the bounds check, the
                                    // initial statuses and the per-record constants of the
                                    // workgroup's records run in its own prologue (no
                                    // check_record_bounds / gcm_prep_kernel launches); descs
                                    // are the caller's, checked against in_bytes / out_bytes
  uint64_t in_bytes, out_bytes;     // fused: sizes of the caller's in / out buffers
  const unsigned long long* cut_work;  // fused, non-null: the work of each count range
                                       // (range_work_kernel); each workgroup takes the
                                       // records between its two work cuts instead
  uint32_t cut_snap;                // cut_work: snap a cut to a session-run boundary within
                                    // cut_snap / 1024 of a share of the work (0: exact cuts)
  const uint2* pieces;              // fused, non-null: whole pieces (a session run inside
  const uint32_t* n_pieces;         // one count range) sorted by work, largest first; workgroup
                                    // w takes pieces m*G + (m even ? w : G-1-w) (piece_sort_kernel;
                                    // *n_pieces == 0: the count ranges)
  unsigned long long* wg_times;     // diagnostic (TLSGPU_WG_TIMES=1), normally null: per
                                    // workgroup {start, end (s_memrealtime), rlo, rhi}
  uint32_t tls13;                   // the table's sessions are TLS 1.3: the GCM launchers run
                                    // the kernels compiled for that record layout (their *13
                                    // twins), launch_chacha the staged kernel's TLS 1.3
                                    // instantiation, and each, after an open, the unpad pass
  tlsgpu_record* type_out;          // TLS 1.3 open, non-null (tlsgpu_open_wire: the engine's own
                                    // descriptors): the unpad pass also moves every opened
                                    // record's inner content type into len_type's type bits
  uint32_t cc_pad;                  // seal: the table holds a TLS 1.3 ChaCha session with a
                                    // padding block (run_batch); launch_chacha then runs the
                                    // staged kernel's PAD instantiation
};

// Work-balanced ranges (round 5): a record's work for the cut — its payload
// bytes plus a per-record cost (parse, J0 / tag, the GHASH finish: about a
// quarter of a 1 KiB record's time in the queue kernel).  Any positive weight
// gives a correct partition (each cut is computed the same way by the two
// workgroups that share it); this one balances the Zipf-length workload.
constexpr uint32_t kCutRecordWork = 256;
__host__ __device__ __forceinline__ uint64_t cut_work_of(uint32_t len_type) {
  return (uint64_t)(len_type & 0xFFFFFFu) + kCutRecordWork;
}

// Average session-run length below which the per-wave-session kernel (gcm_pw.hip)
// replaces the queue kernel: a run shorter than the workgroup's wave count leaves
// waves idle at the run barrier.
constexpr uint32_t kPwsRun = 12;
// Selection words of the prep pass per key size: kSelSlots slots of kSelWords
// words (one 64-B line each) = {packable flag, session-run starts, records};
// a workgroup adds into slot blockIdx % kSelSlots, readers sum the slots.
constexpr int kSelSlots = 16;
constexpr int kSelWords = 16;
__host__ __device__ __forceinline__ bool pws_selected(uint32_t mode, uint32_t runs, uint32_t recs) {
  return mode == 2 || (mode == 0 && runs * kPwsRun > recs);
}

// Per-record constants of the hybrid kernel (gcm_prep_kernel, one per record,
// 48 B in a stream-ordered scratch buffer; read back with s_load).  All in the
// little-endian column form of the T-table path (gcm_device.h rec_consts).
struct alignas(16) RecPre {
  uint32_t ek0[4];    // E_K(J0), the tag mask
  uint32_t k1a, k1b;  // counter-independent parts of round-1 columns 0, 1 (incl. rk1)
  uint32_t k2[4];     // round-2 constants of the T-table fast path
  uint32_t sb2[2];    // SubBytes of round-1 output columns 2, 3 (bitsliced round 2)
};
static_assert(sizeof(RecPre) == 48, "RecPre layout");

}  // namespace tg

// Kernel launchers (defined in the .hip files).
namespace tg {
int launch_gcm(const BatchArgs& a, bool seal, bool raw, int rounds, int groups,
               hipStream_t s);
int launch_gcm_split(const BatchArgs& a, bool seal, int rounds, hipStream_t s);
int launch_gcm_prep(const BatchArgs& a, RecPre* pre, bool seal, int rounds, hipStream_t s);
int launch_range_work(const BatchArgs& a, int groups, unsigned long long* out, hipStream_t s);
// Whole-piece balance (round 5): the pieces of every count range, then all of
// them sorted by work (gcm_queue.hip).  scratch: kPieceScratchBytes(groups).
constexpr uint32_t kPiecesPerRange = 16;  // more in one count range: no plan (count ranges)
constexpr uint32_t kMaxPieces = 4096;     // the sort's LDS capacity
__host__ __device__ constexpr size_t kPieceScratchBytes(uint32_t groups) {
  return (size_t)groups * kPiecesPerRange * 16 + (size_t)((groups + 3) & ~3u) * 4 +
         (size_t)groups * kPiecesPerRange * 8 + 256;
}
int launch_piece_plan(const BatchArgs& a, int groups, uint8_t* scratch, const uint2** pieces,
                      const uint32_t** n_pieces, hipStream_t s);
int launch_gcm_queue(const BatchArgs& a, const RecPre* pre, bool seal, int rounds, int groups,
                     hipStream_t s);
int launch_gcm_queue_b16(const BatchArgs& a, const RecPre* pre, bool seal, int rounds, int groups,
                         hipStream_t s);
int launch_gcm_pw(const BatchArgs& a, const RecPre* pre, bool seal, int rounds, int groups,
                  hipStream_t s);
// The same launchers for TLS 1.3 session tables (gcm_kernels13.hip, gcm_queue13.hip,
// gcm_pw13.hip: the kernels compiled for the RFC 8446 record layout).  The host
// units call the launchers above, which forward here when a.tls13 is set.
int launch_gcm13(const BatchArgs& a, bool seal, bool raw, int rounds, int groups, hipStream_t s);
int launch_gcm_split13(const BatchArgs& a, bool seal, int rounds, hipStream_t s);
int launch_gcm_prep13(const BatchArgs& a, RecPre* pre, bool seal, int rounds, hipStream_t s);
int launch_gcm_queue13(const BatchArgs& a, const RecPre* pre, bool seal, int rounds, int groups,
                       hipStream_t s);
int launch_gcm_pw13(const BatchArgs& a, const RecPre* pre, bool seal, int rounds, int groups,
                    hipStream_t s);
// TLS 1.3 open: inner-plaintext lengths in a.status -> content lengths, for the
// records of sessions with `rounds` AES rounds (session_kernels.hip; called by
// the TLS 1.3 launchers after their kernels, once per key size; rounds 0: the
// ChaCha sessions, after launch_chacha's kernel)
int launch_tls13_unpad(const BatchArgs& a, int rounds, hipStream_t s);
int launch_gcm_stream(const DevSession* sessions, const DevGcmTables* tables, uint32_t session,
                      GcmStream* st, const GcmStreamOp* ops, uint32_t nops, hipStream_t s);
int launch_gcm_hy10(const BatchArgs& a, const RecPre* pre, bool seal, int bs_waves, int groups,
                    hipStream_t s);
int launch_gcm_fused10(const BatchArgs& a, const RecPre* pre, bool seal, int groups, hipStream_t s);
int launch_gcm_fused14(const BatchArgs& a, const RecPre* pre, bool seal, int groups, hipStream_t s);
int launch_gcm_hy14(const BatchArgs& a, const RecPre* pre, bool seal, int bs_waves, int groups,
                    hipStream_t s);
int launch_bs_ecb(const DevSession* sessions, uint32_t session, int rounds, const void* d_in,
                  void* d_out, uint32_t nblocks, hipStream_t s);
// rfc / old: the batch may hold records of the staged kernel's suite (RFC 7905,
// or in a TLS 1.3 table TLSGPU_CHACHA20_POLY1305_TLS13) / of the draft suite
int launch_chacha(const BatchArgs& a, bool seal, bool raw, bool rfc, bool old, hipStream_t s);

// Doorbell slot of the persistent EVP server (evp_server.hip, evp_doorbell.cpp): one
// per calling thread, in pinned host memory, 256 B.  The thread fills the job
// (the RawJob itself and, when they fit, its nonce and AAD inline), then
// stores `post` (its next job number); a server workgroup that sees post != the
// number it last served copies the slot into LDS with one wave load, runs the
// job (its input read from and its output and status written to the thread's
// pinned staging buffer, zero-copy) and stores `done` = post after the output
// and status are visible to the host.
struct alignas(256) DoorbellSlot {
  uint32_t post;        // host: number of the posted job (written last)
  uint32_t done;        // device: number of the last job finished
  uint32_t op;          // bit 0: seal; bits 8-15: AES rounds (10 / 14); bit 16:
                        // nonce (then AAD) inline in `inl`
  uint32_t n_sessions;  // capacity of the context's session table
  uint32_t key_id;      // unique per installed key (process-wide): a server
                        // workgroup keeps the GCM tables of the last key it
                        // served in LDS and skips reloading them for the same id
  uint32_t reserved;
  uint64_t status;      // device address of the job's int32 status
  uint64_t sessions;    // const DevSession* of the context's table
  uint64_t gcm_tables;  // const DevGcmTables*
  RawJob job;           // 56 B; job.nonce / job.aad ignored when inline
  uint8_t inl[152];     // inline nonce || AAD
};
static_assert(sizeof(RawJob) == 56, "RawJob layout");
static_assert(sizeof(DoorbellSlot) == 256 && offsetof(DoorbellSlot, job) == 48,
              "DoorbellSlot layout");
constexpr uint32_t kDoorbellInline = 152;
// DoorbellSlot::op bits beyond the job (evp_server.hip): install the session
// image whose device address is in inl[0..7] before the job (deferred
// EVP_AEAD_CTX_init), with its GCM tables; op code (bits 8-15) 30: scrub the slot
constexpr uint32_t kDoorbellOpInstall = 1u << 17;
constexpr uint32_t kDoorbellOpInstallTables = 1u << 18;
constexpr uint32_t kDoorbellOpScrub = 30;
struct ServerArgs {
  DoorbellSlot* slots;        // device view of the pinned slot array
  uint32_t nslots;
  const uint32_t* stop;       // pinned word: non-zero = exit now
  unsigned long long lifetime;  // s_memrealtime ticks (100 MHz) a workgroup serves at most
  uint32_t* exited;             // pinned [gridDim.x]: a workgroup stores `seq` here as it
                                // leaves (the host's exit drain waits on it, no HIP call)
  uint32_t seq;                 // this instance's launch number (from 1)
  unsigned long long* trace;    // null, or pinned [nslots][kTraceWords]: realtime at pick,
                                // slot loaded, GCM job marks 0..6, job done, answer
                                // released (TLSGPU_EVP_DOORBELL_TRACE)
  unsigned long long* scrubs;   // HBM [1 + kScrubRing + 1]: scrub count, the ring of
                                // scrubbed key ids ((index + 1) << 32 | key), flushes done
};
constexpr uint32_t kScrubRing = 256;
constexpr int kTraceWords = 16;  // + the last working wave's marks 7, 8 at [11], [12]
int launch_evp_server(const ServerArgs& a, int groups, hipStream_t s);
int launch_session_install_arg(DevSession* sessions, DevGcmTables* tables,
                               const tlsgpu_session_params& p, uint32_t id, hipStream_t s);
int launch_session_install(DevSession* sessions, DevGcmTables* tables,
                           const tlsgpu_session_params* d_params, uint32_t first,
                           uint32_t n, hipStream_t s);
int launch_wire_frame(const tlsgpu_wire_stream* streams, uint32_t n_streams, const uint8_t* wire,
                      const DevSession* sessions, uint32_t n_sessions, uint32_t max_records,
                      tlsgpu_record* recs, tlsgpu_wire_result* results, uint32_t* total,
                      hipStream_t s);
int launch_wire_seal_frame(const tlsgpu_write_stream* streams, uint32_t n_streams,
                           const DevSession* sessions, uint32_t n_sessions, uint8_t* wire,
                           uint64_t wire_bytes, uint32_t max_records, tlsgpu_record* recs,
                           tlsgpu_write_result* results, uint32_t* total, hipStream_t s);
int launch_wire_finish(uint32_t n_streams, tlsgpu_wire_result* results, int32_t* status,
                       hipStream_t s);
// tlsgpu_gather_wire (wire_kernels.hip): the plan writes, per record slot it
// takes, the record's absolute destination offset into dst[max_records], which
// the caller has preset to kNoGather (bytes of 0xFF); the copy moves the slots
// that have one.  piece: bytes of a record per wave, 16384 / piece waves per
// record slot: kGatherPiece where the wire buffer holds more than
// kGatherSplitBytes per record slot (long records: 8 waves each), else
// kGatherWhole (one wave per slot; the waves of pieces a short record does not
// have cost more than splitting gains: DESIGN.md §4.6b has the measurement the
// threshold comes from).  4096 is compiled too (TLSGPU_GATHER_PIECE forces one
// of the three, experiments only).
constexpr uint64_t kNoGather = ~0ull;
constexpr uint32_t kGatherPiece = 2048, kGatherWhole = 16384;
constexpr uint64_t kGatherSplitBytes = 9216;
int launch_wire_gather_plan(const tlsgpu_wire_stream* streams, const tlsgpu_wire_result* results,
                            uint32_t n_streams, const tlsgpu_record* recs, const int32_t* status,
                            uint32_t max_records, uint64_t wire_bytes,
                            const tlsgpu_read_stream* reads, uint64_t app_bytes, uint64_t* dst,
                            tlsgpu_read_result* out, hipStream_t s);
int launch_wire_gather_copy(const tlsgpu_record* recs, const int32_t* status, uint32_t max_records,
                            const uint8_t* wire, uint64_t wire_bytes, const uint64_t* dst,
                            uint8_t* app, uint64_t app_bytes, uint32_t piece, hipStream_t s);
// tlsgpu_open_wire with the table's KeyUpdate switch on (wire_peek.hip).  The
// peek runs between launch_wire_frame and the open: it cuts every TLS 1.3 stream
// after its first record whose first plaintext block looks like a KeyUpdate
// (descriptors behind it back to all ones, the result rewritten, key_update =
// TLSGPU_WIRE_KU_HELD).  The confirmation runs after launch_wire_finish and
// turns HELD into TLSGPU_WIRE_KU_UPDATE / _REQUESTED from the verified record.
int launch_wire_peek13(const tlsgpu_wire_stream* streams, uint32_t n_streams, const uint8_t* wire,
                       const DevSession* sessions, uint32_t n_sessions, uint32_t max_records,
                       tlsgpu_record* recs, tlsgpu_wire_result* results, hipStream_t s);
int launch_wire_ku_confirm(const tlsgpu_wire_stream* streams, uint32_t n_streams,
                           const uint8_t* wire, uint32_t max_records, const tlsgpu_record* recs,
                           const int32_t* status, tlsgpu_wire_result* results, hipStream_t s);
// tlsgpu_read_wire (wire_read.hip).  The plan runs between launch_wire_frame and
// an out-of-place open into d_app: it gives every placed record its destination
// (out_off), cuts each stream before the first record that is not placed
// (descriptors from there on back to all ones, the wire result rewritten) and
// leaves the stop in `out`.  The finish runs after launch_wire_finish and
// completes `out` from the delivered records' statuses.
int launch_wire_read_plan(const tlsgpu_wire_stream* streams, uint32_t n_streams,
                          const DevSession* sessions, uint32_t n_sessions, uint32_t max_records,
                          uint64_t wire_bytes, const tlsgpu_read_stream* reads, uint64_t app_bytes,
                          tlsgpu_record* recs, tlsgpu_wire_result* results, tlsgpu_read_result* out,
                          hipStream_t s);
int launch_wire_read_finish(const tlsgpu_wire_stream* streams, const tlsgpu_wire_result* results,
                            uint32_t n_streams, const tlsgpu_record* recs, const int32_t* status,
                            uint32_t max_records, tlsgpu_read_result* out, hipStream_t s);
int launch_fill_synthetic(uint8_t* d_out, uint64_t stride, uint32_t span_len,
                          uint32_t n, uint64_t seed, uint64_t index0, hipStream_t s);
int launch_upload_session(const void* img, DevSession* sess, DevGcmTables* tab,
                          uint32_t table_bytes, hipStream_t s);
int launch_scrub_session(DevSession* sess, DevGcmTables* tab, hipStream_t s);
// The device key schedule (key_schedule.hip).  A table's
// scratch holds one entry per session of a call's chunk: what the derive kernel
// (one lane per entry) leaves for the install kernel (one wave per entry), and
// what a hipMemsetAsync behind the two zeroes again.
struct alignas(16) KeyScratch {
  tlsgpu_session_params params;  // the derived key and IV as an install takes them
  uint32_t secret_len;           // the secret the slot keeps: its length and bytes, laid
  uint8_t secret[48];            // out as DevSession::secret_len / secret are
  int32_t status;                // TLSGPU_OK: install it; anything else: skip the entry
  uint32_t id;                   // the slot
  uint32_t reserved;
};
static_assert(sizeof(KeyScratch) == 128 && sizeof(tlsgpu_session_params) == 64 &&
                  sizeof(tlsgpu_secret_params) == 60,
              "key schedule layouts");
constexpr uint32_t kKeyScratchEntries = 65536;  // longer calls run in chunks of this
// Derive n entries.  Install form (secrets != null): entry i is secrets[i] for
// slot first + i.  Update form (secrets == null): entry i is slot ids[i] moved
// to its next generation; `claim` (one word per slot) and `epoch` (unique per
// call, never 0) let an id listed several times derive once: the first entry to
// swap the epoch in owns the slot, the others report TLSGPU_OK and install
// nothing.  status may be null (install form).  scratch == null (update form on
// a table that never held a secret): statuses only.
int launch_tls13_derive(const tlsgpu_secret_params* secrets, const DevSession* sessions,
                        uint32_t capacity, const uint32_t* ids, uint32_t first, uint32_t n,
                        uint32_t* claim, uint32_t epoch, KeyScratch* scratch, int32_t* status,
                        hipStream_t s);
int launch_tls13_install(DevSession* sessions, DevGcmTables* tables, const KeyScratch* scratch,
                         uint32_t n, hipStream_t s);
int launch_wire_ku_ids(const tlsgpu_wire_stream* streams, const tlsgpu_wire_result* results,
                       uint32_t n_streams, uint32_t* ids, hipStream_t s);
// GCM table bytes the default kernels read (basis + Shoup tables; the
// bitsliced masks only in the experimental build)
#ifdef TG_EXPERIMENTAL
constexpr uint32_t kGcmTableUploadBytes = sizeof(DevGcmTables);
#else
constexpr uint32_t kGcmTableUploadBytes = offsetof(DevGcmTables, bsrk);
#endif
// session_host.cpp: the image install_body writes, built on the host (the
// bitsliced masks only when a kernel of this build reads them)
bool host_crypto_ok();  // AES-NI + PCLMUL present: the host image can be built
bool host_session_image(const tlsgpu_session_params& p, DevSession* s, DevGcmTables* t,
                        bool bitsliced_masks = kGcmTableUploadBytes > offsetof(DevGcmTables, bsrk),
                        bool compact = false);
void host_image_complete(DevGcmTables* t);  // a compact image's Shoup entries
int launch_check_bounds(const tlsgpu_record* recs, tlsgpu_record* safe, uint32_t n,
                        const DevSession* sessions, uint32_t n_sessions, uint64_t in_bytes,
                        uint64_t out_bytes, bool seal, int32_t* status, uint32_t* ctl,
                        uint32_t ctl_words, hipStream_t s);
int launch_fill_synthetic_spans(uint8_t* d_out, const uint64_t* d_offs, const uint32_t* d_lens,
                                uint32_t n, uint64_t seed, uint64_t index0, hipStream_t s);
// TaLoS TLS-processing hooks (talos_hooks.cpp): is a callback registered, and
// fire it (the callback may change *len) — used by the host-delivery paths.
bool talos_read_hooked();
bool talos_write_hooked();
void talos_read(const void* ssl, uint8_t* data, uint32_t* len);
void talos_write(const void* ssl, uint8_t* data, uint32_t* len);

}  // namespace tg
