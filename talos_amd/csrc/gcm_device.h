// gcm_device.h — device-side building blocks shared by the AES-GCM kernels
// (gcm_kernels.hip: T-table batch kernel; gcm_bs_kernels.hip: bitsliced and
// hybrid kernels).  Layout and mapping notes: gcm_kernels.hip header and
// DESIGN.md §4.  Each translation unit gets its own copy of the LDS array.
#pragma once
#include <utility>

#include "aes_common.h"
#include "bs_aes.h"
#include "tlsgpu_internal.h"

// The TLS record layout is fixed per translation unit: TG_TLS13 = 0 (default)
// compiles the TLS 1.2 AEAD layout (explicit nonce, 13-byte AAD), TG_TLS13 = 1
// the TLS 1.3 one (RFC 8446 5.2-5.4) — gcm_queue13.hip, gcm_pw13.hip and
// gcm_kernels13.hip include their TLS 1.2 twins with it set.  As runtime
// session fields the same differences cost the queue kernel's pack variants
// eight more spilled VGPRs, so a session table holds one
// generation and run_batch picks the launchers (TG_GEN names) by it.
#ifndef TG_TLS13
#define TG_TLS13 0
#endif
#if TG_TLS13
#define TG_GEN(f) f##13
#else
#define TG_GEN(f) f
#endif

namespace tg {

constexpr bool kTls13 = TG_TLS13 != 0;

static __device__ const WordTable g_te0 = kTe0;

constexpr int kThreads = 1024;
constexpr int kWaves = kThreads / kWave;
// The GHASH byte-position table sits at LDS offset 0 and the AES T-tables at
// 64 KiB: a table address is then a single v_perm with no base add — the
// KT lookups' base is 0, and the T-table base 0x10000 rides in byte 2 of the
// lane's `laneoff` operand, which taddr's selector copies (aes_laneoff).
constexpr uint32_t KT_OFF = 0;
constexpr uint32_t AES_OFF = 0x10000;
static_assert(AES_OFF == 0x10000, "taddr takes the T-table base from byte 2 of laneoff");
constexpr uint32_t SH_OFF = 131072;
// Shoup tables: entry (e, v) of H^e (e = 1..65, nibble v) at
// SH_OFF + ((e-1)/16) * 4 KiB + v * 256 + ((e-1) % 16) * 16 (sh_base), i.e. the
// power picks the 16-B column: the lanes of a ds_read_b128 group (distinct lane
// % 16) need powers with distinct (e-1) % 16 in the per-lane chain weights, so
// their lookups are conflict-free whatever the nibbles.
constexpr uint32_t SH_BYTES = ((kPowMax + 15) / 16) * 4096;
constexpr uint32_t R4_OFF = SH_OFF + SH_BYTES;
constexpr uint32_t Q_OFF = R4_OFF + 64;      // hybrid kernel: per-run record queue
constexpr uint32_t DBG_OFF = Q_OFF + 16;     // hybrid kernel: phase counters (diagnostic)
constexpr uint32_t PLAN_OFF = DBG_OFF + 32 * 8;  // queue kernel: per-run pack plan
constexpr uint32_t kPlanCap = 2048;                // records planned per run (runs split)
// Queue kernel: the session's lengths-block table (load_len_table, GhLaneLen),
// 8 rows of 16 entries: rows p < kLenRows (nibble v at nibble position p of the
// ciphertext bit count) * H, row kLenRows the TLS AAD bit count * H in every
// entry, row 7 zero.
constexpr uint32_t LEN_OFF = PLAN_OFF + 4 * kPlanCap;
constexpr uint32_t kLenRows = 6;
constexpr uint32_t kLenEntries = 8 * 16;
static_assert(8ull * TLSGPU_MAX_RECORD < (1ull << (4 * kLenRows)), "ciphertext bit count nibbles");
#ifdef TG_LDS_BYTES  // a translation unit with its own LDS plan (gcm_pw.hip)
constexpr uint32_t LDS_BYTES = TG_LDS_BYTES;
#else
constexpr uint32_t LDS_BYTES = LEN_OFF + 16 * kLenEntries;
#endif

__shared__ __attribute__((aligned(16))) uint8_t s_lds[LDS_BYTES];

// Wave-uniform data (session header, round keys, descriptors) is read through
// the constant address space so it lands in SGPRs via s_load.  A persistent
// kernel (evp_server.hip: TG_VECTOR_SESSION_LOADS) reads the same data as
// plain global loads instead: a kernel launch invalidates the scalar cache, a
// long-running kernel never gets that, and session slots are re-keyed while it
// runs; its per-job acquire fence invalidates only the vector caches.
#ifdef TG_VECTOR_SESSION_LOADS
// a uniform word read by a vector load and moved to an SGPR (readfirstlane)
struct cu32_word {
  uint32_t raw;
  __device__ __forceinline__ operator uint32_t() const {
    return __builtin_amdgcn_readfirstlane(raw);
  }
};
typedef const cu32_word cu32;
#else
typedef __attribute__((address_space(4))) const uint32_t cu32;
#endif
template <typename T>
__device__ __forceinline__ cu32* as_const(const T* p) { return (cu32*)(p); }

// ---------------------------------------------------------------------------
// LDS access helpers
__device__ __forceinline__ uint32_t lds_u32(uint32_t off) {
  return *reinterpret_cast<const uint32_t*>(s_lds + off);
}
__device__ __forceinline__ uint4 lds_u128(uint32_t off) {
  return *reinterpret_cast<const uint4*>(s_lds + off);
}

// The lane's T-table operand: its bank offset (lane % 32) * 4 in byte 0 and
// the table base AES_OFF >> 16 in byte 2.
__device__ __forceinline__ uint32_t aes_laneoff(uint32_t lane) { return ((lane & 31) * 4) | AES_OFF; }
// address of Te0[byte r of w] for this lane: [0, AES_OFF >> 16, byte, lane bank].
// Byte 1 already sits where the address wants it: (w & 0xFF00) | laneoff in one
// full-rate v_bitop3_b32 (truth table 0xEA = (a & b) | c) instead of a
// v_perm_b32, which measured 3.4 cycles per wave64 instruction at 4 waves/SIMD
// against 2.1 (tools/ubench.hip); VALU issue adds to the T-table waves' LDS
// lookup time nearly 1:1 (profiles/r03b_ubench_set2.jsonl).
template <int R>
__device__ __forceinline__ uint32_t taddr(uint32_t w, uint32_t laneoff) {
  if constexpr (R == 1) return __builtin_amdgcn_bitop3_b32(w, 0xFF00u, laneoff, 0xEA);
  return __builtin_amdgcn_perm(w, laneoff, 0x0C020000u | ((4u + R) << 8));
}
__device__ __forceinline__ uint32_t rotl16(uint32_t x) { return __builtin_amdgcn_alignbit(x, x, 16); }
// three-input XOR in one VALU op: v_bitop3_b32 with truth table 0x96 (gfx950
// has no v_xor3_b32; hipcc does not form bitop3 from these ^ chains).  The
// builtin, not inline asm: a wave-uniform operand (round-key word) stays in
// its SGPR instead of being copied to a VGPR first, and the scheduler sees it.
__device__ __forceinline__ uint32_t xor3(uint32_t a, uint32_t b, uint32_t c) {
#ifdef TG_XOR3_ASM  // opaque to the scheduler: gcm_pw.hip (the builtin's schedule spills there)
  uint32_t d;
  asm("v_bitop3_b32 %0, %1, %2, %3 bitop3:0x96" : "=v"(d) : "v"(a), "v"(b), "v"(c));
  return d;
#else
  return __builtin_amdgcn_bitop3_b32(a, b, c, 0x96);
#endif
}

#define TE0(w, r) lds_u32(taddr<r>((w), laneoff))
#define TE1(w, r) lds_u32(128 + taddr<r>((w), laneoff))

// One full AES round on little-endian columns (ShiftRows: row r of output
// column c comes from input column c+r).  kr_c = rotr16(k_c) is folded into the
// rotated half so a column costs xor3 + alignbit + xor3:
//   t = Te0[a] ^ Te1[b] ^ rotl16(Te0[c] ^ Te1[d] ^ rotr16(k))
__device__ __forceinline__ void aes_round(uint32_t& s0, uint32_t& s1, uint32_t& s2, uint32_t& s3,
                                          uint32_t k0, uint32_t k1, uint32_t k2, uint32_t k3,
                                          uint32_t laneoff) {
  uint32_t t0 = xor3(TE0(s0, 0), TE1(s1, 1), rotl16(xor3(TE0(s2, 2), TE1(s3, 3), k0)));
  uint32_t t1 = xor3(TE0(s1, 0), TE1(s2, 1), rotl16(xor3(TE0(s3, 2), TE1(s0, 3), k1)));
  uint32_t t2 = xor3(TE0(s2, 0), TE1(s3, 1), rotl16(xor3(TE0(s0, 2), TE1(s1, 3), k2)));
  uint32_t t3 = xor3(TE0(s3, 0), TE1(s0, 1), rotl16(xor3(TE0(s1, 2), TE1(s2, 3), k3)));
  s0 = t0; s1 = t1; s2 = t2; s3 = t3;
}

// Two independent blocks per call, written so the 32 lookups of a round are
// issued together and the scheduler is told to keep them together: 32 address
// perms, 32 DS reads, then the 24 combining ops (T19 sched_group_barrier).
__device__ __forceinline__ void aes_round2(uint32_t (&a)[4], uint32_t (&b)[4], uint32_t k0,
                                           uint32_t k1, uint32_t k2, uint32_t k3,
                                           uint32_t laneoff) {
  uint32_t ta[16], tb[16];
#pragma unroll
  for (int c = 0; c < 4; c++) {
    ta[4 * c + 0] = TE0(a[c], 0);
    ta[4 * c + 1] = TE1(a[(c + 1) & 3], 1);
    ta[4 * c + 2] = TE0(a[(c + 2) & 3], 2);
    ta[4 * c + 3] = TE1(a[(c + 3) & 3], 3);
  }
#pragma unroll
  for (int c = 0; c < 4; c++) {
    tb[4 * c + 0] = TE0(b[c], 0);
    tb[4 * c + 1] = TE1(b[(c + 1) & 3], 1);
    tb[4 * c + 2] = TE0(b[(c + 2) & 3], 2);
    tb[4 * c + 3] = TE1(b[(c + 3) & 3], 3);
  }
  const uint32_t k[4] = {k0, k1, k2, k3};
#pragma unroll
  for (int c = 0; c < 4; c++)
    a[c] = xor3(ta[4 * c], ta[4 * c + 1], rotl16(xor3(ta[4 * c + 2], ta[4 * c + 3], k[c])));
#pragma unroll
  for (int c = 0; c < 4; c++)
    b[c] = xor3(tb[4 * c], tb[4 * c + 1], rotl16(xor3(tb[4 * c + 2], tb[4 * c + 3], k[c])));
  __builtin_amdgcn_sched_group_barrier(0x002, 16, 0);  // A addresses
  __builtin_amdgcn_sched_group_barrier(0x100, 16, 0);  // A lookups
  __builtin_amdgcn_sched_group_barrier(0x002, 16, 0);  // B addresses
  __builtin_amdgcn_sched_group_barrier(0x100, 16, 0);  // B lookups
  __builtin_amdgcn_sched_group_barrier(0x002, 24, 0);  // combine
}

// Final round: SubBytes/ShiftRows only.  S[x] is byte 1 (and 2) of Te0_le[x]
// and byte 3 of Te1_le[x].
__device__ __forceinline__ uint32_t last_col(uint32_t a, uint32_t b, uint32_t c, uint32_t d,
                                             uint32_t k, uint32_t laneoff) {
  uint32_t lo = __builtin_amdgcn_perm(TE0(b, 1), TE0(a, 0), 0x0C0C0501u);
  uint32_t hi = __builtin_amdgcn_perm(TE1(d, 3), TE0(c, 2), 0x07020C0Cu);
  return lo ^ hi ^ k;
}
__device__ __forceinline__ void aes_last(uint32_t& s0, uint32_t& s1, uint32_t& s2, uint32_t& s3,
                                         cu32* rk, uint32_t laneoff) {
  uint32_t t0 = last_col(s0, s1, s2, s3, rk[0], laneoff);
  uint32_t t1 = last_col(s1, s2, s3, s0, rk[1], laneoff);
  uint32_t t2 = last_col(s2, s3, s0, s1, rk[2], laneoff);
  uint32_t t3 = last_col(s3, s0, s1, s2, rk[3], laneoff);
  s0 = t0; s1 = t1; s2 = t2; s3 = t3;
}

// Full block encryption (used for E_K(J0)).
template <int ROUNDS>
__device__ __forceinline__ void aes_block(uint32_t s[4], cu32* rk, cu32* rkr,
                                          uint32_t laneoff) {
  s[0] ^= rk[0]; s[1] ^= rk[1]; s[2] ^= rk[2]; s[3] ^= rk[3];
#pragma unroll
  for (int r = 1; r < ROUNDS; r++)
    aes_round(s[0], s[1], s[2], s[3], rkr[4 * r], rkr[4 * r + 1], rkr[4 * r + 2], rkr[4 * r + 3],
              laneoff);
  aes_last(s[0], s[1], s[2], s[3], rk + 4 * ROUNDS, laneoff);
}

// Per-record CTR constants: J0 columns 0..2 through AddRoundKey 0 and the
// constant three quarters of round 1 (only column 3 carries the counter).
struct CtrConst { uint32_t k1[4]; uint32_t rk03; };

__device__ __forceinline__ CtrConst ctr_setup(const uint32_t j0[4], cu32* rk,
                                              uint32_t laneoff) {
  uint32_t s0 = j0[0] ^ rk[0], s1 = j0[1] ^ rk[1], s2 = j0[2] ^ rk[2];
  CtrConst c;
  c.k1[0] = TE0(s0, 0) ^ TE1(s1, 1) ^ rotl16(TE0(s2, 2)) ^ rk[4];
  c.k1[1] = TE0(s1, 0) ^ TE1(s2, 1) ^ rotl16(TE1(s0, 3)) ^ rk[5];
  c.k1[2] = TE0(s2, 0) ^ rotl16(TE0(s0, 2) ^ TE1(s1, 3)) ^ rk[6];
  c.k1[3] = TE1(s0, 1) ^ rotl16(TE0(s1, 2) ^ TE1(s2, 3)) ^ rk[7];
  c.rk03 = rk[3];
  return c;
}

// Keystream block for 32-bit counter value ctr (big-endian in bytes 12..15),
// general form: only round 1 is shortened.
template <int ROUNDS>
__device__ __forceinline__ void aes_ctr(uint32_t ks[4], uint32_t ctr, const CtrConst& c,
                                        cu32* rk, cu32* rkr, uint32_t laneoff) {
  uint32_t v = bswap32(ctr) ^ c.rk03;
  uint32_t s0 = c.k1[0] ^ rotl16(TE1(v, 3));
  uint32_t s1 = c.k1[1] ^ rotl16(TE0(v, 2));
  uint32_t s2 = c.k1[2] ^ TE1(v, 1);
  uint32_t s3 = c.k1[3] ^ TE0(v, 0);
#pragma unroll
  for (int r = 2; r < ROUNDS; r++)
    aes_round(s0, s1, s2, s3, rkr[4 * r], rkr[4 * r + 1], rkr[4 * r + 2], rkr[4 * r + 3], laneoff);
  aes_last(s0, s1, s2, s3, rk + 4 * ROUNDS, laneoff);
  ks[0] = s0; ks[1] = s1; ks[2] = s2; ks[3] = s3;
}

// Per-record constants for counters below 2^16 (every TLS record: the counter
// runs 2..nb+1 with nb <= 65534).  Counter bytes 12-13 are then zero, so after
// round 1 only columns 0 and 1 depend on the counter and round 2 needs 8
// lookups instead of 16; E_K(J0) rides along.  Computed for 64 records at a
// time (one per lane) and broadcast with readlane when a record is processed.
struct RecConsts {
  uint32_t ek0[4];   // E_K(J0)
  uint32_t k1a, k1b; // round-1 constants of columns 0, 1
  uint32_t k2[4];    // round-2 constants
};

template <int ROUNDS>
__device__ __forceinline__ RecConsts rec_consts(const uint32_t j0[4], cu32* rk, cu32* rkr,
                                                uint32_t laneoff) {
  RecConsts r;
  uint32_t e[4] = {j0[0], j0[1], j0[2], j0[3]};
  aes_block<ROUNDS>(e, rk, rkr, laneoff);
  r.ek0[0] = e[0]; r.ek0[1] = e[1]; r.ek0[2] = e[2]; r.ek0[3] = e[3];
  CtrConst c = ctr_setup(j0, rk, laneoff);
  const uint32_t v0 = c.rk03;           // counter bytes 12..15 = 0 (bytes 12,13 stay 0)
  const uint32_t s2 = c.k1[2] ^ TE1(v0, 1);
  const uint32_t s3 = c.k1[3] ^ TE0(v0, 0);
  r.k1a = c.k1[0];
  r.k1b = c.k1[1];
  r.k2[0] = rotl16(TE0(s2, 2) ^ TE1(s3, 3)) ^ rk[8];
  r.k2[1] = TE1(s2, 1) ^ rotl16(TE0(s3, 2)) ^ rk[9];
  r.k2[2] = TE0(s2, 0) ^ TE1(s3, 1) ^ rk[10];
  r.k2[3] = TE0(s3, 0) ^ rotl16(TE1(s2, 3)) ^ rk[11];
  return r;
}

// Fast keystream for ctr < 2^16: round 1 = 2 lookups, round 2 = 8 lookups.
template <int ROUNDS>
__device__ __forceinline__ void aes_ctr16(uint32_t ks[4], uint32_t ctr, const RecConsts& c,
                                          uint32_t rk03, cu32* rk, cu32* rkr, uint32_t laneoff) {
  const uint32_t v = bswap32(ctr) ^ rk03;
  const uint32_t s0 = c.k1a ^ rotl16(TE1(v, 3));
  const uint32_t s1 = c.k1b ^ rotl16(TE0(v, 2));
  uint32_t t0 = xor3(c.k2[0], TE0(s0, 0), TE1(s1, 1));
  uint32_t t1 = xor3(c.k2[1], TE0(s1, 0), rotl16(TE1(s0, 3)));
  uint32_t t2 = c.k2[2] ^ rotl16(TE0(s0, 2) ^ TE1(s1, 3));
  uint32_t t3 = xor3(c.k2[3], TE1(s0, 1), rotl16(TE0(s1, 2)));
#pragma unroll
  for (int r = 3; r < ROUNDS; r++)
    aes_round(t0, t1, t2, t3, rkr[4 * r], rkr[4 * r + 1], rkr[4 * r + 2], rkr[4 * r + 3], laneoff);
  aes_last(t0, t1, t2, t3, rk + 4 * ROUNDS, laneoff);
  ks[0] = t0; ks[1] = t1; ks[2] = t2; ks[3] = t3;
}

// Two keystream blocks (counters c0, c1) with interleaved rounds.
template <int ROUNDS>
__device__ __forceinline__ void aes_ctr16x2(uint32_t ka[4], uint32_t kb[4], uint32_t c0,
                                            uint32_t c1, const RecConsts& c, uint32_t rk03,
                                            cu32* rk, cu32* rkr, uint32_t laneoff) {
  const uint32_t va = bswap32(c0) ^ rk03, vb = bswap32(c1) ^ rk03;
  const uint32_t a0 = c.k1a ^ rotl16(TE1(va, 3)), a1 = c.k1b ^ rotl16(TE0(va, 2));
  const uint32_t b0 = c.k1a ^ rotl16(TE1(vb, 3)), b1 = c.k1b ^ rotl16(TE0(vb, 2));
  uint32_t A[4], B[4];
  A[0] = xor3(c.k2[0], TE0(a0, 0), TE1(a1, 1));
  A[1] = xor3(c.k2[1], TE0(a1, 0), rotl16(TE1(a0, 3)));
  A[2] = c.k2[2] ^ rotl16(TE0(a0, 2) ^ TE1(a1, 3));
  A[3] = xor3(c.k2[3], TE1(a0, 1), rotl16(TE0(a1, 2)));
  B[0] = xor3(c.k2[0], TE0(b0, 0), TE1(b1, 1));
  B[1] = xor3(c.k2[1], TE0(b1, 0), rotl16(TE1(b0, 3)));
  B[2] = c.k2[2] ^ rotl16(TE0(b0, 2) ^ TE1(b1, 3));
  B[3] = xor3(c.k2[3], TE1(b0, 1), rotl16(TE0(b1, 2)));
#pragma unroll
  for (int r = 3; r < ROUNDS; r++)
    aes_round2(A, B, rkr[4 * r], rkr[4 * r + 1], rkr[4 * r + 2], rkr[4 * r + 3], laneoff);
  aes_last(A[0], A[1], A[2], A[3], rk + 4 * ROUNDS, laneoff);
  aes_last(B[0], B[1], B[2], B[3], rk + 4 * ROUNDS, laneoff);
#pragma unroll
  for (int w = 0; w < 4; w++) { ka[w] = A[w]; kb[w] = B[w]; }
}

// ---------------------------------------------------------------------------
// GHASH helpers.  The record code (gcm_blocks*, gcm_finish, gcm_record_x4) is
// generic in a GHASH policy G with two members:
//   G::mul64(x, o)      o = x * H^64 (LE words), the per-lane Horner step;
//   G::shoup(X, e, Z)   Z = X * H^e, e = 1..65 (BE words), the chain weights.
// GhLane: the session's 64 KiB byte-position table and Shoup tables in LDS,
// shared by the workgroup (queue kernel, one session per run).  GhNib
// (gcm_pw.hip): a per-wave 8 KiB nibble-position table and Shoup tables read
// from HBM/L2 (per-wave-session kernel, any session per wave).
struct GhLane {
  bool c2, c1;       // word-rotation selects for m = lane % 16
  uint32_t r;        // byte rotation
  uint32_t cq[4];    // slot bytes: cq[q].byte[i] = ((4q + i + m) & 15) * 16
  __device__ __forceinline__ void mul64(const uint32_t x[4], uint32_t o[4]) const;
  __device__ __forceinline__ void shoup(const uint32_t X[4], uint32_t e, uint32_t Z[4]) const;
};

// GhLane plus the session's lengths-block table at LEN_OFF (load_len_table):
// the queue kernel's policy.  gcm_finish then takes LEN * H from the table
// instead of folding the lengths block into a lane chain (gcm_close_len).
struct GhLaneLen : GhLane {};
// GhLaneLen whose chain weights take one reduction per multiply
// (mul_shoup_fold): the queue kernel's no-pack variants.
struct GhLaneFold : GhLane {
  __device__ __forceinline__ void shoup(const uint32_t X[4], uint32_t e, uint32_t Z[4]) const;
};
template <class G> inline constexpr bool gh_has_len_table = false;
template <> inline constexpr bool gh_has_len_table<GhLaneLen> = true;
template <> inline constexpr bool gh_has_len_table<GhLaneFold> = true;

__device__ __forceinline__ GhLane gh_lane(uint32_t lane) {
  GhLane g;
  uint32_t m = lane & 15;
  g.c2 = (m >> 3) & 1;
  g.c1 = (m >> 2) & 1;
  g.r = m & 3;
#pragma unroll
  for (int q = 0; q < 4; q++) {
    uint32_t v = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) v |= (((4 * q + i + m) & 15) << 4) << (8 * i);
    g.cq[q] = v;
  }
  return g;
}

template <int K>
__device__ __forceinline__ uint32_t kaddr(uint32_t y, uint32_t cq) {
  return __builtin_amdgcn_perm(y, cq, 0x0C0C0000u | ((4u + K) << 8) | K);
}

// out = x * H^64 using the LDS byte-position table (LE words).
__device__ __forceinline__ void mul_k(const uint32_t x[4], uint32_t o[4], const GhLane& g) {
  uint32_t a0 = g.c2 ? x[2] : x[0], a1 = g.c2 ? x[3] : x[1];
  uint32_t a2 = g.c2 ? x[0] : x[2], a3 = g.c2 ? x[1] : x[3];
  uint32_t b0 = g.c1 ? a1 : a0, b1 = g.c1 ? a2 : a1, b2 = g.c1 ? a3 : a2, b3 = g.c1 ? a0 : a3;
  uint32_t y[4];
  y[0] = __builtin_amdgcn_alignbyte(b1, b0, g.r);
  y[1] = __builtin_amdgcn_alignbyte(b2, b1, g.r);
  y[2] = __builtin_amdgcn_alignbyte(b3, b2, g.r);
  y[3] = __builtin_amdgcn_alignbyte(b0, b3, g.r);
  uint4 acc = make_uint4(0, 0, 0, 0);
#pragma unroll
  for (int q = 0; q < 4; q++) {
    uint4 v0 = lds_u128(KT_OFF + kaddr<0>(y[q], g.cq[q]));
    uint4 v1 = lds_u128(KT_OFF + kaddr<1>(y[q], g.cq[q]));
    uint4 v2 = lds_u128(KT_OFF + kaddr<2>(y[q], g.cq[q]));
    uint4 v3 = lds_u128(KT_OFF + kaddr<3>(y[q], g.cq[q]));
    acc.x = xor3(acc.x, xor3(v0.x, v1.x, v2.x), v3.x);
    acc.y = xor3(acc.y, xor3(v0.y, v1.y, v2.y), v3.y);
    acc.z = xor3(acc.z, xor3(v0.z, v1.z, v2.z), v3.z);
    acc.w = xor3(acc.w, xor3(v0.w, v1.w, v2.w), v3.w);
  }
  o[0] = acc.x; o[1] = acc.y; o[2] = acc.z; o[3] = acc.w;
}

// Two independent chains at once: o_a = x_a * H^64, o_b = x_b * H^64, with all
// 32 lookups issued before any is combined (the chains' latencies overlap).
__device__ __forceinline__ void mul_k2(const uint32_t xa[4], const uint32_t xb[4], uint32_t oa[4],
                                       uint32_t ob[4], const GhLane& g) {
  uint32_t addr[2][16];
  const uint32_t* xs[2] = {xa, xb};
#pragma unroll
  for (int c = 0; c < 2; c++) {
    const uint32_t* x = xs[c];
    uint32_t a0 = g.c2 ? x[2] : x[0], a1 = g.c2 ? x[3] : x[1];
    uint32_t a2 = g.c2 ? x[0] : x[2], a3 = g.c2 ? x[1] : x[3];
    uint32_t b0 = g.c1 ? a1 : a0, b1 = g.c1 ? a2 : a1, b2 = g.c1 ? a3 : a2, b3 = g.c1 ? a0 : a3;
    uint32_t y[4];
    y[0] = __builtin_amdgcn_alignbyte(b1, b0, g.r);
    y[1] = __builtin_amdgcn_alignbyte(b2, b1, g.r);
    y[2] = __builtin_amdgcn_alignbyte(b3, b2, g.r);
    y[3] = __builtin_amdgcn_alignbyte(b0, b3, g.r);
#pragma unroll
    for (int q = 0; q < 4; q++) {
      addr[c][4 * q + 0] = KT_OFF + kaddr<0>(y[q], g.cq[q]);
      addr[c][4 * q + 1] = KT_OFF + kaddr<1>(y[q], g.cq[q]);
      addr[c][4 * q + 2] = KT_OFF + kaddr<2>(y[q], g.cq[q]);
      addr[c][4 * q + 3] = KT_OFF + kaddr<3>(y[q], g.cq[q]);
    }
  }
  // two halves of 8 lookups per chain: at most 16 reads (64 VGPRs) in flight
  uint4 acc[2];
#pragma unroll
  for (int h = 0; h < 2; h++) {
    uint4 v[2][8];
#pragma unroll
    for (int m = 0; m < 8; m++) {
      v[0][m] = lds_u128(addr[0][8 * h + m]);
      v[1][m] = lds_u128(addr[1][8 * h + m]);
    }
#pragma unroll
    for (int c = 0; c < 2; c++) {
      uint4 t;
      t.x = xor3(v[c][0].x, v[c][1].x, v[c][2].x);
      t.y = xor3(v[c][0].y, v[c][1].y, v[c][2].y);
      t.z = xor3(v[c][0].z, v[c][1].z, v[c][2].z);
      t.w = xor3(v[c][0].w, v[c][1].w, v[c][2].w);
#pragma unroll
      for (int m = 3; m < 7; m += 2) {
        t.x = xor3(t.x, v[c][m].x, v[c][m + 1].x);
        t.y = xor3(t.y, v[c][m].y, v[c][m + 1].y);
        t.z = xor3(t.z, v[c][m].z, v[c][m + 1].z);
        t.w = xor3(t.w, v[c][m].w, v[c][m + 1].w);
      }
      if (h == 0) {
        acc[c].x = t.x ^ v[c][7].x; acc[c].y = t.y ^ v[c][7].y;
        acc[c].z = t.z ^ v[c][7].z; acc[c].w = t.w ^ v[c][7].w;
      } else {
        acc[c].x = xor3(acc[c].x, t.x, v[c][7].x); acc[c].y = xor3(acc[c].y, t.y, v[c][7].y);
        acc[c].z = xor3(acc[c].z, t.z, v[c][7].z); acc[c].w = xor3(acc[c].w, t.w, v[c][7].w);
      }
    }
  }
  oa[0] = acc[0].x; oa[1] = acc[0].y; oa[2] = acc[0].z; oa[3] = acc[0].w;
  ob[0] = acc[1].x; ob[1] = acc[1].y; ob[2] = acc[1].z; ob[3] = acc[1].w;
}

// LDS address of the Shoup table of H^e (e = 1..65); entry v at + v * 256.
__device__ __forceinline__ uint32_t sh_base(uint32_t e) {
  const uint32_t i = e - 1;
  return SH_OFF + (i >> 4) * 4096u + (i & 15u) * 16u;
}

// rem_4bit[r] >> 32 (gcm128.c:327-331) on the VALU: (r * 0xE1, carry-less) << 21,
// 0xE1 = x^0 + x^5 + x^6 + x^7, so r*0xE1 = r ^ ((r ^ r<<1 ^ r<<2) << 5).  (A
// 16-entry LDS table read with a random index costs 3-4-way bank conflicts.)
__device__ __forceinline__ uint32_t rem4(uint32_t r) {
  const uint32_t a = xor3(r, r << 1, r << 2);
  return (r << 21) ^ (a << 26);
}

// z = x * H^e (Shoup 4-bit, gcm128.c:333-393), all in big-endian words.
__device__ __forceinline__ void mul_shoup(const uint32_t X[4], uint32_t e, uint32_t Z[4]) {
  const uint32_t base = sh_base(e);
  uint32_t n0 = X[3] & 0xF;
  uint4 m = lds_u128(base + n0 * 256);
  uint32_t z0 = m.x, z1 = m.y, z2 = m.z, z3 = m.w;
#pragma unroll
  for (int k = 1; k < 32; k++) {
    uint32_t nib = (X[3 - k / 8] >> (4 * (k % 8))) & 0xF;
    uint32_t rem = z3 & 0xF;
    z3 = __builtin_amdgcn_alignbit(z2, z3, 4);
    z2 = __builtin_amdgcn_alignbit(z1, z2, 4);
    z1 = __builtin_amdgcn_alignbit(z0, z1, 4);
    z0 = (z0 >> 4) ^ rem4(rem);
    uint4 t = lds_u128(base + nib * 256);
    z0 ^= t.x; z1 ^= t.y; z2 ^= t.z; z3 ^= t.w;
  }
  Z[0] = z0; Z[1] = z1; Z[2] = z2; Z[3] = z3;
}

// The same product with its table reads issued ahead of the chain (round 3):
// the reads depend only on x's nibbles, but the compiler waited for each read
// right after issuing it, so a multiply cost 32 LDS round trips in series.
// Used by the per-record finish (GhLane::shoup); the pack path keeps
// mul_shoup, whose lanes hold their plaintext through the multiply (the
// look-ahead registers made that kernel spill 60 VGPRs).
constexpr int kShoupAhead = 4;
__device__ __forceinline__ void mul_shoup_ahead(const uint32_t X[4], uint32_t e, uint32_t Z[4]) {
  const uint32_t base = sh_base(e);
  uint4 t[32];
#pragma unroll
  for (int k = 0; k < 32; k++) t[k] = lds_u128(base + ((X[3 - k / 8] >> (4 * (k % 8))) & 0xF) * 256);
  uint32_t z0 = t[0].x, z1 = t[0].y, z2 = t[0].z, z3 = t[0].w;
#pragma unroll
  for (int k = 1; k < 32; k++) {
    const uint32_t rem = z3 & 0xF;
    z3 = __builtin_amdgcn_alignbit(z2, z3, 4);
    z2 = __builtin_amdgcn_alignbit(z1, z2, 4);
    z1 = __builtin_amdgcn_alignbit(z0, z1, 4);
    z0 = (z0 >> 4) ^ rem4(rem);
    z0 ^= t[k].x; z1 ^= t[k].y; z2 ^= t[k].z; z3 ^= t[k].w;
  }
  // schedule: kShoupAhead reads first, then one read per chain step
  __builtin_amdgcn_sched_group_barrier(0x100, kShoupAhead, 0);
#pragma unroll
  for (int k = 0; k < 32 - kShoupAhead; k++) {
    __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
    __builtin_amdgcn_sched_group_barrier(0x002, 10, 0);
  }
  Z[0] = z0; Z[1] = z1; Z[2] = z2; Z[3] = z3;
}

// One reduction for a whole multiply.  s(Z) = (Z >> 4) ^ rem4(Z & 0xF) is the
// multiplication by x^4 modulo the GCM polynomial and linear, so the Horner
// sum of mul_shoup, sum_k s^(31-k)(T[nib_k]), may be added up unreduced as the
// 256-bit value W = sum_k (T[nib_k] << 128) >> 4 (31 - k) (BE words, W[0] the
// high one; its low four bits are zero) and reduced once: bit 127 - j of
// O = W[4..7] stands for x^(128 + j) = x^j (1 + x + x^2 + x^7), so
// Z = W[0..3] ^ O ^ (O >> 1) ^ (O >> 2) ^ (O >> 7).  Of the bits the shifts
// drop only bits 6..4 of O can be set (in O >> 7: x^(128 + j'), j' = 0..2);
// they are folded the same way once more, within the high word.
__device__ __forceinline__ void gh_fold(const uint32_t W[8], uint32_t Z[4]) {
  const uint32_t* O = W + 4;
  const uint32_t t = O[3] << 25;
  Z[0] = xor3(W[0], O[0], O[0] >> 1) ^ xor3(O[0] >> 2, O[0] >> 7, xor3(t, t >> 1, t >> 2)) ^ (t >> 7);
#pragma unroll
  for (int w = 1; w < 4; w++)
    Z[w] = xor3(W[w], O[w], __builtin_amdgcn_alignbit(O[w - 1], O[w], 1)) ^
           __builtin_amdgcn_alignbit(O[w - 1], O[w], 2) ^ __builtin_amdgcn_alignbit(O[w - 1], O[w], 7);
}

// z = x * H^e as mul_shoup gives it (the same 32 table reads), with gh_fold's
// single reduction instead of a 31-step dependent chain.  The four nibbles at
// bit 4 j of X[0..3] share the bit shift 4 (7 - j), and their entries lie whole
// words apart (X[c]'s c words down): group j XORs its four entries into a
// seven-word sum by word placement, shifts that once across the words and adds
// it to W.  The next group's reads are issued before a group is combined (8
// reads, 32 VGPRs, in flight at the most); shifts and nibble positions are
// inline constants.  The queue kernels' record finish (GhLaneFold).
__device__ __forceinline__ void mul_shoup_fold(const uint32_t X[4], uint32_t e, uint32_t Z[4]) {
  const uint32_t base = sh_base(e);
  uint32_t W[8];
  uint4 tt[2][4];
#pragma unroll
  for (int c = 0; c < 4; c++) tt[1][c] = lds_u128(base + ((X[c] >> 28) & 0xF) * 256);
#pragma unroll
  for (int j = 7; j >= 0; j--) {
    const uint4* t = tt[j & 1];
    if (j > 0) {
#pragma unroll
      for (int c = 0; c < 4; c++) tt[(j - 1) & 1][c] = lds_u128(base + ((X[c] >> (4 * (j - 1))) & 0xF) * 256);
    }
    uint32_t S[7];
    S[0] = t[0].x;
    S[1] = t[0].y ^ t[1].x;
    S[2] = xor3(t[0].z, t[1].y, t[2].x);
    S[3] = xor3(t[0].w, t[1].z, t[2].y) ^ t[3].x;
    S[4] = xor3(t[1].w, t[2].z, t[3].y);
    S[5] = t[2].w ^ t[3].z;
    S[6] = t[3].w;
    if (j == 7) {  // no shift; W's low word is still empty
#pragma unroll
      for (int w = 0; w < 7; w++) W[w] = S[w];
      W[7] = 0;
    } else {
      const int sh = 4 * (7 - j);
      W[0] ^= S[0] >> sh;
#pragma unroll
      for (int w = 1; w < 7; w++) W[w] ^= __builtin_amdgcn_alignbit(S[w - 1], S[w], sh);
      W[7] ^= S[6] << (32 - sh);
    }
    // W group by group: left to itself the compiler sums word by word over
    // all eight groups, with all 32 reads (128 VGPRs) in flight
    asm volatile("" : "+v"(W[0]), "+v"(W[1]), "+v"(W[2]), "+v"(W[3]), "+v"(W[4]), "+v"(W[5]),
                      "+v"(W[6]), "+v"(W[7]));
  }
  gh_fold(W, Z);
}

__device__ __forceinline__ void GhLane::mul64(const uint32_t x[4], uint32_t o[4]) const {
  mul_k(x, o, *this);
}
__device__ __forceinline__ void GhLane::shoup(const uint32_t X[4], uint32_t e, uint32_t Z[4]) const {
  mul_shoup_ahead(X, e, Z);
}
__device__ __forceinline__ void GhLaneFold::shoup(const uint32_t X[4], uint32_t e, uint32_t Z[4]) const {
  mul_shoup_fold(X, e, Z);
}

// Two independent Shoup multiplies, interleaved; e == 0 gives zero.
__device__ __forceinline__ void mul_shoup2(const uint32_t A[4], uint32_t ea, uint32_t ZA[4],
                                           const uint32_t B[4], uint32_t eb, uint32_t ZB[4]) {
  // empty chains (e == 0) read the H^1 table and are masked to zero at the end
  const uint32_t base_a = sh_base(ea ? ea : 1), base_b = sh_base(eb ? eb : 1);
  const uint32_t ma = ea ? 0xFFFFFFFFu : 0u, mb = eb ? 0xFFFFFFFFu : 0u;
  uint4 m = lds_u128(base_a + (A[3] & 0xF) * 256);
  uint4 n = lds_u128(base_b + (B[3] & 0xF) * 256);
  uint32_t a0 = m.x, a1 = m.y, a2 = m.z, a3 = m.w;
  uint32_t b0 = n.x, b1 = n.y, b2 = n.z, b3 = n.w;
#pragma unroll
  for (int k = 1; k < 32; k++) {
    const uint32_t na = (A[3 - k / 8] >> (4 * (k % 8))) & 0xF;
    const uint32_t nb = (B[3 - k / 8] >> (4 * (k % 8))) & 0xF;
    const uint32_t ra = a3 & 0xF, rb = b3 & 0xF;
    const uint4 ta = lds_u128(base_a + na * 256), tb = lds_u128(base_b + nb * 256);
    const uint32_t qa = rem4(ra), qb = rem4(rb);
    a3 = __builtin_amdgcn_alignbit(a2, a3, 4);
    a2 = __builtin_amdgcn_alignbit(a1, a2, 4);
    a1 = __builtin_amdgcn_alignbit(a0, a1, 4);
    a0 = (a0 >> 4) ^ qa;
    b3 = __builtin_amdgcn_alignbit(b2, b3, 4);
    b2 = __builtin_amdgcn_alignbit(b1, b2, 4);
    b1 = __builtin_amdgcn_alignbit(b0, b1, 4);
    b0 = (b0 >> 4) ^ qb;
    a0 ^= ta.x; a1 ^= ta.y; a2 ^= ta.z; a3 ^= ta.w;
    b0 ^= tb.x; b1 ^= tb.y; b2 ^= tb.z; b3 ^= tb.w;
  }
  ZA[0] = a0 & ma; ZA[1] = a1 & ma; ZA[2] = a2 & ma; ZA[3] = a3 & ma;
  ZB[0] = b0 & mb; ZB[1] = b1 & mb; ZB[2] = b2 & mb; ZB[3] = b3 & mb;
}

// Serial GHASH over a byte string with H (all lanes redundantly, rare path:
// non-96-bit IVs and RAW-mode AAD).  x is big-endian words.  When final_mul
// is false the last block is only XORed in (no trailing multiply).
__device__ void ghash_serial(uint32_t x[4], const uint8_t* p, uint64_t len, bool final_mul) {
  const bool al4 = ((uintptr_t)p & 3) == 0;
  for (uint64_t off = 0; off < len; off += 16) {
    uint32_t b[4] = {0, 0, 0, 0};
    if (al4) {  // whole words (a 4-B aligned word cannot cross a page), tail bytes masked
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const int64_t nb = (int64_t)(len - off) - 4 * k;
        if (nb > 0) {
          const uint32_t w = reinterpret_cast<const uint32_t*>(p + off)[k];
          b[k] = bswap32(nb >= 4 ? w : (w & ((1u << (8 * nb)) - 1u)));
        }
      }
    } else {
#pragma unroll
      for (int k = 0; k < 16; k++)
        if (off + k < len) b[k >> 2] |= (uint32_t)p[off + k] << (24 - 8 * (k & 3));
    }
    x[0] ^= b[0]; x[1] ^= b[1]; x[2] ^= b[2]; x[3] ^= b[3];
    if (off + 16 < len || final_mul) {
      uint32_t z[4];
      mul_shoup(x, 1, z);
      x[0] = z[0]; x[1] = z[1]; x[2] = z[2]; x[3] = z[3];
    }
  }
}

__device__ __forceinline__ void be_from_le(const uint32_t* l, uint32_t* b) {
  b[0] = bswap32(l[0]); b[1] = bswap32(l[1]); b[2] = bswap32(l[2]); b[3] = bswap32(l[3]);
}

// ---------------------------------------------------------------------------
// Memory helpers (records are byte-aligned in general).
__device__ __forceinline__ uint32_t load_u32_bytes(const uint8_t* p) {
  if (((uintptr_t)p & 3) == 0) return *reinterpret_cast<const uint32_t*>(p);  // one load, not four
  return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

// (load16_any / store16_any: tlsgpu_internal.h)
__device__ __forceinline__ void load_block(const uint8_t* p, uint32_t nbytes, bool aligned,
                                           uint32_t v[4]) {
  if (aligned && nbytes == 16) {
    uint4 t = *reinterpret_cast<const uint4*>(p);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  } else if (nbytes == 16) {
    load16_any(p, v);
  } else if (nbytes != 0 && ((uintptr_t)p & 15) == 0) {
    // a partial last block at a 16-B aligned address: one 16-B load (it cannot
    // cross a page) with the bytes past the end masked, not up to 15 byte loads
    const uint4 t = *reinterpret_cast<const uint4*>(p);
    const uint32_t w[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const int32_t b = (int32_t)nbytes - 4 * k;
      v[k] = w[k] & (b >= 4 ? 0xFFFFFFFFu : (b <= 0 ? 0u : ((1u << (8 * b)) - 1u)));
    }
  } else {
    v[0] = v[1] = v[2] = v[3] = 0;
#pragma unroll
    for (uint32_t k = 0; k < 16; k++)
      if (k < nbytes) v[k >> 2] |= (uint32_t)p[k] << (8 * (k & 3));
  }
}

__device__ __forceinline__ void store_block(uint8_t* p, uint32_t nbytes, bool aligned,
                                            const uint32_t v[4]) {
  if (nbytes == 16 && aligned) {
    *reinterpret_cast<uint4*>(p) = make_uint4(v[0], v[1], v[2], v[3]);
  } else if (nbytes == 16) {
    store16_any(p, v);
  } else {
#pragma unroll
    for (uint32_t k = 0; k < 16; k++)
      if (k < nbytes) p[k] = (uint8_t)(v[k >> 2] >> (8 * (k & 3)));
  }
}


// ---------------------------------------------------------------------------
// Per-record context after parsing (TLS descriptor or raw job).
struct RecCtx {
  const uint8_t* src;     // open: ciphertext ; seal: plaintext
  uint8_t* dst;           // open: plaintext  ; seal: ciphertext
  const uint8_t* tag_in;  // open: received tag (tag_len bytes)
  uint32_t tag_byte;      // open: tag_in[lane] for lane < tag_len, loaded at parse
                          // time so the tag check never waits on HBM
  uint8_t* tag_out;       // seal: where the tag goes
  uint32_t n;             // plaintext length (TLS 1.3: the inner plaintext, content || type)
  uint32_t inner;         // 0, or for a TLS 1.3 seal 0x100 | inner content type | the source
                          // length << 9: src holds that many content bytes, counted from
                          // the record's start (< 2^20, TLSGPU_MAX_RECORD), the byte after
                          // them is this type and zeros follow up to n (RFC 8446 5.2,
                          // 5.4); src is never read past the content.  One word, so the
                          // context is the TLS 1.2 kernels' and no wider than it was
  uint32_t j0[4];         // J0 (LE words)
  uint32_t aad_be[4];     // AAD' = Horner of the AAD blocks without the final
                          // multiply (gcm128.c:826-881 folded), BE words
  uint64_t aad_len;       // bytes of AAD (for the lengths block)
  uint64_t zero_len;      // bytes of dst zero-filled on failure
  int32_t ok_status;      // status written on success
};

// Bytes of the record that come from rc.src: all of them, or a TLS 1.3 seal's
// content (the type byte and the padding are synthesized).  The wide full-step
// loops count their steps over these, so the block that holds the type byte and
// the padding blocks always take a tail path (load_tail) and the step loops
// load 16 source bytes per block as before.  (min: the split kernel's context
// of a wave's range ends at rc.n, the source maybe later.)
__device__ __forceinline__ uint32_t src_bytes(const RecCtx& rc) {
  if constexpr (kTls13) return rc.inner ? min(rc.inner >> 9, rc.n) : rc.n;
  return rc.n;
}

// Block i of the record's input for the tail paths, `nbytes` (0..16) of it
// valid: load_block of the bytes that src holds, then a TLS 1.3 seal's inner
// content type in the one block that holds offset src_len.  A block that holds
// the type byte alone, and every padding block past it, loads nothing and is
// zero (a padding block's ciphertext is the key stream).
template <bool SEAL>
__device__ __forceinline__ void load_tail(const RecCtx& rc, uint32_t i, uint32_t nbytes,
                                          bool aligned, uint32_t v[4]) {
  if constexpr (!SEAL || !kTls13) {
    load_block(rc.src + 16u * i, nbytes, aligned, v);
  } else {
    const uint32_t ns = rc.inner ? rc.inner >> 9 : rc.n, off = 16u * i;  // the source length
    const uint32_t lb = min(nbytes, ns > off ? ns - off : 0u);
    load_block(rc.src + off, lb, aligned, v);
    if (rc.inner != 0 && (ns >> 4) == i && nbytes != 0) {  // the type byte is byte lb of this block
      const uint32_t t = (rc.inner & 0xFFu) << (8u * (lb & 3u));
#pragma unroll
      for (uint32_t w = 0; w < 4; w++) v[w] |= (lb >> 2) == w ? t : 0u;
    }
  }
}

// Close the lane chains of a record: the lengths block BE64(aad bits) ||
// BE64(ct bits) joins lane (nb % 64)'s chain at j = nb (gcm128.c:1477-1500),
// then each lane's value still needs the weight H^e, e = nb + 1 - (index of
// the chain's last element).  Returns the BE chain value and e (0 = empty).
template <class G>
__device__ __forceinline__ uint32_t gcm_close_chain(const RecCtx& rc, uint32_t (&x)[4],
                                                    uint32_t (&xb)[4], uint32_t lane,
                                                    const G& gl) {
  const uint32_t n = rc.n;
  const uint32_t nb = (n + 15) >> 4;
  const uint32_t lstar = nb & 63;
  uint32_t xk[4];
  gl.mul64(x, xk);
  if (lane == lstar) {
    uint64_t ab = rc.aad_len * 8, cb = (uint64_t)n * 8;
    x[0] = xk[0] ^ bswap32((uint32_t)(ab >> 32));
    x[1] = xk[1] ^ bswap32((uint32_t)ab);
    x[2] = xk[2] ^ bswap32((uint32_t)(cb >> 32));
    x[3] = xk[3] ^ bswap32((uint32_t)cb);
  }
  int32_t jlast;
  if (lane == lstar) {
    jlast = (int32_t)nb;
  } else if (lane < nb) {
    jlast = (int32_t)(lane + ((nb - 1 - lane) & ~63u));
  } else {
    jlast = (rc.aad_len != 0 && lane == 63) ? -1 : -2;  // -2: empty chain
  }
  be_from_le(x, xb);
  return jlast == -2 ? 0u : (uint32_t)((int32_t)nb + 1 - jlast);
}

// The same close without the all-lane multiply (policies with a lengths-block
// table, GhLaneLen).  gcm_close_chain gives lane l* = nb % 64 the value
// x * H^64 ^ LEN at weight H^1; that is x * H^65 ^ LEN * H, so here lane l*
// keeps x and takes the weight H^65 (its chain's last element is block
// nb - 64, or the AAD for nb = 63, or nothing: x = 0), and the caller adds
// LEN * H (len_term) to the wave sum.  Every other lane is as above.  Kernels
// whose AAD length varies per job (gcm_raw.h) or that have no room for the
// table (gcm_pw.hip) keep gcm_close_chain.
__device__ __forceinline__ uint32_t gcm_close_len(const RecCtx& rc, const uint32_t (&x)[4],
                                                  uint32_t (&xb)[4], uint32_t lane) {
  const uint32_t nb = (rc.n + 15) >> 4;
  be_from_le(x, xb);
  if (lane == (nb & 63)) return (uint32_t)kPowMax;
  if (lane < nb) return nb + 1 - (lane + ((nb - 1 - lane) & ~63u));
  return lane == 63 ? nb + 2 : 0u;  // the AAD alone (j = -1), or an empty chain
}

// This lane's share of LEN * H, LEN = BE64(AAD bits) || BE64(8 n) (BE words): lane
// p < kLenRows reads the entry of nibble p of the ciphertext bit count, lane
// kLenRows an AAD entry, the others a zero entry of row 7 — one ds_read_b128 for
// the wave; the wave sum of gcm_tag adds the shares up.  Row and nibble go
// through inline constants only, and the lane through an empty asm: nothing
// of this is kept in VGPRs across the step loop (lane constants and literals
// hoisted out of the record loop made the open kernels spill).
__device__ __forceinline__ uint4 len_term(const RecCtx& rc, uint32_t lane) {
  asm volatile("" : "+v"(lane));
  const uint32_t row = min(lane, 7u);
  const uint32_t nib = ((rc.n * 8u) >> (4u * row)) & 0xFu;
  return lds_u128(LEN_OFF + ((row << 8) + (nib << 4)));
}

// Zero n bytes at d (the plaintext of a record whose tag failed,
// evp_aead.c:137-143): the whole wave, 16-B stores for the aligned bulk (a
// byte loop made a tampered 16 KiB record's wave 256 store rounds long).
__device__ __forceinline__ void zero_fill_wave(uint8_t* d, uint64_t n, uint32_t lane) {
  const uint64_t head = min(n, (uint64_t)((16u - ((uintptr_t)d & 15u)) & 15u));
  if (lane < head) d[lane] = 0;
  uint4* b = reinterpret_cast<uint4*>(d + head);
  const uint64_t nb = (n - head) >> 4;
  for (uint64_t k = lane; k < nb; k += kWave) b[k] = make_uint4(0, 0, 0, 0);
  const uint64_t done = head + 16 * nb;
  if (lane < n - done) d[done + lane] = 0;
}

// Sum the weighted lane values across the wave, form the tag (GHASH ^ E_K(J0))
// and check it (open, constant time over the tag bytes, zero-fill on failure:
// e_aes.c:1492-1506, evp_aead.c:137-143) or write it (seal, e_aes.c:1452-1456).
template <bool SEAL>
__device__ __forceinline__ void gcm_tag(const RecCtx& rc, uint32_t (&y)[4], const uint32_t ek0[4],
                                        const DevSession* __restrict__ S, int32_t* status_slot,
                                        uint32_t lane) {
  y[0] = wave_xor_total(y[0]);
  y[1] = wave_xor_total(y[1]);
  y[2] = wave_xor_total(y[2]);
  y[3] = wave_xor_total(y[3]);
  // tag = GHASH ^ E_K(J0)  (y is BE words, ek0 LE words)
  uint32_t tag[4] = {bswap32(y[0]) ^ ek0[0], bswap32(y[1]) ^ ek0[1], bswap32(y[2]) ^ ek0[2],
                     bswap32(y[3]) ^ ek0[3]};
  const uint32_t tag_len = as_const(&S->tag_len)[0];
  const uint32_t tw = lane >> 2;
  const uint32_t tword = tw == 0 ? tag[0] : tw == 1 ? tag[1] : tw == 2 ? tag[2] : tag[3];
  const uint32_t tbyte = (tword >> (8 * (lane & 3))) & 0xFF;
  if (SEAL) {
    if (lane < tag_len) rc.tag_out[lane] = (uint8_t)tbyte;
    if (lane == 0) *status_slot = rc.ok_status;
  } else {
    uint32_t diff = 0;
    if (lane < tag_len) diff = rc.tag_byte ^ tbyte;
    bool bad = __any(diff != 0);  // constant-time in the data: every lane compares
    if (bad) {
      zero_fill_wave(rc.dst, rc.zero_len, lane);
    }
    if (lane == 0) *status_slot = bad ? TLSGPU_REC_BAD_MAC : rc.ok_status;
  }
}

// Finish one record (chains -> weights -> tag).
template <bool SEAL, class G>
__device__ __forceinline__ void gcm_finish(const RecCtx& rc, uint32_t (&x)[4], const uint32_t ek0[4],
                                           const DevSession* __restrict__ S, int32_t* status_slot,
                                           uint32_t lane, const G& gl) {
  uint32_t xb[4], y[4] = {0, 0, 0, 0};
  if constexpr (gh_has_len_table<G>) {
    const uint32_t e = gcm_close_len(rc, x, xb, lane);
    if (e != 0) gl.shoup(xb, e, y);
    const uint4 lt = len_term(rc, lane);
    y[0] ^= lt.x; y[1] ^= lt.y; y[2] ^= lt.z; y[3] ^= lt.w;
  } else {
    const uint32_t e = gcm_close_chain(rc, x, xb, lane, gl);
    if (e != 0) gl.shoup(xb, e, y);
  }
  gcm_tag<SEAL>(rc, y, ek0, S, status_slot, lane);
}

// Finish two records with their Shoup multiplies interleaved (two independent
// 32-step LDS chains per lane instead of two back-to-back ones).
template <bool SEAL>
__device__ __forceinline__ void gcm_finish2(const RecCtx (&rc)[2], uint32_t (&x)[2][4],
                                            const uint32_t (&ek)[2][4],
                                            const DevSession* __restrict__ S, int32_t* slot_a,
                                            int32_t* slot_b, uint32_t lane, const GhLane& gl) {
  uint32_t xb[2][4], y[2][4];
  const uint32_t ea = gcm_close_chain(rc[0], x[0], xb[0], lane, gl);
  const uint32_t eb = gcm_close_chain(rc[1], x[1], xb[1], lane, gl);
  mul_shoup2(xb[0], ea, y[0], xb[1], eb, y[1]);
  gcm_tag<SEAL>(rc[0], y[0], ek[0], S, slot_a, lane);
  gcm_tag<SEAL>(rc[1], y[1], ek[1], S, slot_b, lane);
}

// CTR en/decryption of blocks [start, nb) fused with the lane GHASH chains x
// (start is a multiple of 64: block i belongs to lane i % 64's chain).
// FAST: counters < 2^16 and the per-record constants `rcc` were precomputed
// (wave-uniform values); otherwise `cc` (ctr_setup) is used.
template <bool SEAL, int ROUNDS, bool FAST, class G>
__device__ __forceinline__ void gcm_blocks(const RecCtx& rc, const DevSession* __restrict__ S,
                                           const RecConsts& rcc, const CtrConst& cc,
                                           uint32_t (&x)[4], uint32_t start, uint32_t lane,
                                           uint32_t laneoff, const G& gl) {
  cu32* rk = as_const(S->rk);
  cu32* rkr = as_const(S->rk_rot);
  const uint32_t n = rc.n;
  const uint32_t nb = (n + 15) >> 4;
  const uint32_t rk03 = rk[3];
  auto keystream = [&](uint32_t ks[4], uint32_t ctr) {
    if (FAST)
      aes_ctr16<ROUNDS>(ks, ctr, rcc, rk03, rk, rkr, laneoff);
    else
      aes_ctr<ROUNDS>(ks, ctr, cc, rk, rkr, laneoff);
  };
  const uint32_t ctr0 = bswap32(rc.j0[3]) + 1u;  // inc32(J0), gcm128.c:815-823
  const bool aligned = ((((uintptr_t)rc.src) | ((uintptr_t)rc.dst)) & 15) == 0;

  // Full-block steps, two per iteration (two independent AES chains per lane
  // keep twice as many LDS lookups in flight), with the next iteration's
  // ciphertext loads issued before this iteration's AES.
  const uint32_t nfull_steps = (src_bytes(rc) >> 4) / kWave;  // never the type byte's block
  uint32_t base = start;
  if (nfull_steps >= start / kWave + 2) {
    uint32_t c0[4], c1[4];
    load_block(rc.src + 16u * (start + lane), 16, aligned, c0);
    load_block(rc.src + 16u * (start + lane + kWave), 16, aligned, c1);
    uint32_t t = start / kWave;
    for (; t + 2 <= nfull_steps; t += 2, base += 2 * kWave) {
      const uint32_t i = base + lane;
      uint32_t n0[4] = {0, 0, 0, 0}, n1[4] = {0, 0, 0, 0};
      if (t + 4 <= nfull_steps) {
        load_block(rc.src + 16u * (i + 2 * kWave), 16, aligned, n0);
        load_block(rc.src + 16u * (i + 3 * kWave), 16, aligned, n1);
      }
      uint32_t k0[4], k1[4];
      if (FAST) {
        aes_ctr16x2<ROUNDS>(k0, k1, ctr0 + i, ctr0 + i + kWave, rcc, rk03, rk, rkr, laneoff);
      } else {
        keystream(k0, ctr0 + i);
        keystream(k1, ctr0 + i + kWave);
      }
      uint32_t o0[4] = {c0[0] ^ k0[0], c0[1] ^ k0[1], c0[2] ^ k0[2], c0[3] ^ k0[3]};
      uint32_t o1[4] = {c1[0] ^ k1[0], c1[1] ^ k1[1], c1[2] ^ k1[2], c1[3] ^ k1[3]};
      store_block(rc.dst + 16u * i, 16, aligned, o0);
      store_block(rc.dst + 16u * (i + kWave), 16, aligned, o1);
      uint32_t xk[4];
      gl.mul64(x, xk);
      const uint32_t* g0 = SEAL ? o0 : c0;
      const uint32_t* g1 = SEAL ? o1 : c1;
      x[0] = xk[0] ^ g0[0]; x[1] = xk[1] ^ g0[1]; x[2] = xk[2] ^ g0[2]; x[3] = xk[3] ^ g0[3];
      gl.mul64(x, xk);
      x[0] = xk[0] ^ g1[0]; x[1] = xk[1] ^ g1[1]; x[2] = xk[2] ^ g1[2]; x[3] = xk[3] ^ g1[3];
#pragma unroll
      for (int w = 0; w < 4; w++) { c0[w] = n0[w]; c1[w] = n1[w]; }
    }
  }
  // Two remaining steps at a time when the first is full (short records have
  // no full step pairs; this halves their serial AES latency), masked second.
  if (FAST) {
    for (; base + kWave < nb; base += 2 * kWave) {
      const uint32_t i0 = base + lane, i1 = i0 + kWave;  // i0 < nb always
      const bool a1 = i1 < nb;
      const uint32_t nb0 = min(16u, n - 16u * i0), nb1 = a1 ? min(16u, n - 16u * i1) : 0u;
      uint32_t in0[4], in1[4], k0[4], k1[4];
      load_tail<SEAL>(rc, i0, nb0, aligned, in0);
      load_tail<SEAL>(rc, i1, nb1, aligned, in1);
      aes_ctr16x2<ROUNDS>(k0, k1, ctr0 + i0, ctr0 + i1, rcc, rk[3], rk, as_const(S->rk_rot), laneoff);
#pragma unroll
      for (int w = 0; w < 4; w++) {
        const int32_t b0 = (int32_t)nb0 - 4 * w, b1 = (int32_t)nb1 - 4 * w;
        k0[w] &= b0 >= 4 ? 0xFFFFFFFFu : (b0 <= 0 ? 0u : ((1u << (8 * b0)) - 1u));
        k1[w] &= b1 >= 4 ? 0xFFFFFFFFu : (b1 <= 0 ? 0u : ((1u << (8 * b1)) - 1u));
      }
      uint32_t o0[4] = {in0[0] ^ k0[0], in0[1] ^ k0[1], in0[2] ^ k0[2], in0[3] ^ k0[3]};
      uint32_t o1[4] = {in1[0] ^ k1[0], in1[1] ^ k1[1], in1[2] ^ k1[2], in1[3] ^ k1[3]};
      store_block(rc.dst + 16u * i0, nb0, aligned, o0);
      if (a1) store_block(rc.dst + 16u * i1, nb1, aligned, o1);
      uint32_t xk[4];
      gl.mul64(x, xk);
      const uint32_t* g0 = SEAL ? o0 : in0;
      x[0] = xk[0] ^ g0[0]; x[1] = xk[1] ^ g0[1]; x[2] = xk[2] ^ g0[2]; x[3] = xk[3] ^ g0[3];
      gl.mul64(x, xk);
      if (a1) {
        const uint32_t* g1 = SEAL ? o1 : in1;
        x[0] = xk[0] ^ g1[0]; x[1] = xk[1] ^ g1[1]; x[2] = xk[2] ^ g1[2]; x[3] = xk[3] ^ g1[3];
      }
    }
  }
  // Remaining steps (odd full step, partial wave, partial last block).
  for (; base < nb; base += kWave) {
    const uint32_t i = base + lane;
    const bool active = i < nb;
    const uint32_t nbytes = active ? min(16u, n - 16u * i) : 0u;
    uint32_t in[4];
    load_tail<SEAL>(rc, i, nbytes, aligned, in);
    uint32_t ks[4];
    keystream(ks, ctr0 + i);
#pragma unroll
    for (int w = 0; w < 4; w++) {  // zero-padded GHASH block for the partial tail
      int32_t b = (int32_t)nbytes - 4 * w;
      uint32_t keep = b >= 4 ? 0xFFFFFFFFu : (b <= 0 ? 0u : ((1u << (8 * b)) - 1u));
      ks[w] &= keep;
    }
    uint32_t ob[4] = {in[0] ^ ks[0], in[1] ^ ks[1], in[2] ^ ks[2], in[3] ^ ks[3]};
    if (active) store_block(rc.dst + 16u * i, nbytes, aligned, ob);
    uint32_t xk[4];
    gl.mul64(x, xk);
    if (active) {
      const uint32_t* c = SEAL ? ob : in;
      x[0] = xk[0] ^ c[0]; x[1] = xk[1] ^ c[1]; x[2] = xk[2] ^ c[2]; x[3] = xk[3] ^ c[3];
    }
  }

}

// GHASH(AAD || C || lengths) with the lane chains described in the header,
// fused with CTR en/decryption.  Checks the tag (open) or writes it (seal).
template <bool SEAL, int ROUNDS, bool FAST>
__device__ void gcm_record(const RecCtx& rc, const DevSession* __restrict__ S,
                           const RecConsts& rcc, int32_t* status_slot, uint32_t lane,
                           uint32_t laneoff, const GhLane& gl) {
  cu32* rk = as_const(S->rk);
  cu32* rkr = as_const(S->rk_rot);
  uint32_t ek0[4];
  CtrConst cc;
  if (FAST) {
    ek0[0] = rcc.ek0[0]; ek0[1] = rcc.ek0[1]; ek0[2] = rcc.ek0[2]; ek0[3] = rcc.ek0[3];
  } else {
    ek0[0] = rc.j0[0]; ek0[1] = rc.j0[1]; ek0[2] = rc.j0[2]; ek0[3] = rc.j0[3];
    aes_block<ROUNDS>(ek0, rk, rkr, laneoff);
    cc = ctr_setup(rc.j0, rk, laneoff);
  }
  // Horner chain state (LE words).  The AAD' element sits at j = -1, i.e. in
  // lane 63's chain one H^64 step before C_63.
  uint32_t x[4] = {0, 0, 0, 0};
  if (rc.aad_len != 0 && lane == 63) {
    x[0] = bswap32(rc.aad_be[0]); x[1] = bswap32(rc.aad_be[1]);
    x[2] = bswap32(rc.aad_be[2]); x[3] = bswap32(rc.aad_be[3]);
  }
  gcm_blocks<SEAL, ROUNDS, FAST>(rc, S, rcc, cc, x, 0, lane, laneoff, gl);
  gcm_finish<SEAL>(rc, x, ek0, S, status_slot, lane, gl);
}

// ---------------------------------------------------------------------------
// L2 prefetch: one dword of each 128-B line of [p, p + bytes), N lines per
// lane.  Ordinary (cached) loads whose values are handed to an empty asm at
// prefetch_done(), so the compiler counts them in vmcnt and waits for them
// only there; as the wave's oldest loads they have long completed by then.
template <int N>
struct Prefetch {
  uint32_t v[N];
};
template <int N>
__device__ __forceinline__ Prefetch<N> l2_prefetch(const uint8_t* p, uint32_t bytes, uint32_t lane) {
  Prefetch<N> f;
#pragma unroll
  for (int k = 0; k < N; k++) {
    const uint32_t off = (uint32_t)(k * 64 + lane) * 128u;
    f.v[k] = off < bytes ? *reinterpret_cast<const uint32_t*>(p + off) : 0u;
  }
  return f;
}
template <int N>
__device__ __forceinline__ void prefetch_done(const Prefetch<N>& f) {
#pragma unroll
  for (int k = 0; k < N; k++) asm volatile("" ::"v"(f.v[k]));
}

// ---------------------------------------------------------------------------
// Phase timing (diagnostic, BatchArgs::dbg != null, env TLSGPU_PHASE_STATS):
// shader-clock cycles per phase summed over waves, dbg[2i] = cycles,
// dbg[2i+1] = events.
struct PhaseClock {
  unsigned long long* dbg;
  uint64_t t;
  __device__ __forceinline__ PhaseClock(unsigned long long* d) : dbg(d), t(d ? __builtin_amdgcn_s_memtime() : 0) {}
  // counters live in LDS (DBG_OFF) during the launch; the kernel flushes them
  __device__ __forceinline__ void lap(int i, uint32_t lane) {
    if (dbg) {
      const uint64_t n = __builtin_amdgcn_s_memtime();
      if (lane == 0) {
        unsigned long long* c = reinterpret_cast<unsigned long long*>(s_lds + DBG_OFF);
        atomicAdd(c + 2 * i, (unsigned long long)(n - t));
        atomicAdd(c + 2 * i + 1, 1ull);
      }
      t = __builtin_amdgcn_s_memtime();
    }
  }
};
// A lap on a clock the caller may not have (hand-over slots 0, 7, 8: the queue
// kernel's no-pack variants without a bitsliced role pass one, started before
// the plain claim; the pack variants and the other callers none).
__device__ __forceinline__ void lap_if(PhaseClock* c, int i, uint32_t lane) {
  if (c) c->lap(i, lane);
}
// Slots of the hand-over interval (queue kernel, T-table role)
constexpr int kLapDesc = 0;    // claim -> descriptor arrived
constexpr int kLapConsts = 7;  // descriptor -> bounds, parse, RecPre constants ready
constexpr int kLapFirst = 8;   // constants ready -> first group's loads issued, AES next

// ---------------------------------------------------------------------------
// NB-block T-table keystream (the hybrid kernel's T-table waves run alone on
// their SIMD's LDS share, so they keep 16 * NB lookups in flight per round).
template <int NB>
__device__ __forceinline__ void aes_roundN(uint32_t (&s)[NB][4], uint32_t k0, uint32_t k1,
                                           uint32_t k2, uint32_t k3, uint32_t laneoff) {
  uint32_t t[NB][16];
#pragma unroll
  for (int b = 0; b < NB; b++)
#pragma unroll
    for (int c = 0; c < 4; c++) {
      t[b][4 * c + 0] = TE0(s[b][c], 0);
      t[b][4 * c + 1] = TE1(s[b][(c + 1) & 3], 1);
      t[b][4 * c + 2] = TE0(s[b][(c + 2) & 3], 2);
      t[b][4 * c + 3] = TE1(s[b][(c + 3) & 3], 3);
    }
  const uint32_t k[4] = {k0, k1, k2, k3};
#pragma unroll
  for (int b = 0; b < NB; b++)
#pragma unroll
    for (int c = 0; c < 4; c++)
      s[b][c] = xor3(t[b][4 * c], t[b][4 * c + 1], rotl16(xor3(t[b][4 * c + 2], t[b][4 * c + 3], k[c])));
#ifdef TG_SCHED_HINTS  // measured 3 % slower than the compiler schedule (queue kernel)
#pragma unroll
  for (int b = 0; b < NB; b++) {
    __builtin_amdgcn_sched_group_barrier(0x002, 16, 0);  // addresses of block b
    __builtin_amdgcn_sched_group_barrier(0x100, 16, 0);  // its lookups
  }
  __builtin_amdgcn_sched_group_barrier(0x002, 12 * NB, 0);  // combine
#endif
}

// Rounds 3 .. ROUNDS of NB blocks whose state after round 2 is in A (the
// round-2 cache below).  aes_ctr16xN keeps these rounds in its own body:
// calling this tail from it gave the queue kernel's pack variants another
// schedule (4 -> 14 VGPR spills), and their code is to stay as it is.
template <int NB, int ROUNDS, class Hook>
__device__ __forceinline__ void aes_ctr16xN_tail(uint32_t (&ks)[NB][4], uint32_t (&A)[NB][4],
                                                 cu32* rk, cu32* rkr, uint32_t laneoff,
                                                 Hook&& hook) {
#pragma unroll
  for (int r = 3; r < ROUNDS; r++) {
    aes_roundN<NB>(A, rkr[4 * r], rkr[4 * r + 1], rkr[4 * r + 2], rkr[4 * r + 3], laneoff);
    hook(r);  // work independent of A (GHASH of the previous group) between rounds
  }
#pragma unroll
  for (int b = 0; b < NB; b++) {
    aes_last(A[b][0], A[b][1], A[b][2], A[b][3], rk + 4 * ROUNDS, laneoff);
#pragma unroll
    for (int w = 0; w < 4; w++) ks[b][w] = A[b][w];
  }
}

// NB keystream blocks for counters ctr[b] < 2^16 (aes_ctr16 generalised).
template <int NB, int ROUNDS, class Hook>
__device__ __forceinline__ void aes_ctr16xN(uint32_t (&ks)[NB][4], const uint32_t (&ctr)[NB],
                                            const RecConsts& c, uint32_t rk03, cu32* rk,
                                            cu32* rkr, uint32_t laneoff, Hook&& hook) {
  uint32_t A[NB][4];
#pragma unroll
  for (int b = 0; b < NB; b++) {
    const uint32_t v = bswap32(ctr[b]) ^ rk03;
    const uint32_t s0 = c.k1a ^ rotl16(TE1(v, 3)), s1 = c.k1b ^ rotl16(TE0(v, 2));
    A[b][0] = xor3(c.k2[0], TE0(s0, 0), TE1(s1, 1));
    A[b][1] = xor3(c.k2[1], TE0(s1, 0), rotl16(TE1(s0, 3)));
    A[b][2] = c.k2[2] ^ rotl16(TE0(s0, 2) ^ TE1(s1, 3));
    A[b][3] = xor3(c.k2[3], TE1(s0, 1), rotl16(TE0(s1, 2)));
  }
#pragma unroll
  for (int r = 3; r < ROUNDS; r++) {
    aes_roundN<NB>(A, rkr[4 * r], rkr[4 * r + 1], rkr[4 * r + 2], rkr[4 * r + 3], laneoff);
    hook(r);  // work independent of A (GHASH of the previous group) between rounds
  }
#pragma unroll
  for (int b = 0; b < NB; b++) {
    aes_last(A[b][0], A[b][1], A[b][2], A[b][3], rk + 4 * ROUNDS, laneoff);
#pragma unroll
    for (int w = 0; w < 4; w++) ks[b][w] = A[b][w];
  }
}

// ---------------------------------------------------------------------------
// Round-2 cache (the queue kernel's open no-pack variants of the TLS 1.2
// unit).
// For a counter below 2^16 the state after round 2 separates exactly,
//   state2(ctr) = F(ctr & 0xFF) ^ G(ctr >> 8) ^ k2,
// F the four T-table words fed by s0 = k1a ^ rotl16(TE1(v, 3)) and G the four
// fed by s1 = k1b ^ rotl16(TE0(v, 2)) in aes_ctr16xN above.  A record's block
// i runs in lane i % 64 at step i / 64 with counter 2 + i (J0 = IV || 1), so a
// lane's low counter byte at step s is that of step s & 3: four F variants per
// lane and record, k2 folded in, 20 lookups instead of 5 per block.  The high
// byte is s >> 2 in lanes 0..61 and (s + 1) >> 2 in lanes 62 and 63, which
// carry one step early — it is not wave-uniform.  G is looked up once per four
// steps, at s % 4 == 0, for the high byte of step s + 3: the value of all four
// steps in lanes 0..61 and of step s + 3 only in lanes 62 and 63, which take
// lanes 58..61's words (r2c_before_carry) for the three steps before.
__device__ __forceinline__ void r2c_build_f(uint32_t (&F)[4][4], uint32_t ctr_lane,
                                            const RecConsts& c, uint32_t rk03, uint32_t laneoff) {
#pragma unroll
  for (int v = 0; v < 4; v++) {
    const uint32_t x = bswap32(ctr_lane + kWave * v) ^ rk03;
    const uint32_t s0 = c.k1a ^ rotl16(TE1(x, 3));
    F[v][0] = c.k2[0] ^ TE0(s0, 0);
    F[v][1] = c.k2[1] ^ rotl16(TE1(s0, 3));
    F[v][2] = c.k2[2] ^ rotl16(TE0(s0, 2));
    F[v][3] = c.k2[3] ^ TE1(s0, 1);
  }
}
__device__ __forceinline__ void r2c_lookup_g(uint32_t (&G)[4], uint32_t ctr, const RecConsts& c,
                                             uint32_t rk03, uint32_t laneoff) {
  const uint32_t x = bswap32(ctr) ^ rk03;
  const uint32_t s1 = c.k1b ^ rotl16(TE0(x, 2));
  G[0] = TE1(s1, 1);
  G[1] = TE0(s1, 0);
  G[2] = rotl16(TE1(s1, 3));
  G[3] = rotl16(TE0(s1, 2));
}
// G of the steps before lanes 62 and 63 carry: lanes 60..63 take the word of
// the lane two below (row_shr:2 on row 3, bank 3), every other lane its own.
__device__ __forceinline__ uint32_t r2c_before_carry(uint32_t g) {
  return (uint32_t)__builtin_amdgcn_update_dpp((int)g, (int)g, 0x112, 0x8, 0x8, false);
}
template <int NB, int ROUNDS>
__device__ __forceinline__ void aes_ctr16xN(uint32_t (&ks)[NB][4], const uint32_t (&ctr)[NB],
                                            const RecConsts& c, uint32_t rk03, cu32* rk,
                                            cu32* rkr, uint32_t laneoff) {
  aes_ctr16xN<NB, ROUNDS>(ks, ctr, c, rk03, rk, rkr, laneoff, [](int) {});
}

// Full NB-step groups of a record (any alignment) from block `start` on (FAST
// constants only): NB keystream blocks per lane in flight, the next group's
// input loads issued first, and the GHASH of NB blocks folded into the AES
// rounds (the chain's LDS round trips then overlap the AES lookups instead of
// trailing them).  GHASH runs over ciphertext:
//   * seal, and open without OWN: each group's blocks (gp) are hashed in the
//     rounds of the following group, step b after round 3 + 2b; the first
//     group runs without the hook and the last group's NB steps follow the
//     loop (seal's ciphertext is the output; open without OWN is the same
//     order, kept where the other order was measured slower: DESIGN.md §4.1);
//   * open with OWN: the ciphertext is the input, in c[b] before the group's
//     AES starts, so every group — the first included — hashes its own blocks
//     in its own rounds; nothing is carried to the next group and no GHASH
//     step follows the loop.  A record's first group (its ciphertext loads
//     were issued just before) takes step b after round FR0 + FRS * b, so a
//     caller can put the wave's wait for those loads some rounds later.
// R2C: rounds 1 and 2 from the per-lane round-2 cache above instead of ten
// lookups per block (NB = 2 and start = 0 only; the F variants are built behind
// the first group's loads, G at every fourth step, so nothing of an earlier
// record is seen).
// Advances `start` past the groups done; the caller finishes the record with
// gcm_blocks.
template <bool SEAL, int ROUNDS, int NB, class G, bool OWN = false, int FR0 = 3, int FRS = 2,
          bool R2C = false>
__device__ __forceinline__ void gcm_blocks_xN(const RecCtx& rc, const DevSession* __restrict__ S,
                                              const RecConsts& rcc, uint32_t (&x)[4],
                                              uint32_t& start, uint32_t lane, uint32_t laneoff,
                                              const G& gl, PhaseClock* hc = nullptr) {
  const bool aligned = ((((uintptr_t)rc.src) | ((uintptr_t)rc.dst)) & 15) == 0;
#ifndef TG_XN_UNALIGNED
  if (!aligned) return;
#endif
  cu32* rk = as_const(S->rk);
  cu32* rkr = as_const(S->rk_rot);
  const uint32_t rk03 = rk[3];
  const uint32_t ctr0 = bswap32(rc.j0[3]) + 1u;
  const uint32_t nfull_steps = (src_bytes(rc) >> 4) / kWave;  // never the type byte's block
  uint32_t t = start / kWave;
  if (t + NB > nfull_steps) return;
  constexpr bool kLateGh = SEAL || !OWN;  // hash a group in the next group's rounds
  uint32_t c[NB][4];
  [[maybe_unused]] uint32_t gp[NB][4];  // the previous group's ciphertext (kLateGh)
#pragma unroll
  for (int b = 0; b < NB; b++) load_block(rc.src + 16u * (start + kWave * b + lane), 16, aligned, c[b]);
  auto ghash_step = [&](int b) {
    uint32_t xk[4];
    gl.mul64(x, xk);
    const uint32_t(&g)[4] = kLateGh ? gp[b] : c[b];  // own rounds: the group's own input
    x[0] = xk[0] ^ g[0]; x[1] = xk[1] ^ g[1]; x[2] = xk[2] ^ g[2]; x[3] = xk[3] ^ g[3];
  };
  // all NB steps fall inside rounds 3 .. ROUNDS-1 (aes_ctr16xN calls the hook there)
  static_assert(3 + 2 * (NB - 1) < ROUNDS, "GHASH steps must fit between the AES rounds");
  static_assert(FR0 >= 3 && FRS >= 1 && FR0 + FRS * (NB - 1) < ROUNDS,
                "the first group's GHASH steps must fit between the AES rounds");
  auto hook = [&](int r) {
#pragma unroll
    for (int b = 0; b < NB; b++)
      if (r == 3 + 2 * b) ghash_step(b);
  };
  [[maybe_unused]] auto hook_first = [&](int r) {
#pragma unroll
    for (int b = 0; b < NB; b++)
      if (r == FR0 + FRS * b) ghash_step(b);
  };
  [[maybe_unused]] uint32_t F2[4][4], G2[4];  // the round-2 cache (R2C)
  if constexpr (R2C) {
    static_assert(NB == 2, "the round-2 cache's step map is that of two blocks per lane");
    if (start != 0) return;  // t even and a G lookup in the first trip (the caller's tail is right)
    r2c_build_f(F2, ctr0 + lane, rcc, rk03, laneoff);
  }
  lap_if(hc, kLapFirst, lane);  // the first group's loads are issued, not waited for
  bool first = true;
  for (; t + NB <= nfull_steps; t += NB, start += NB * kWave) {
    const uint32_t i = start + lane;
    uint32_t nx[NB][4];
    if (t + 2 * NB <= nfull_steps) {
#pragma unroll
      for (int b = 0; b < NB; b++) load_block(rc.src + 16u * (i + kWave * (NB + b)), 16, aligned, nx[b]);
    }
    uint32_t ctr[NB], k[NB][4];
#pragma unroll
    for (int b = 0; b < NB; b++) ctr[b] = ctr0 + i + kWave * b;
    [[maybe_unused]] uint32_t A[NB][4];
    if constexpr (R2C) {
      // steps t (even) and t + 1: variants t & 3 and (t & 3) + 1, G of the
      // steps before the carry except at t + 1 = 3 mod 4
      // a wave-uniform branch on t & 2, so every F2 index is static: four
      // XORs per block, and the G lookup sits in the branch it belongs to
      // (one body with a masked select of the variants measured slower than
      // the ten lookups: profiles/r09_round2_cache.txt)
      if ((t & 2u) == 0) {
        r2c_lookup_g(G2, ctr0 + lane + kWave * (t + 3u), rcc, rk03, laneoff);
#pragma unroll
        for (int w = 0; w < 4; w++) {
          const uint32_t gb = r2c_before_carry(G2[w]);
          A[0][w] = F2[0][w] ^ gb;
          A[1][w] = F2[1][w] ^ gb;
        }
      } else {
#pragma unroll
        for (int w = 0; w < 4; w++) {
          A[0][w] = F2[2][w] ^ r2c_before_carry(G2[w]);
          A[1][w] = F2[3][w] ^ G2[w];
        }
      }
      if (first) {
        if constexpr (kLateGh)
          aes_ctr16xN_tail<NB, ROUNDS>(k, A, rk, rkr, laneoff, [](int) {});
        else
          aes_ctr16xN_tail<NB, ROUNDS>(k, A, rk, rkr, laneoff, hook_first);
      } else {
        aes_ctr16xN_tail<NB, ROUNDS>(k, A, rk, rkr, laneoff, hook);
      }
    } else if (first) {
      // a record's first group: no hook (nothing to hash yet), or its own rounds
      if constexpr (kLateGh)
        aes_ctr16xN<NB, ROUNDS>(k, ctr, rcc, rk03, rk, rkr, laneoff);
      else
        aes_ctr16xN<NB, ROUNDS>(k, ctr, rcc, rk03, rk, rkr, laneoff, hook_first);
    } else {
      aes_ctr16xN<NB, ROUNDS>(k, ctr, rcc, rk03, rk, rkr, laneoff, hook);
    }
    first = false;
#pragma unroll
    for (int b = 0; b < NB; b++) {
      uint32_t o[4] = {c[b][0] ^ k[b][0], c[b][1] ^ k[b][1], c[b][2] ^ k[b][2], c[b][3] ^ k[b][3]};
      store_block(rc.dst + 16u * (i + kWave * b), 16, aligned, o);
      if constexpr (kLateGh) {
#pragma unroll
        for (int w = 0; w < 4; w++) gp[b][w] = SEAL ? o[w] : c[b][w];
      }
    }
#pragma unroll
    for (int b = 0; b < NB; b++)
#pragma unroll
      for (int w = 0; w < 4; w++) c[b][w] = nx[b][w];
  }
  if constexpr (kLateGh) {
#pragma unroll
    for (int b = 0; b < NB; b++) ghash_step(b);  // the last group's GHASH
  }
}

// gcm_record<SEAL, ROUNDS, true> with the NB-wide full-block loop first.
// OWN: open hashes each group in its own AES rounds, a record's first group
// one round apart with the last step after round ROUNDS - 2 (the queue
// kernel's no-pack variants).
template <bool SEAL, int ROUNDS, int NB = 4, class G = GhLane, bool OWN = false, bool R2C = false>
__device__ void gcm_record_x4(const RecCtx& rc, const DevSession* __restrict__ S,
                              const RecConsts& rcc, int32_t* status_slot, uint32_t lane,
                              uint32_t laneoff, const G& gl,
                              unsigned long long* dbg = nullptr, PhaseClock* hc = nullptr) {
  PhaseClock pc(dbg);
  uint32_t x[4] = {0, 0, 0, 0};
  if (rc.aad_len != 0 && lane == 63) {
    x[0] = bswap32(rc.aad_be[0]); x[1] = bswap32(rc.aad_be[1]);
    x[2] = bswap32(rc.aad_be[2]); x[3] = bswap32(rc.aad_be[3]);
  }
  uint32_t start = 0;
  gcm_blocks_xN<SEAL, ROUNDS, NB, G, OWN, OWN ? ROUNDS - 1 - NB : 3, OWN ? 1 : 2, R2C>(
      rc, S, rcc, x, start, lane, laneoff, gl, hc);
#ifdef TG_XN_ODD_STEP
  // an odd full step left by the NB-wide loop: the pipelined one-step loop
  if (NB > 1) gcm_blocks_xN<SEAL, ROUNDS, 1>(rc, S, rcc, x, start, lane, laneoff, gl);
#endif
  pc.lap(9, lane);
  const CtrConst none = {};
  gcm_blocks<SEAL, ROUNDS, true>(rc, S, rcc, none, x, start, lane, laneoff, gl);
  pc.lap(10, lane);
  gcm_finish<SEAL>(rc, x, rcc.ek0, S, status_slot, lane, gl);
  pc.lap(11, lane);
}

__device__ __forceinline__ uint64_t uni64(uint64_t v) {
  return ((uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)(v >> 32)) << 32) |
         __builtin_amdgcn_readfirstlane((uint32_t)v);
}
__device__ __forceinline__ tlsgpu_record load_desc(const tlsgpu_record* p) {
  cu32* w = as_const(p);
  tlsgpu_record d;
  d.in_off = ((uint64_t)w[1] << 32) | w[0];
  d.out_off = ((uint64_t)w[3] << 32) | w[2];
  d.seq = ((uint64_t)w[5] << 32) | w[4];
  d.session = w[6];
  d.len_type = w[7];
  return d;
}

// J0 of record r for this lane (the batched constant pass): fixed IV(4) ||
// explicit nonce(8) || 0x00000001 — the explicit nonce is the record's first
// 8 bytes on open and the sequence number on seal (t1_enc.c:887-892, 941-948).
// TLS 1.3 (gcm_tls13): write IV(12) XOR (0^32 || BE64(seq)) || 0x00000001, both
// ways (RFC 8446 5.3).
__device__ __forceinline__ bool gcm_tls13(const DevSession* __restrict__) {
  return kTls13;  // per translation unit; the table's sessions are all of this generation
}
// words 1, 2 of the sequence-number nonce: seq alone (TLS 1.2 seal), or XORed
// into the TLS 1.3 write IV
__device__ __forceinline__ void seq_j0(const DevSession* __restrict__ S, bool t13, uint64_t seq,
                                       uint32_t j0[4]) {
  j0[1] = bswap32((uint32_t)(seq >> 32)) ^ (t13 ? as_const(S->fixed_nonce)[1] : 0u);
  j0[2] = bswap32((uint32_t)seq) ^ (t13 ? as_const(S->fixed_nonce)[2] : 0u);
}
template <bool SEAL>
__device__ __forceinline__ void lane_j0(const tlsgpu_record* D, uint32_t r, uint32_t run_end,
                                        const DevSession* __restrict__ S, const uint8_t* in,
                                        uint32_t j0[4]) {
  j0[0] = as_const(S->fixed_nonce)[0];
  j0[1] = j0[2] = 0;
  j0[3] = 0x01000000u;
  if (r >= run_end) return;
  const tlsgpu_record d = D[r];
  const bool t13 = gcm_tls13(S);
  if (SEAL || t13) {
    seq_j0(S, t13, d.seq, j0);
  } else if ((d.len_type & 0xFFFFFFu) >= 8) {
    const uint8_t* p = in + d.in_off;
    j0[1] = load_u32_bytes(p);
    j0[2] = load_u32_bytes(p + 4);
  }
}

// Build the per-record context from a TLS descriptor (t1_enc.c:832-975; for a
// TLS 1.3 session RFC 8446 5.2-5.3: no explicit nonce, the inner content type
// appended on seal, the 5-byte record header as AAD).  Returns false (and
// writes the status) when tls1_enc would return 0.  Open leaves a TLS 1.3
// record's inner plaintext length as its status; tls13_unpad_kernel turns it
// into the content length.
template <bool SEAL>
__device__ __forceinline__ bool parse_tls(const tlsgpu_record& d, const DevSession* __restrict__ S,
                                          const uint8_t* in, uint8_t* out, int32_t* status_slot,
                                          uint32_t lane, RecCtx& rc) {
  uint32_t len = d.len_type & 0xFFFFFFu;
  uint32_t type = d.len_type >> 24;
  const uint8_t* ip = in + d.in_off;
  uint8_t* op = out + d.out_off;
  uint32_t tag_len = as_const(&S->tag_len)[0];
  const bool t13 = gcm_tls13(S);
  const uint32_t eiv = t13 ? 0u : 8u;      // explicit nonce in the fragment
  // seal: the synthesized type byte and the session's padding (tls13_inner_len;
  // a record longer than 16384 is never padded, so the bound is the type byte's)
  uint32_t extra = 0;
  if constexpr (kTls13)
    extra = SEAL ? tls13_inner_len(len, as_const(&S->pad_mask)[0]) - len : 0u;
  if (SEAL ? len > TLSGPU_MAX_RECORD - (t13 ? 1u : 0u)
           : (len < eiv || len - eiv < tag_len || len - eiv - tag_len > TLSGPU_MAX_RECORD)) {
    if (lane == 0) *status_slot = TLSGPU_REC_PUBLIC_INVALID;
    return false;
  }
  uint32_t e1, e2;  // nonce words 1, 2
  if (SEAL) {
    rc.n = len + extra;
    rc.inner = t13 ? 0x100u | type | (len << 9) : 0u;
    rc.src = ip;
    rc.dst = op + eiv;
    rc.tag_out = op + eiv + rc.n;
    rc.tag_in = nullptr;
    if (lane < eiv) op[lane] = (uint8_t)(d.seq >> (56 - 8 * lane));  // explicit nonce into the record
    rc.ok_status = (int32_t)(rc.n + eiv + tag_len);
    rc.zero_len = 0;
  } else {
    rc.n = len - eiv - tag_len;
    rc.inner = 0;
    rc.src = ip + eiv;
    rc.dst = op;
    rc.tag_in = ip + eiv + rc.n;
    rc.tag_byte = lane < tag_len ? rc.tag_in[lane] : 0u;
    rc.tag_out = nullptr;
    rc.ok_status = (int32_t)rc.n;
    rc.zero_len = rc.n;
  }
  // TLS 1.2: nonce = fixed_iv(4) || explicit(8), the explicit nonce being the
  // sequence number (seal) or the fragment's first 8 bytes (open); TLS 1.3:
  // the write IV with the sequence number XORed in.  J0 = nonce || 0x00000001
  uint32_t sj[4];
  seq_j0(S, t13, d.seq, sj);
  if (SEAL || t13) {
    e1 = sj[1];
    e2 = sj[2];
  } else {
    e1 = (uint32_t)ip[0] | ((uint32_t)ip[1] << 8) | ((uint32_t)ip[2] << 16) | ((uint32_t)ip[3] << 24);
    e2 = (uint32_t)ip[4] | ((uint32_t)ip[5] << 8) | ((uint32_t)ip[6] << 16) | ((uint32_t)ip[7] << 24);
  }
  rc.j0[0] = as_const(S->fixed_nonce)[0];
  rc.j0[1] = e1;
  rc.j0[2] = e2;
  rc.j0[3] = 0x01000000u;
  if (t13) {
    // AAD = 0x17 0x03 0x03 BE16(ciphertext length with the tag), one zero-padded block
    const uint32_t cl = rc.n + tag_len;
    rc.aad_be[0] = 0x17030300u | ((cl >> 8) & 0xFF);
    rc.aad_be[1] = (cl & 0xFF) << 24;
    rc.aad_be[2] = rc.aad_be[3] = 0;
    rc.aad_len = 5;
  } else {
    // AAD = seq(8) || type || version(2) || length(2), one zero-padded block
    uint32_t v = as_const(&S->version)[0];
    rc.aad_be[0] = (uint32_t)(d.seq >> 32);
    rc.aad_be[1] = (uint32_t)d.seq;
    rc.aad_be[2] = (type << 24) | ((v & 0xFFFF) << 8) | ((rc.n >> 8) & 0xFF);
    rc.aad_be[3] = (rc.n & 0xFF) << 24;
    rc.aad_len = 13;
  }
  return true;
}

// Raw EVP_AEAD job (arbitrary nonce and AAD; e_aes.c:1424-1510).  The host
// already applied the argument checks of evp_aead.c / e_aes.c.
template <bool SEAL>
__device__ __forceinline__ void parse_raw(const RawJob& j, const DevSession* __restrict__ S,
                                          RecCtx& rc) {
  const uint8_t* ip = (const uint8_t*)j.in;
  uint8_t* op = (uint8_t*)j.out;
  const uint8_t* nonce = (const uint8_t*)j.nonce;
  uint32_t tag_len = as_const(&S->tag_len)[0];
  rc.inner = 0;
  if (SEAL) {
    rc.n = j.in_len;
    rc.src = ip;
    rc.dst = op;
    rc.tag_out = op + j.in_len;
    rc.tag_in = nullptr;
    rc.ok_status = (int32_t)(j.in_len + tag_len);
  } else {
    rc.n = j.in_len - tag_len;
    rc.src = ip;
    rc.dst = op;
    rc.tag_in = ip + rc.n;
    const uint32_t ln = threadIdx.x & 63;
    rc.tag_byte = ln < tag_len ? rc.tag_in[ln] : 0u;
    rc.tag_out = nullptr;
    rc.ok_status = (int32_t)rc.n;
  }
  rc.zero_len = j.max_out;
  if (j.nonce_len == 12) {
    rc.j0[0] = load_u32_bytes(nonce);
    rc.j0[1] = load_u32_bytes(nonce + 4);
    rc.j0[2] = load_u32_bytes(nonce + 8);
    rc.j0[3] = 0x01000000u;
  } else {  // J0 = GHASH(IV || pad || 0^64 || [len(IV)]_64)  (gcm128.c:770-812)
    uint32_t xb[4] = {0, 0, 0, 0};
    ghash_serial(xb, nonce, j.nonce_len, true);
    uint64_t bits = (uint64_t)j.nonce_len * 8;
    xb[2] ^= (uint32_t)(bits >> 32);
    xb[3] ^= (uint32_t)bits;
    uint32_t z[4];
    mul_shoup(xb, 1, z);
    rc.j0[0] = bswap32(z[0]); rc.j0[1] = bswap32(z[1]);
    rc.j0[2] = bswap32(z[2]); rc.j0[3] = bswap32(z[3]);
  }
  rc.aad_be[0] = rc.aad_be[1] = rc.aad_be[2] = rc.aad_be[3] = 0;
  rc.aad_len = j.aad_len;
  if (j.aad_len) ghash_serial(rc.aad_be, (const uint8_t*)j.aad, j.aad_len, false);
}

// ---------------------------------------------------------------------------
// Workgroup prologue / session table staging
template <int NT, bool R4 = true>
__device__ void fill_aes_lds() {
  for (uint32_t t = threadIdx.x; t < 1024; t += NT) {  // 1024 x 64 B = 64 KiB
    const uint32_t row = t >> 2, part = t & 3;
    uint32_t v = g_te0.v[row];
    if (part >= 2) v = rotl32(v, 8);  // Te1 = rotl8(Te0)
    uint4 w = make_uint4(v, v, v, v);
    uint4* dst = reinterpret_cast<uint4*>(s_lds + AES_OFF + row * 256 + part * 64);
    dst[0] = w; dst[1] = w; dst[2] = w; dst[3] = w;
  }
  const uint32_t t = threadIdx.x;
  if (R4 && t < 16) {  // rem_4bit >> 32 (gcm128.c:327-331), derived by four x-shifts
    uint64_t hi = 0, lo = t;
    for (int k = 0; k < 4; k++) {
      uint64_t c = lo & 1;
      lo = (lo >> 1) | (hi << 63);
      hi = (hi >> 1) ^ (c ? 0xE100000000000000ull : 0);
    }
    *reinterpret_cast<uint32_t*>(s_lds + R4_OFF + t * 4) = (uint32_t)(hi >> 32);
  }
}

// Expand the session's 128 basis vectors K*x^p into T[j][b] and copy the
// Shoup tables of H^1..H^65.
// OPAQUE (the queue kernel): the thread index goes through an empty asm, as in
// load_len_table, so the byte masks and the lane's copy address are computed
// here, once per session change, and not hoisted out of the caller's run loop
// into VGPRs that the record loop then lacks (they were that kernel's spilled
// values).  The other callers keep the plain index and their code.
template <int NT, bool OPAQUE = false>
__device__ void load_session_tables(const DevGcmTables* __restrict__ tab) {
  uint32_t tid = threadIdx.x;
  if constexpr (OPAQUE) asm volatile("" : "+v"(tid));
  const uint32_t bl = tid & 63;
  for (uint32_t jj = tid >> 6; jj < 16; jj += NT / kWave) {
    const uint32_t j = __builtin_amdgcn_readfirstlane(jj);  // byte position
    uint32_t lo[4] = {0, 0, 0, 0};
#ifdef TG_VECTOR_SESSION_LOADS
    // the persistent server: the wave's 8 basis entries in one lane-parallel
    // load (lane k < 8: x^(8j + 7 - k)), then lane reads — one memory round
    // trip instead of eight serialised uniform loads (round-4 trace: a key
    // change cost 4.3 µs)
    uint4 own = make_uint4(0, 0, 0, 0);
    if (bl < 8) own = *reinterpret_cast<const uint4*>(tab->basis[8 * j + 7 - bl]);
    struct LaneWord {
      uint4 v;
      __device__ __forceinline__ uint32_t operator()(int k, int c) const {
        const uint32_t w = c == 0 ? v.x : c == 1 ? v.y : c == 2 ? v.z : v.w;
        return (uint32_t)__builtin_amdgcn_readlane((int)w, k);
      }
    } bw{own};
#pragma unroll
    for (int k = 0; k < 6; k++) {   // bit k of the byte <-> x^(8j + 7 - k)
      uint32_t msk = 0u - ((bl >> k) & 1u);
      lo[0] ^= bw(k, 0) & msk; lo[1] ^= bw(k, 1) & msk; lo[2] ^= bw(k, 2) & msk; lo[3] ^= bw(k, 3) & msk;
    }
    const uint32_t b6[4] = {bw(6, 0), bw(6, 1), bw(6, 2), bw(6, 3)};  // x^(8j + 1)
    const uint32_t b7[4] = {bw(7, 0), bw(7, 1), bw(7, 2), bw(7, 3)};  // x^(8j)
#else
#pragma unroll
    for (int k = 0; k < 6; k++) {   // bit k of the byte <-> x^(8j + 7 - k)
      uint32_t msk = 0u - ((bl >> k) & 1u);
      cu32* bv = as_const(tab->basis[8 * j + 7 - k]);
      lo[0] ^= bv[0] & msk; lo[1] ^= bv[1] & msk; lo[2] ^= bv[2] & msk; lo[3] ^= bv[3] & msk;
    }
    cu32* b6 = as_const(tab->basis[8 * j + 1]);
    cu32* b7 = as_const(tab->basis[8 * j + 0]);
#endif
#pragma unroll
    for (int q = 0; q < 4; q++) {
      uint32_t m6 = (q & 1) ? 0xFFFFFFFFu : 0u, m7 = (q & 2) ? 0xFFFFFFFFu : 0u;
      uint4 v = make_uint4(lo[0] ^ (b6[0] & m6) ^ (b7[0] & m7), lo[1] ^ (b6[1] & m6) ^ (b7[1] & m7),
                           lo[2] ^ (b6[2] & m6) ^ (b7[2] & m7), lo[3] ^ (b6[3] & m6) ^ (b7[3] & m7));
      uint32_t b = bl + 64u * q;
      *reinterpret_cast<uint4*>(s_lds + KT_OFF + b * 256 + j * 16) = v;
    }
  }
  const uint4* sh = reinterpret_cast<const uint4*>(&tab->shoup[0][0][0]);
  for (uint32_t k = tid; k < kPowMax * 16; k += NT)  // k = 16 (e - 1) + v
    *reinterpret_cast<uint4*>(s_lds + sh_base(1 + (k >> 4)) + (k & 15u) * 256u) = sh[k];
}

// The session's lengths-block table (LEN_OFF, read by len_term), BE words:
// entry 16 p + v is (nibble v at nibble p of the ciphertext bit count) * H for
// p < kLenRows, BE64(ab) * H for p = kLenRows (ab = the AAD bits of parse_tls:
// 13 * 8 for TLS 1.2, 5 * 8 for TLS 1.3), zero for p = 7.  With T[v] the H^1
// Shoup entries and s() the 4-bit shift of
// mul_shoup, X * H is the Horner sum z = s(z) ^ T[nibble k] over X's nibbles
// k = 0..31 (k = 0: the low nibble of byte 15), so a nibble v alone at k gives
// s^(31 - k)(T[v]).  Reads the table in global memory, so it needs no barrier
// after load_session_tables' copy; the last two waves take it (the first
// have two entries of that copy each).
template <int NT>
__device__ void load_len_table(const DevGcmTables* __restrict__ tab) {
  constexpr uint32_t ab = kTls13 ? 5 * 8 : 13 * 8;  // AAD bits: nibble k = 16 is ab & 15, k = 17 is ab >> 4
  static_assert(ab < 256, "two nibbles");
  static_assert(NT >= (int)kLenEntries, "one entry per thread");
  const uint4* sh = reinterpret_cast<const uint4*>(&tab->shoup[0][0][0]);
  // the entry index through an empty asm: what derives from it is computed
  // here, once per run, not hoisted out of the caller's run loop into VGPRs
  // that the record loop then lacks
  uint32_t i = NT - 1 - threadIdx.x;
  asm volatile("" : "+v"(i));
  if (i >= kLenEntries) return;
  const uint32_t p = i >> 4;
  const bool aad = p == kLenRows;
  // s^(31 - k) as one shift by 4 (31 - k) bits and one gh_fold: nibble p < 6
  // moves down three words and 28 - 4 p bits, the AAD's nibbles 17 and 16 one
  // word and 24 and 28 bits
  const uint4 z = sh[aad ? ab >> 4 : i & 15u];
  const uint32_t r = aad ? 24u : 28u - 4u * p;
  uint32_t v[5];  // (z << 32) >> r
  v[0] = z.x >> r;
  v[1] = __builtin_amdgcn_alignbit(z.x, z.y, r);
  v[2] = __builtin_amdgcn_alignbit(z.y, z.z, r);
  v[3] = __builtin_amdgcn_alignbit(z.z, z.w, r);
  v[4] = __builtin_amdgcn_alignbit(z.w, 0u, r);  // (row 7: r = 0, zeroed below)
  if (aad) {
    const uint4 u = sh[ab & 15u];
    v[0] ^= u.x >> 28;
    v[1] ^= __builtin_amdgcn_alignbit(u.x, u.y, 28);
    v[2] ^= __builtin_amdgcn_alignbit(u.y, u.z, 28);
    v[3] ^= __builtin_amdgcn_alignbit(u.z, u.w, 28);
    v[4] ^= u.w << 4;
  }
  const uint32_t W[8] = {0u, aad ? v[0] : 0u, aad ? v[1] : 0u, aad ? v[2] : v[0],
                         aad ? v[3] : v[1], aad ? v[4] : v[2], aad ? 0u : v[3], aad ? 0u : v[4]};
  uint32_t f[4];
  gh_fold(W, f);
  uint4 o = make_uint4(f[0], f[1], f[2], f[3]);
  if (p > kLenRows) o = make_uint4(0, 0, 0, 0);
  *reinterpret_cast<uint4*>(s_lds + LEN_OFF + 16u * i) = o;
}

// Bitsliced round-key masks from the round-key words (SGPRs): s_bfe_i32
// sign-extends the key bit into 0 / ~0.
struct SgprMasks {
  cu32* rk;
  __device__ __forceinline__ uint32_t mask(int r, int i) const {
    return (uint32_t)__builtin_amdgcn_sbfe((int32_t)rk[4 * r + (i >> 5)], (uint32_t)(i & 31), 1u);
  }
};

__device__ __forceinline__ bool is_gcm(uint32_t kind) {
  return kind == TLSGPU_AES_128_GCM || kind == TLSGPU_AES_256_GCM;
}

}  // namespace tg
