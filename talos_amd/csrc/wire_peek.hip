// wire_peek.hip — tlsgpu_open_wire's KeyUpdate cut (RFC 8446 4.6.3, 7.2;
// include/tlsgpu.h "KeyUpdate on the wire read path").
//
// Every record behind a KeyUpdate is protected under the next traffic keys, so
// a stream's batch has to end at the KeyUpdate before anything behind it is
// opened (an open under the old keys fails the tag and zero-fills the
// ciphertext in place).  Whether a record is a KeyUpdate is known only after
// decryption; but all three TLS 1.3 suites are counter-mode ciphers, so a
// record's first 16 plaintext bytes cost one cipher block and no authentication:
//   AES-GCM   E_K(nonce || 00000002)      (J0 + 1: the first data counter)
//   ChaCha20  the block with counter 1    (counter 0 is the Poly1305 key)
//
//   wire_peek13_kernel      between wire_frame_kernel and the open, one wave
//                           per stream: peeks at each framed record's first
//                           block and cuts the stream after the first record
//                           that looks like a KeyUpdate alone in its record;
//   wire_ku_confirm_kernel  after wire_finish_kernel, one lane per stream: the
//                           verdict, from the record the open has verified.
// The peek is unauthenticated: it decides where the batch is cut and nothing
// else.  The cipher and framing kernels are not touched.
#include "aes_common.h"
#include "chacha_common.h"
#include "tlsgpu_internal.h"

namespace tg {

static __device__ const WordTable g_te0_peek = kTe0;

constexpr uint32_t kTag13 = 16;      // every TLS 1.3 suite here (valid_params)
constexpr uint32_t kKuInnerMin = 6;  // 18 00 00 01 rr || inner type 22
constexpr uint32_t kHandshake = 22;
constexpr uint32_t kKuMsgLen = 5;    // the KeyUpdate handshake message

__device__ __forceinline__ uint32_t peek_uni(uint32_t v) {
  return __builtin_amdgcn_readfirstlane(v);
}

// E_K(in): 16 bytes as little-endian (memory order) words in and out, the
// T-table cipher of gcm_stream.hip's aes_be with Te0 in LDS and the session's
// little-endian column round keys (wave-uniform).
__device__ __forceinline__ void peek_aes(const uint32_t* te, const uint32_t* __restrict__ rk,
                                         uint32_t rounds, const uint32_t in[4], uint32_t o[4]) {
  auto T0 = [&](uint32_t w, int b) { return te[(w >> (8 * b)) & 0xFF]; };
  auto T1 = [&](uint32_t w, int b) { return rotl32(te[(w >> (8 * b)) & 0xFF], 8); };
  auto SB = [&](uint32_t w, int b) { return (te[(w >> (8 * b)) & 0xFF] >> 8) & 0xFF; };
  uint32_t s0 = in[0] ^ rk[0], s1 = in[1] ^ rk[1], s2 = in[2] ^ rk[2], s3 = in[3] ^ rk[3];
  for (uint32_t r = 1; r < rounds; r++) {
    const uint32_t* k = rk + 4 * r;
    const uint32_t t0 = T0(s0, 0) ^ T1(s1, 1) ^ rotl32(T0(s2, 2) ^ T1(s3, 3), 16) ^ k[0];
    const uint32_t t1 = T0(s1, 0) ^ T1(s2, 1) ^ rotl32(T0(s3, 2) ^ T1(s0, 3), 16) ^ k[1];
    const uint32_t t2 = T0(s2, 0) ^ T1(s3, 1) ^ rotl32(T0(s0, 2) ^ T1(s1, 3), 16) ^ k[2];
    const uint32_t t3 = T0(s3, 0) ^ T1(s0, 1) ^ rotl32(T0(s1, 2) ^ T1(s2, 3), 16) ^ k[3];
    s0 = t0; s1 = t1; s2 = t2; s3 = t3;
  }
  const uint32_t* k = rk + 4 * rounds;
  o[0] = (SB(s0, 0) | (SB(s1, 1) << 8) | (SB(s2, 2) << 16) | (SB(s3, 3) << 24)) ^ k[0];
  o[1] = (SB(s1, 0) | (SB(s2, 1) << 8) | (SB(s3, 2) << 16) | (SB(s0, 3) << 24)) ^ k[1];
  o[2] = (SB(s2, 0) | (SB(s3, 1) << 8) | (SB(s0, 2) << 16) | (SB(s1, 3) << 24)) ^ k[2];
  o[3] = (SB(s3, 0) | (SB(s0, 1) << 8) | (SB(s1, 2) << 16) | (SB(s2, 3) << 24)) ^ k[3];
}

// The candidate predicate on the first nb = min(16, inner length) >= 6 bytes of a
// record's TLSInnerPlaintext (little-endian words; bytes from nb on are not the
// record's and do not count): 18 00 00 01 rr 16 00*, rr <= 1 — a KeyUpdate
// (handshake type 24, length 1, request_update rr) followed by the inner type
// 22 and zero padding only.
__device__ __forceinline__ bool ku_candidate(const uint32_t p[4], uint32_t nb) {
  auto mask = [&](uint32_t w) {  // the bytes of word w below nb
    const int32_t b = (int32_t)nb - 4 * (int32_t)w;
    return b >= 4 ? 0xFFFFFFFFu : b <= 0 ? 0u : (1u << (8 * b)) - 1u;
  };
  return p[0] == 0x01000018u && ((p[1] & mask(1)) & ~1u) == 0x00001600u && (p[2] & mask(2)) == 0 &&
         (p[3] & mask(3)) == 0;
}

// One wave per stream (four per workgroup, as wire_finish_kernel), 64 records
// per step; the session is the wave's, so the key is wave-uniform and only the
// nonce differs per lane.  The first candidate of the stream is found with a
// ballot (wire_gather_plan_kernel's pattern); the lanes behind it, in this step
// and every later one, put their descriptors back to all ones (unused slots:
// the open skips them and touches none of their bytes), and lane 0 rewrites the
// stream's result: records and delivered = the candidate's index + 1, consumed
// ends with its fragment, a header-level alert from behind the cut is dropped,
// key_update = TLSGPU_WIRE_KU_HELD until wire_ku_confirm_kernel says otherwise.
// Reads of d_wire: the first min(16, inner length) bytes of framed records, and
// only whole dwords that hold one of them (load16_any / load16_upto).
__global__ __launch_bounds__(256) void wire_peek13_kernel(
    const tlsgpu_wire_stream* __restrict__ streams, uint32_t n_streams, const uint8_t* wire,
    const DevSession* __restrict__ sessions, uint32_t n_sessions, uint32_t max_records,
    tlsgpu_record* __restrict__ recs, tlsgpu_wire_result* __restrict__ results) {
  __shared__ uint32_t te[256];
  te[threadIdx.x] = g_te0_peek.v[threadIdx.x];
  __syncthreads();
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t s = blockIdx.x * 4 + peek_uni(threadIdx.x >> 6);
  if (s >= n_streams) return;
  const tlsgpu_wire_stream st = streams[s];
  tlsgpu_wire_result r = results[s];
  const uint32_t sid = peek_uni(st.session);
  if (sid >= n_sessions) return;
  const DevSession* S = sessions + sid;
  const uint32_t kind = peek_uni(S->kind);
  if (!tls13_session(kind, peek_uni(S->nonce_in_record))) return;
  const uint32_t first = peek_uni(r.first), nrec = peek_uni(r.records);
  if ((uint64_t)first + nrec > max_records) return;  // (framing keeps a stream's slots inside)
  const bool chacha = kind == TLSGPU_CHACHA20_POLY1305_TLS13;
  const uint32_t rounds = peek_uni(S->rounds);
  const uint32_t* fx = reinterpret_cast<const uint32_t*>(S->fixed_nonce);
  const uint32_t fx0 = fx[0], fx1 = fx[1], fx2 = fx[2];
  tlsgpu_record ones;
  ones.in_off = ones.out_off = ones.seq = ~0ull;
  ones.session = ones.len_type = ~0u;

  bool cut = false;
  uint32_t cut_records = 0, cut_consumed = 0;
  for (uint32_t i0 = 0; i0 < nrec; i0 += 64) {
    const uint32_t i = i0 + lane;
    const bool in = i < nrec;
    tlsgpu_record* dp = recs + (size_t)first + i;
    if (cut) {  // behind the cut
      if (in) *dp = ones;
      continue;
    }
    bool cand = false;
    uint32_t end = 0;  // the fragment's end within the stream
    if (in) {
      const tlsgpu_record d = *dp;
      const uint32_t len = d.len_type & 0xFFFFFFu;
      const uint64_t rel = d.in_off - st.wire_off;
      // a fragment framing laid inside the stream, long enough for the message
      if (len >= kTag13 + kKuInnerMin && d.in_off >= st.wire_off && rel <= st.wire_len &&
          len <= st.wire_len - rel) {
        const uint32_t nb = min(16u, len - kTag13);
        const uint8_t* p = wire + d.in_off;
        uint32_t c[4], ks[4];
        if (nb == 16) load16_any(p, c);
        else load16_upto(p, nb, c);
        // the record nonce: write IV XOR (0^32 || BE64(seq)) (RFC 8446 5.3; seq_j0, cc_tls_rec)
        const uint32_t n1 = fx1 ^ bswap32((uint32_t)(d.seq >> 32)), n2 = fx2 ^ bswap32((uint32_t)d.seq);
        if (chacha) {  // the block with counter 1 (chacha-merged.c:230-236: counter in words 12-13)
          const uint32_t* kw = reinterpret_cast<const uint32_t*>(S->chacha_key);
          uint32_t x[16], y[16];
          x[0] = 0x61707865u; x[1] = 0x3320646eu; x[2] = 0x79622d32u; x[3] = 0x6b206574u;
#pragma unroll
          for (int k = 0; k < 8; k++) x[4 + k] = kw[k];
          x[12] = 1u; x[13] = fx0; x[14] = n1; x[15] = n2;
          chacha_block(x, y);
          ks[0] = y[0]; ks[1] = y[1]; ks[2] = y[2]; ks[3] = y[3];
        } else {  // E_K(nonce || 00000002)
          const uint32_t j[4] = {fx0, n1, n2, 0x02000000u};
          peek_aes(te, S->rk, rounds, j, ks);
        }
        const uint32_t pt[4] = {c[0] ^ ks[0], c[1] ^ ks[1], c[2] ^ ks[2], c[3] ^ ks[3]};
        cand = ku_candidate(pt, nb);
        end = (uint32_t)rel + len;
      }
    }
    const uint64_t hit = __ballot(cand);
    if (!hit) continue;
    const uint32_t fl = (uint32_t)__builtin_ctzll(hit);  // the first candidate's lane
    if (in && lane > fl) *dp = ones;
    cut = true;
    cut_records = i0 + fl + 1;
    cut_consumed = (uint32_t)__shfl((int)end, (int)fl);
  }
  if (cut && lane == 0) {
    r.records = cut_records;
    r.delivered = cut_records;
    r.consumed = cut_consumed;
    r.alert = 0;  // a header-level alert lies behind the cut: the next call finds it again
    r.alert_record = cut_records;
    r.key_update = TLSGPU_WIRE_KU_HELD;
    results[s] = r;
  }
}

// One lane per stream, after the open and wire_finish_kernel.  Everything read
// here is authenticated plaintext or the engine's own outputs: a stream the
// peek cut is told "KeyUpdate" only if nothing failed up to and including the
// candidate (delivered == records), the candidate's inner type (the unpad pass
// left it in the descriptor) is handshake, its content is 5 bytes and those are
// 18 00 00 01 rr with rr <= 1.  Anything else stays TLSGPU_WIRE_KU_HELD.
__global__ __launch_bounds__(256) void wire_ku_confirm_kernel(
    const tlsgpu_wire_stream* __restrict__ streams, uint32_t n_streams, const uint8_t* wire,
    uint32_t max_records, const tlsgpu_record* __restrict__ recs,
    const int32_t* __restrict__ status, tlsgpu_wire_result* results) {
  const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n_streams) return;
  const tlsgpu_wire_result r = results[s];
  if (r.key_update != TLSGPU_WIRE_KU_HELD) return;
  if (r.delivered != r.records || r.records == 0 || (uint64_t)r.first + r.records > max_records)
    return;
  const size_t slot = (size_t)r.first + r.records - 1;
  const tlsgpu_record d = recs[slot];
  if ((d.len_type >> 24) != kHandshake || status[slot] != (int32_t)kKuMsgLen) return;
  const tlsgpu_wire_stream st = streams[s];
  const uint64_t rel = d.out_off - st.wire_off;
  if (d.out_off < st.wire_off || rel > st.wire_len || st.wire_len - rel < kKuMsgLen) return;
  const auto p = gld<uint8_t>(wire + d.out_off);
  const uint32_t rr = p[4];
  if (p[0] == 0x18 && p[1] == 0 && p[2] == 0 && p[3] == 1 && rr <= 1)
    results[s].key_update = TLSGPU_WIRE_KU_UPDATE + rr;
}

int launch_wire_peek13(const tlsgpu_wire_stream* streams, uint32_t n_streams, const uint8_t* wire,
                       const DevSession* sessions, uint32_t n_sessions, uint32_t max_records,
                       tlsgpu_record* recs, tlsgpu_wire_result* results, hipStream_t s) {
  if (n_streams == 0 || max_records == 0) return 0;
  hipLaunchKernelGGL(wire_peek13_kernel, dim3((n_streams + 3) / 4), dim3(256), 0, s, streams,
                     n_streams, wire, sessions, n_sessions, max_records, recs, results);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_wire_ku_confirm(const tlsgpu_wire_stream* streams, uint32_t n_streams,
                           const uint8_t* wire, uint32_t max_records, const tlsgpu_record* recs,
                           const int32_t* status, tlsgpu_wire_result* results, hipStream_t s) {
  if (n_streams == 0 || max_records == 0) return 0;
  hipLaunchKernelGGL(wire_ku_confirm_kernel, dim3((n_streams + 255) / 256), dim3(256), 0, s,
                     streams, n_streams, wire, max_records, recs, status, results);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace tg
