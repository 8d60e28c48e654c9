// wire_read.hip — tlsgpu_read_wire (include/tlsgpu.h "One-call wire read path";
// DESIGN.md §4.6e): TLS 1.2 streams opened out of place, straight into each
// stream's contiguous application run, so no second pass copies the plaintext.
//
// Under TLS 1.2 a record's plaintext length (fragment - explicit nonce - tag)
// and its content type are in its header, so where its plaintext belongs in
// the run is known before anything is opened:
//   wire_read_plan_kernel    between wire_frame_kernel and the open, one wave
//                            per stream: walks the framed records in order,
//                            gives each placed record its destination in d_app
//                            (the descriptor's out_off) and cuts the stream
//                            before the first record that is not application
//                            data, does not fit the room or leaves the wire;
//   wire_read_finish_kernel  after wire_finish_kernel, one wave per stream: the
//                            read result, from the statuses of the delivered
//                            records.
// The plan reads descriptors, streams and the session's kind and tag length and
// not one byte of d_wire.  Its cut is wire_peek.hip's: descriptors behind it go
// back to all ones, so the open neither reads nor writes what lies there.  The
// type and the length a stop reports come from the unverified header (the type
// is part of the AAD: whoever opens the record next authenticates it), so a
// forged header can only shorten the batch.  The framing and cipher kernels are
// not touched.
#include "tlsgpu_internal.h"

namespace tg {

constexpr uint32_t kReadAppData = 23;

__device__ __forceinline__ uint32_t read_uni(uint32_t v) {
  return __builtin_amdgcn_readfirstlane(v);
}

// inclusive wave scan of a 64-bit value (wire_kernels.hip wave_scan64); all 64 lanes active
__device__ __forceinline__ uint64_t read_scan64(uint64_t v, uint32_t lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t lo = __shfl_up((uint32_t)v, d), hi = __shfl_up((uint32_t)(v >> 32), d);
    if (lane >= (uint32_t)d) v += ((uint64_t)hi << 32) | lo;
  }
  return v;
}

// The records a stream's wire result names, kept inside the descriptor array
// (framing keeps a stream's slots inside max_records; nothing here relies on it).
__device__ __forceinline__ uint32_t slots_inside(uint32_t first, uint32_t n, uint32_t max_records) {
  return min(n, max_records - min(first, max_records));
}

// One wave per stream (four per workgroup, as wire_gather_plan_kernel), 64
// records per step.  The only place the rule is written (include/tlsgpu.h states
// it).  Record i of the stream has p_i = max(0, len_i - eiv - tag) plaintext
// bytes; T is the sum of p over the records placed so far, room = min(app_cap,
// app_bytes - app_off) or 0 past the buffer's end.  In this order:
//   start != 0                          OUT_OF_BOUNDS, the stream is cut to nothing;
//   [in_off, in_off + len_i) leaves     OUT_OF_BOUNDS, cut before i;
//     wire_bytes
//   the header's type is not 23         NOT_APP_DATA, cut before i, stop_type /
//                                       stop_len = the header's type / p_i;
//   T + p_i > room                      FULL, cut before i, stop_type 23, stop_len p_i;
//   otherwise                           placed: out_off = app_off + T, T += p_i.
// Each lane computes its record's p, a 64-bit inclusive scan carries T across
// the steps, one ballot finds the first lane that cuts.  A cut at i: records =
// delivered = alert_record = i, consumed ends with record i - 1, a header-level
// alert from behind the cut is dropped, the descriptors from i on go back to all
// ones.  The read result written here is provisional (stop, stop_type,
// stop_len): wire_read_finish_kernel completes it.
__global__ __launch_bounds__(256) void wire_read_plan_kernel(
    const tlsgpu_wire_stream* __restrict__ streams, uint32_t n_streams,
    const DevSession* __restrict__ sessions, uint32_t n_sessions, uint32_t max_records,
    uint64_t wire_bytes, const tlsgpu_read_stream* __restrict__ reads, uint64_t app_bytes,
    tlsgpu_record* __restrict__ recs, tlsgpu_wire_result* __restrict__ results,
    tlsgpu_read_result* __restrict__ out) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t s = blockIdx.x * 4 + read_uni(threadIdx.x >> 6);
  if (s >= n_streams) return;
  const tlsgpu_wire_stream st = streams[s];
  const tlsgpu_read_stream rd = reads[s];
  tlsgpu_wire_result wr = results[s];
  const uint32_t first = read_uni(wr.first);
  const uint32_t nrec = slots_inside(first, read_uni(wr.records), max_records);
  // explicit nonce + tag of the session's AEAD (GCM 8 + tag, ChaCha 0 + tag; truncated
  // tags count); an unknown session: 0, its records are placed whole and the open
  // leaves them PUBLIC_INVALID
  uint32_t over = 0;
  const uint32_t sid = read_uni(st.session);
  if (sid < n_sessions) {
    const uint32_t kind = read_uni(sessions[sid].kind);
    over = (kind == TLSGPU_AES_128_GCM || kind == TLSGPU_AES_256_GCM ? 8u : 0u) +
           read_uni(sessions[sid].tag_len);
  }
  uint32_t room = rd.app_cap;  // min(app_cap, app_bytes - app_off), 0 past the buffer's end
  if (rd.app_off > app_bytes) room = 0;
  else if (app_bytes - rd.app_off < room) room = (uint32_t)(app_bytes - rd.app_off);
  // (a run that starts past the buffer's end has no room, so only empty records are
  // placed there: their out_off is the buffer's end, which the open's bounds accept)
  const uint64_t app_base = min((uint64_t)rd.app_off, app_bytes);
  tlsgpu_record ones;
  ones.in_off = ones.out_off = ones.seq = ~0ull;
  ones.session = ones.len_type = ~0u;

  tlsgpu_read_result r = {};
  bool cut = read_uni(rd.start) != 0;  // wave-uniform throughout
  uint32_t cut_records = 0, cut_consumed = 0;
  if (cut) r.stop = TLSGPU_READ_OUT_OF_BOUNDS;
  uint64_t total = 0;     // T: plaintext bytes of the records placed so far (<= room)
  uint32_t prev_end = 0;  // the end of the last record of the steps before, within the stream
  for (uint32_t i0 = 0; i0 < nrec; i0 += 64) {
    const uint32_t nin = min(64u, nrec - i0);  // records of this step
    const bool in = lane < nin;
    tlsgpu_record* dp = recs + (size_t)first + i0 + lane;
    if (cut) {  // behind the cut
      if (in) *dp = ones;
      continue;
    }
    uint32_t lt = 0;
    uint64_t in_off = 0;
    if (in) {
      lt = dp->len_type;
      in_off = dp->in_off;
    }
    const uint32_t len = lt & 0xFFFFFFu, type = lt >> 24;
    const uint32_t p = len > over ? len - over : 0u;
    const bool frag_ok = in_off <= wire_bytes && len <= wire_bytes - in_off;
    const bool app = type == kReadAppData;
    const uint32_t add = in && frag_ok && app ? p : 0u;
    const uint64_t incl = read_scan64(add, lane);
    const uint64_t before = total + incl - add;  // T in front of this lane's record
    const int32_t code = !in             ? TLSGPU_READ_END
                         : !frag_ok      ? TLSGPU_READ_OUT_OF_BOUNDS
                         : !app          ? TLSGPU_READ_NOT_APP_DATA
                         : before + p > room ? TLSGPU_READ_FULL
                                         : TLSGPU_READ_END;
    const uint32_t end = (uint32_t)(in_off - st.wire_off) + len;  // this record's, within the stream
    const uint64_t stops = __ballot(code != TLSGPU_READ_END);
    const uint32_t take = stops ? (uint32_t)__builtin_ctzll(stops) : nin;  // records placed
    if (lane < take) dp->out_off = app_base + before;
    if (take) {
      const uint32_t lo = __shfl((uint32_t)incl, (int)take - 1);
      const uint32_t hi = __shfl((uint32_t)(incl >> 32), (int)take - 1);
      total += ((uint64_t)hi << 32) | lo;
    }
    const uint32_t last_end = take ? (uint32_t)__shfl((int)end, (int)take - 1) : prev_end;
    if (stops) {
      const int fl = (int)take;  // the first lane that cuts
      if (in && lane >= take) *dp = ones;
      cut = true;
      cut_records = i0 + take;
      cut_consumed = last_end;
      r.stop = __shfl(code, fl);
      const uint32_t stype = __shfl(type, fl), slen = __shfl(p, fl);
      if (r.stop != TLSGPU_READ_OUT_OF_BOUNDS) {
        r.stop_type = stype;
        r.stop_len = slen;
      }
    }
    prev_end = last_end;
  }
  if (lane == 0) {
    if (cut) {
      wr.records = cut_records;
      wr.delivered = cut_records;
      wr.consumed = cut_consumed;
      wr.alert = 0;  // a header-level alert lies behind the cut: the next call finds it again
      wr.alert_record = cut_records;
      results[s] = wr;  // (`first` stays framing's, also for a stream cut to nothing)
    }
    out[s] = r;
  }
}

// One wave per stream, after the open and wire_finish_kernel: records = next =
// delivered, app_len = the sum of the delivered records' statuses (a wave sum),
// consumed runs through record delivered - 1.  A stream that an AEAD failure or
// an over-long record ended before its last kept record stops with
// TLSGPU_READ_END (the wire result's alert says why); otherwise the plan's stop
// stands.
__global__ __launch_bounds__(256) void wire_read_finish_kernel(
    const tlsgpu_wire_stream* __restrict__ streams, const tlsgpu_wire_result* __restrict__ results,
    uint32_t n_streams, const tlsgpu_record* __restrict__ recs, const int32_t* __restrict__ status,
    uint32_t max_records, tlsgpu_read_result* __restrict__ out) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t s = blockIdx.x * 4 + read_uni(threadIdx.x >> 6);
  if (s >= n_streams) return;
  const tlsgpu_wire_result wr = results[s];
  const uint32_t first = read_uni(wr.first);
  const uint32_t kept = slots_inside(first, read_uni(wr.records), max_records);
  const uint32_t D = min(read_uni(wr.delivered), kept);
  uint32_t sum = 0;  // (<= the room, which is 32 bits)
  for (uint32_t i = lane; i < D; i += 64) sum += (uint32_t)status[(size_t)first + i];
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) sum += __shfl_xor(sum, d);
  if (lane == 0) {
    tlsgpu_read_result r = out[s];  // the plan's stop, stop_type, stop_len
    r.app_len = sum;
    r.records = r.next = D;
    r.consumed = 0;
    if (D) {
      const tlsgpu_record last = recs[(size_t)first + D - 1];
      r.consumed = (uint32_t)(last.in_off + (last.len_type & 0xFFFFFFu) - streams[s].wire_off);
    }
    if (D < kept) {
      r.stop = TLSGPU_READ_END;
      r.stop_type = r.stop_len = 0;
    }
    r.reserved = 0;
    out[s] = r;
  }
}

int launch_wire_read_plan(const tlsgpu_wire_stream* streams, uint32_t n_streams,
                          const DevSession* sessions, uint32_t n_sessions, uint32_t max_records,
                          uint64_t wire_bytes, const tlsgpu_read_stream* reads, uint64_t app_bytes,
                          tlsgpu_record* recs, tlsgpu_wire_result* results, tlsgpu_read_result* out,
                          hipStream_t s) {
  if (n_streams == 0) return 0;
  hipLaunchKernelGGL(wire_read_plan_kernel, dim3((n_streams + 3) / 4), dim3(256), 0, s, streams,
                     n_streams, sessions, n_sessions, max_records, wire_bytes, reads, app_bytes, recs,
                     results, out);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_wire_read_finish(const tlsgpu_wire_stream* streams, const tlsgpu_wire_result* results,
                            uint32_t n_streams, const tlsgpu_record* recs, const int32_t* status,
                            uint32_t max_records, tlsgpu_read_result* out, hipStream_t s) {
  if (n_streams == 0) return 0;
  hipLaunchKernelGGL(wire_read_finish_kernel, dim3((n_streams + 3) / 4), dim3(256), 0, s, streams,
                     results, n_streams, recs, status, max_records, out);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace tg
