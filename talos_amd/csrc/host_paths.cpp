// host_paths.cpp — the batch ABI's paths around run_batch for data that starts
// or ends on the host or on the wire: the host-resident pipeline
// (tlsgpu_open_host / tlsgpu_seal_host), session owners and host delivery with
// the TaLoS plaintext hooks, wire open, gather, read and seal, and the synthetic fills.
#include "host_internal.h"

using namespace tg;

// grow-only device buffer
static bool grow(void** p, size_t* cap, size_t want) {
  if (*cap >= want) return true;
  if (*p) (void)hipFree(*p);
  *p = nullptr;
  *cap = 0;
  if (hipMalloc(p, want ? want : 1) != hipSuccess) return false;
  *cap = want;
  return true;
}

extern "C" int tlsgpu_host_pipeline(tlsgpu_engine* e, unsigned streams, size_t chunk_bytes) {
  if (!e || streams > 8) return fail(TLSGPU_EINVAL, "bad arguments");
  std::lock_guard<std::mutex> lk(e->host.mu);
  if (streams) e->host.nstreams = streams;
  if (chunk_bytes) e->host.chunk_bytes = chunk_bytes;
  return TLSGPU_OK;
}

// Test hook (TLSGPU_TEST_HOST_FAIL_CHUNK=k): the host pipeline fails right
// after queueing chunk k's copy in, with earlier chunks still in flight.
static const long g_host_fail_chunk = [] {
  const char* v = getenv("TLSGPU_TEST_HOST_FAIL_CHUNK");
  return v && *v ? strtol(v, nullptr, 10) : -1L;
}();

// The host-resident pipeline for both directions (tlsgpu_open_host /
// tlsgpu_seal_host).  Open: in = record fragments, out = plaintext; seal: in =
// plaintext, out = fragments.  The TaLoS plaintext hooks run on the host
// plaintext: after the batch for reads, before its first copy for writes.
// The batch-shape hints of a host-resident slice (tlsgpu_sessions_hint): no
// record short enough for a pack (GCM n <= 992 B, the open length with the
// explicit nonce and the longest tag), and session runs long enough for the
// run-at-a-time queue kernel (pws_selected: runs * kPwsRun <= records).  A
// TLS 1.3 table: 62 blocks of inner plaintext, i.e. 992 B + the tag on open (no
// explicit nonce) and on seal a padded inner plaintext (tls13_inner_len under
// the session's padding mask) of at most 992 B: 991 B of content without a
// padding block, none with a block of 1024 or more.
static unsigned host_hints(const tlsgpu_sessions* t, const tlsgpu_record* r, uint32_t n, bool seal,
                           bool t13) {
  const uint32_t short_max = t13 ? (seal ? 992u : 992u + 16u) : (seal ? 992u : 992u + 8u + 16u);
  bool shorts = false;
  uint32_t runs = 0;
  for (uint32_t i = 0; i < n; i++) {
    uint32_t len = r[i].len_type & 0xFFFFFFu;
    if (t13 && seal)
      len = tls13_inner_len(len, r[i].session < t->capacity ? t->pad_masks[r[i].session] : 0u);
    shorts |= len <= short_max;
    runs += (i == 0 || r[i].session != r[i - 1].session) ? 1u : 0u;
  }
  return (shorts ? 0u : TLSGPU_HINT_NO_SHORT_RECORDS) |
         ((uint64_t)runs * kPwsRun <= n ? TLSGPU_HINT_SESSION_RUNS : 0u);
}

static int host_batch(tlsgpu_sessions* t, bool seal, const tlsgpu_record* h_recs, uint32_t n,
                      const uint8_t* h_in, size_t in_bytes, uint8_t* h_out, size_t out_bytes,
                      int32_t* h_status) {
  if (!t || (n && (!h_recs || !h_in || !h_out || !h_status)))
    return fail(TLSGPU_EINVAL, "bad arguments");
  if (n == 0) return TLSGPU_OK;
  tlsgpu_engine* e = t->eng;
  HostPipe& hp = e->host;
  std::lock_guard<std::mutex> lk(hp.mu);
  HIPCHK(hipSetDevice(e->device));
  // TaLoS tls_processing_ssl_write (do_ssl3_write, s3_pkt.c.patch:19-33): on
  // each record's host plaintext before it goes to the device, in record
  // order; the module may rewrite the bytes and shorten the record (then a
  // private copy of the descriptors carries the new length)
  std::vector<tlsgpu_record> hooked;
  if (seal && talos_write_hooked()) {
    for (uint32_t i = 0; i < n; i++) {
      const uint32_t len = h_recs[i].len_type & 0xFFFFFFu;
      if (h_recs[i].session >= t->capacity || h_recs[i].in_off > in_bytes ||
          len > in_bytes - h_recs[i].in_off)
        continue;  // the bounds pass rejects it
      uint32_t hl = len;
      talos_write(t->owners[h_recs[i].session], const_cast<uint8_t*>(h_in) + h_recs[i].in_off,
                  &hl);
      if (hl < len) {
        if (hooked.empty()) hooked.assign(h_recs, h_recs + n);
        hooked[i].len_type = (hooked[i].len_type & 0xFF000000u) | hl;
      }
    }
    if (!hooked.empty()) h_recs = hooked.data();
  }
  const bool in_place = h_out == h_in;
  if (in_place) out_bytes = in_bytes;
  while (hp.streams.size() < 2 + hp.nstreams) {
    hipStream_t hs;
    HIPCHK(hipStreamCreateWithFlags(&hs, hipStreamNonBlocking));
    hp.streams.push_back(hs);
  }
  if (!grow((void**)&hp.d_in, &hp.cap_in, in_bytes) ||
      (!in_place && !grow((void**)&hp.d_out, &hp.cap_out, out_bytes)) ||
      !grow((void**)&hp.d_status, &hp.cap_status, sizeof(int32_t) * (size_t)n) ||
      !grow((void**)&hp.d_recs, &hp.cap_recs, sizeof(tlsgpu_record) * (size_t)n))
    return fail(TLSGPU_ENOMEM, "host pipeline buffers (%zu + %zu bytes)", in_bytes, out_bytes);
  uint8_t* d_in = hp.d_in;
  uint8_t* d_out = in_place ? hp.d_in : hp.d_out;
  // per-record spans (clamped to the buffers; the bounds pre-pass rejects the rest)
  auto span_in = [&](const tlsgpu_record& r, uint64_t* lo, uint64_t* hi) {
    *lo = std::min<uint64_t>(r.in_off, in_bytes);
    *hi = std::min<uint64_t>(r.in_off + (r.len_type & 0xFFFFFFu), in_bytes);
  };
  // the output span exactly (open: the plaintext, explicit nonce and tag
  // excluded — for TLS 1.3 the whole inner plaintext, padding included; seal:
  // the fragment, for TLS 1.3 the padded inner plaintext + tag): a neighbouring
  // chunk's D2H on another stream may own the next byte
  const bool t13 = t->generation == 13;
  auto span_out = [&](const tlsgpu_record& r, uint64_t* lo, uint64_t* hi) {
    const uint64_t len = r.len_type & 0xFFFFFFu;
    uint64_t over = 0;
    if (r.session < t->capacity) {
      const int k = t->kinds[r.session];
      const bool gcm = k == TLSGPU_AES_128_GCM || k == TLSGPU_AES_256_GCM;
      const bool s13 = tls13_session((uint32_t)k, t13 ? 0u : 1u);  // GCM or ChaCha
      // a TLS 1.3 seal: + the type byte and the session's padding
      const uint64_t grow = s13 && seal ? tls13_inner_len((uint32_t)len, t->pad_masks[r.session]) - len : 0;
      over = (gcm && !s13 ? 8 : 0) + grow + t->tag_lens[r.session];
    }
    *lo = std::min<uint64_t>(r.out_off, out_bytes);
    *hi = std::min<uint64_t>(r.out_off + (seal ? len + over : (len > over ? len - over : 0)),
                             out_bytes);
  };
  // chunks of ~chunk_bytes input when the layout ascends, else one chunk
  bool ascending = true;
  for (uint32_t i = 1; i < n && ascending; i++)
    ascending = h_recs[i].in_off >= h_recs[i - 1].in_off &&
                h_recs[i].out_off >= h_recs[i - 1].out_off;
  // chunk sizes ramp up from 1 MiB and back down at the end, so the pipeline
  // fills and drains on small transfers
  std::vector<uint32_t> cuts{0};
  if (ascending) {
    uint64_t total = 0;
    for (uint32_t i = 0; i < n; i++) total += h_recs[i].len_type & 0xFFFFFFu;
    uint64_t acc = 0, done = 0, target = std::min<uint64_t>(hp.chunk_bytes, 1u << 20);
    for (uint32_t i = 0; i < n; i++) {
      const uint64_t l = h_recs[i].len_type & 0xFFFFFFu;
      acc += l;
      done += l;
      if (acc >= target && i + 1 < n) {
        cuts.push_back(i + 1);
        acc = 0;
        const uint64_t left = total - done;
        target = std::min<uint64_t>({(uint64_t)hp.chunk_bytes, 2 * target,
                                     std::max<uint64_t>(left / 2, 1u << 20)});
      }
    }
  }
  cuts.push_back(n);
  const size_t nchunks = cuts.size() - 1;
  while (hp.events.size() < 2 * nchunks) {
    hipEvent_t ev;
    HIPCHK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    hp.events.push_back(ev);
  }
  hipStream_t s_in = hp.streams[0], s_out = hp.streams[1];
  const size_t ncomp = hp.streams.size() - 2;
  // Everything below is asynchronous on the pipeline streams; whatever fails,
  // the streams are drained before returning, so no copy into or out of the
  // caller's buffers is still running once the call has returned.
  auto issue = [&]() -> int {
    // all descriptors in one copy ahead of the first chunk, all statuses in one after the last
    HIPCHK(hipMemcpyAsync(hp.d_recs, h_recs, sizeof(tlsgpu_record) * (size_t)n,
                          hipMemcpyHostToDevice, s_in));
    for (size_t k = 0; k < nchunks; k++) {
      const uint32_t a = cuts[k], b = cuts[k + 1];
      hipStream_t hs = hp.streams[2 + k % ncomp];
      hipEvent_t ev_in = hp.events[2 * k], ev_done = hp.events[2 * k + 1];
      uint64_t ilo = UINT64_MAX, ihi = 0, olo = UINT64_MAX, ohi = 0;
      for (uint32_t i = a; i < b; i++) {
        uint64_t l, h;
        span_in(h_recs[i], &l, &h);
        ilo = std::min(ilo, l);
        ihi = std::max(ihi, h);
        span_out(h_recs[i], &l, &h);
        olo = std::min(olo, l);
        ohi = std::max(ohi, h);
      }
      if (!ascending) {  // one chunk: the whole buffers
        ilo = 0; ihi = in_bytes; olo = 0; ohi = out_bytes;
      }
      // copy in (DMA engine 1) -> kernels (compute stream) -> copy out (DMA engine 2)
      if (ihi > ilo)
        HIPCHK(hipMemcpyAsync(d_in + ilo, h_in + ilo, ihi - ilo, hipMemcpyHostToDevice, s_in));
      if ((long)k == g_host_fail_chunk)  // test hook: a failure with earlier chunks in flight
        return fail(TLSGPU_EHIP, "injected host pipeline failure at chunk %zu", k);
      HIPCHK(hipEventRecord(ev_in, s_in));
      HIPCHK(hipStreamWaitEvent(hs, ev_in, 0));
      // out of place, the HBM mirror is reused across calls: clear the range
      // copied back, so bytes between the records' output spans come back as
      // zeros, never as an earlier call's plaintext (in place, the whole range
      // was just copied in from h_in)
      if (!in_place && ohi > olo) HIPCHK(hipMemsetAsync(d_out + olo, 0, ohi - olo, hs));
      const Bounds bd = {in_bytes, out_bytes};
      const int rc = run_batch(t, hp.d_recs + a, b - a, d_in, d_out, hp.d_status + a, hs, seal,
                               false, &bd, ~0u, host_hints(t, h_recs + a, b - a, seal, t13));
      if (rc != TLSGPU_OK) return rc;
      HIPCHK(hipEventRecord(ev_done, hs));
      HIPCHK(hipStreamWaitEvent(s_out, ev_done, 0));
      if (ohi > olo)
        HIPCHK(hipMemcpyAsync(h_out + olo, d_out + olo, ohi - olo, hipMemcpyDeviceToHost, s_out));
    }
    HIPCHK(hipMemcpyAsync(h_status, hp.d_status, sizeof(int32_t) * (size_t)n,
                          hipMemcpyDeviceToHost, s_out));
    return TLSGPU_OK;
  };
  int rc = issue();
  for (hipStream_t hs : hp.streams) {  // drain on success and on every failure
    const hipError_t e = hipStreamSynchronize(hs);
    if (e != hipSuccess && rc == TLSGPU_OK)
      rc = fail(TLSGPU_EHIP, "host pipeline sync: %s", hipGetErrorString(e));
  }
  if (rc != TLSGPU_OK) return rc;
  // TaLoS tls_processing_ssl_read (ssl3_read_bytes, s3_pkt.c.patch:39-52): on
  // each delivered record's plaintext in h_out, in record order; a module that
  // shortens it shortens what is delivered (h_status)
  if (!seal && talos_read_hooked()) {
    for (uint32_t i = 0; i < n; i++) {
      if (h_status[i] < 0) continue;
      uint32_t hl = (uint32_t)h_status[i];
      talos_read(t->owners[h_recs[i].session], h_out + h_recs[i].out_off, &hl);
      if (hl < (uint32_t)h_status[i]) h_status[i] = (int32_t)hl;
    }
  }
  return TLSGPU_OK;
}

extern "C" int tlsgpu_open_host(tlsgpu_sessions* t, const tlsgpu_record* h_recs, uint32_t n,
                                const uint8_t* h_in, size_t in_bytes, uint8_t* h_out,
                                size_t out_bytes, int32_t* h_status) {
  return host_batch(t, false, h_recs, n, h_in, in_bytes, h_out, out_bytes, h_status);
}

extern "C" int tlsgpu_seal_host(tlsgpu_sessions* t, const tlsgpu_record* h_recs, uint32_t n,
                                const uint8_t* h_in, size_t in_bytes, uint8_t* h_out,
                                size_t out_bytes, int32_t* h_status) {
  if (h_out == h_in && n) return fail(TLSGPU_EINVAL, "tlsgpu_seal_host cannot run in place");
  return host_batch(t, true, h_recs, n, h_in, in_bytes, h_out, out_bytes, h_status);
}

extern "C" int tlsgpu_sessions_set_owner(tlsgpu_sessions* t, uint32_t first, uint32_t n,
                                         const void* const* owners) {
  if (!t || (n && !owners)) return fail(TLSGPU_EINVAL, "bad arguments");
  if ((uint64_t)first + n > t->capacity)
    return fail(TLSGPU_ERANGE, "sessions [%u, %u) exceed capacity %u", first, first + n,
                t->capacity);
  for (uint32_t i = 0; i < n; i++) t->owners[first + i] = owners[i];
  return TLSGPU_OK;
}

// Host delivery of device-resident opens (tlsgpu_open_batch / tlsgpu_open_wire):
// descriptors and statuses back to the host, the delivered records' output
// range to h_out (same offsets as d_out), then the TaLoS read hook on each
// delivered record in record order.
extern "C" int tlsgpu_deliver_host(tlsgpu_sessions* t, const tlsgpu_record* d_recs,
                                   const int32_t* d_status, uint32_t n, const uint8_t* d_out,
                                   size_t out_bytes, uint8_t* h_out, int32_t* h_status,
                                   void* stream) {
  if (!t || (n && (!d_recs || !d_status || !d_out || !h_out || !h_status)))
    return fail(TLSGPU_EINVAL, "bad arguments");
  if (n == 0) return TLSGPU_OK;
  HIPCHK(hipSetDevice(t->eng->device));
  hipStream_t s = stream ? (hipStream_t)stream : t->eng->stream;
  std::vector<tlsgpu_record> recs(n);
  HIPCHK(hipMemcpyAsync(recs.data(), d_recs, sizeof(tlsgpu_record) * (size_t)n,
                        hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(h_status, d_status, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost,
                        s));
  HIPCHK(hipStreamSynchronize(s));
  uint64_t lo = UINT64_MAX, hi = 0;
  for (uint32_t i = 0; i < n; i++) {
    if (h_status[i] < 0) continue;
    const uint64_t o = recs[i].out_off, e = o + (uint64_t)h_status[i];
    if (o > out_bytes || e > out_bytes || recs[i].session >= t->capacity)
      return fail(TLSGPU_ERANGE, "record %u output [%llu, %llu) outside %zu bytes", i,
                  (unsigned long long)o, (unsigned long long)e, out_bytes);
    lo = std::min(lo, o);
    hi = std::max(hi, e);
  }
  if (hi > lo) {
    HIPCHK(hipMemcpyAsync(h_out + lo, d_out + lo, hi - lo, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
  }
  if (talos_read_hooked()) {
    for (uint32_t i = 0; i < n; i++) {
      if (h_status[i] < 0) continue;
      uint32_t hl = (uint32_t)h_status[i];
      talos_read(t->owners[recs[i].session], h_out + recs[i].out_off, &hl);
      if (hl < (uint32_t)h_status[i]) h_status[i] = (int32_t)hl;
    }
  }
  return TLSGPU_OK;
}

// The write side of tlsgpu_seal_wire for callers whose application data starts
// in host memory: the TaLoS write hook on every fragment do_ssl3_write would
// make of each stream (max_send_fragment split, s3_pkt.c:531-536), in place,
// before the caller copies h_data to the device.  Lengths stay.
extern "C" int tlsgpu_hook_write_streams(tlsgpu_sessions* t, const tlsgpu_write_stream* h_streams,
                                         uint32_t n_streams, uint8_t* h_data, size_t data_bytes) {
  if (!t || (n_streams && (!h_streams || !h_data))) return fail(TLSGPU_EINVAL, "bad arguments");
  if (!talos_write_hooked()) return TLSGPU_OK;
  for (uint32_t i = 0; i < n_streams; i++) {
    const tlsgpu_write_stream& st = h_streams[i];
    if (st.session >= t->capacity || st.data_off > data_bytes ||
        st.data_len > data_bytes - st.data_off)
      continue;
    const uint32_t frag = st.max_fragment == 0 || st.max_fragment > 16384 ? 16384 : st.max_fragment;
    for (uint64_t off = 0; off < st.data_len; off += frag) {
      uint32_t hl = (uint32_t)std::min<uint64_t>(frag, st.data_len - off);
      talos_write(t->owners[st.session], h_data + st.data_off + off, &hl);
    }
  }
  return TLSGPU_OK;
}

// The KeyUpdate cut of tlsgpu_open_wire (include/tlsgpu.h): a
// per-table switch, and two launchers that are weak references here for the
// reason the gather's are (below): a library linked without wire_peek.hip's
// kernels fails loudly, and only when the switch is on.
namespace tg {
__attribute__((weak)) int launch_wire_peek13(
    const tlsgpu_wire_stream* streams, uint32_t n_streams, const uint8_t* wire,
    const DevSession* sessions, uint32_t n_sessions, uint32_t max_records, tlsgpu_record* recs,
    tlsgpu_wire_result* results, hipStream_t s);
__attribute__((weak)) int launch_wire_ku_confirm(
    const tlsgpu_wire_stream* streams, uint32_t n_streams, const uint8_t* wire,
    uint32_t max_records, const tlsgpu_record* recs, const int32_t* status,
    tlsgpu_wire_result* results, hipStream_t s);
}  // namespace tg

extern "C" int tlsgpu_sessions_wire_key_update(tlsgpu_sessions* t, int on) {
  if (!t) return fail(TLSGPU_EINVAL, "bad arguments");
  t->wire_key_update.store(on != 0, std::memory_order_relaxed);
  return TLSGPU_OK;
}

extern "C" int tlsgpu_open_wire(tlsgpu_sessions* t, const tlsgpu_wire_stream* d_streams,
                                uint32_t n_streams, uint8_t* d_wire, uint32_t max_records,
                                tlsgpu_record* d_recs, int32_t* d_status,
                                tlsgpu_wire_result* d_results, uint32_t* d_total, void* stream) {
  if (!t || !d_total || (n_streams && (!d_streams || !d_wire || !d_results)) ||
      (max_records && (!d_recs || !d_status)))
    return fail(TLSGPU_EINVAL, "bad arguments");
  const bool ku = t->wire_key_update.load(std::memory_order_relaxed);
  if (ku && (!launch_wire_peek13 || !launch_wire_ku_confirm))
    return fail(TLSGPU_EHIP, "the KeyUpdate kernels are not linked into this library");
  // the cut: TLS 1.3 streams only, and only where there are descriptors to cut
  const bool cut = ku && t->generation == 13 && max_records;
  HIPCHK(hipSetDevice(t->eng->device));
  hipStream_t s = stream ? (hipStream_t)stream : t->eng->stream;
  HIPCHK(hipMemsetAsync(d_total, 0, sizeof(uint32_t), s));
  if (n_streams == 0) return TLSGPU_OK;
  // unused record slots name no session (0xFFFFFFFF): the open kernels skip them
  if (max_records) HIPCHK(hipMemsetAsync(d_recs, 0xFF, sizeof(tlsgpu_record) * (size_t)max_records, s));
  // (streams of TLS 1.3 sessions: the framing kernel reads the generation from
  // the session and applies RFC 8446 5.2's header rules)
  if (launch_wire_frame(d_streams, n_streams, d_wire, t->d_sess, t->capacity, max_records, d_recs,
                        d_results, d_total, s))
    return fail(TLSGPU_EHIP, "wire frame launch: %s", hipGetErrorString(hipGetLastError()));
  // before anything is opened: what lies behind a KeyUpdate stays ciphertext
  if (cut && launch_wire_peek13(d_streams, n_streams, d_wire, t->d_sess, t->capacity, max_records,
                                d_recs, d_results, s))
    return fail(TLSGPU_EHIP, "wire peek launch: %s", hipGetErrorString(hipGetLastError()));
  if (max_records) {
    // TLS 1.3: the open's unpad pass leaves every record's inner content type
    // in its descriptor's type bits, as a TLS 1.2 record's header type is
    int rc = run_batch(t, d_recs, max_records, d_wire, d_wire, d_status, s, false, false, nullptr,
                       ~0u, ~0u, d_recs);
    if (rc != TLSGPU_OK) return rc;
  }
  if (launch_wire_finish(n_streams, d_results, d_status, s))
    return fail(TLSGPU_EHIP, "wire finish launch: %s", hipGetErrorString(hipGetLastError()));
  // the verdict, from the verified record alone
  if (cut && launch_wire_ku_confirm(d_streams, n_streams, d_wire, max_records, d_recs, d_status,
                                    d_results, s))
    return fail(TLSGPU_EHIP, "wire KeyUpdate confirm launch: %s",
                hipGetErrorString(hipGetLastError()));
  return TLSGPU_OK;
}

// The copy kernel's piece size from what the host knows of the batch, the wire
// bytes per record slot: long records are split over 8 waves each, short ones
// get one wave (kGatherSplitBytes).  TLSGPU_GATHER_PIECE=2048 /
// 4096 / 16384 forces one (experiments only).
static const uint32_t g_gather_piece = (uint32_t)env_uint("TLSGPU_GATHER_PIECE", 0, 10);
static uint32_t gather_piece(size_t wire_bytes, uint32_t max_records) {
  if (g_gather_piece) return g_gather_piece;
  return max_records && wire_bytes / max_records > kGatherSplitBytes ? kGatherPiece : kGatherWhole;
}

// The two launchers are weak references in this unit: the kernels' object
// defines them in libtlsgpu.so, but a link of the host objects alone against a
// launcher list written before this call existed (the CPU tests' recording HIP
// stub) must still resolve.  There the call fails loudly, before any HIP call.
namespace tg {
__attribute__((weak)) int launch_wire_gather_plan(
    const tlsgpu_wire_stream* streams, const tlsgpu_wire_result* results, uint32_t n_streams,
    const tlsgpu_record* recs, const int32_t* status, uint32_t max_records, uint64_t wire_bytes,
    const tlsgpu_read_stream* reads, uint64_t app_bytes, uint64_t* dst, tlsgpu_read_result* out,
    hipStream_t s);
__attribute__((weak)) int launch_wire_gather_copy(
    const tlsgpu_record* recs, const int32_t* status, uint32_t max_records, const uint8_t* wire,
    uint64_t wire_bytes, const uint64_t* dst, uint8_t* app, uint64_t app_bytes, uint32_t piece,
    hipStream_t s);
}  // namespace tg

extern "C" int tlsgpu_gather_wire(tlsgpu_sessions* t, const tlsgpu_wire_stream* d_streams,
                                  const tlsgpu_wire_result* d_results, uint32_t n_streams,
                                  const tlsgpu_record* d_recs, const int32_t* d_status,
                                  uint32_t max_records, const uint8_t* d_wire, size_t wire_bytes,
                                  const tlsgpu_read_stream* d_reads, uint8_t* d_app,
                                  size_t app_bytes, tlsgpu_read_result* d_read_results,
                                  void* stream) {
  if (!t || (n_streams && (!d_streams || !d_results || !d_wire || !d_reads || !d_app ||
                           !d_read_results)) ||
      (max_records && (!d_recs || !d_status)))
    return fail(TLSGPU_EINVAL, "bad arguments");
  // the copy reads d_wire while it writes d_app: the two may not share a byte
  const uintptr_t w0 = (uintptr_t)d_wire, a0 = (uintptr_t)d_app;
  if (d_wire && d_app && a0 < w0 + wire_bytes && w0 < a0 + app_bytes)
    return fail(TLSGPU_EINVAL, "d_app overlaps d_wire");
  if (n_streams == 0) return TLSGPU_OK;
  if (!launch_wire_gather_plan || !launch_wire_gather_copy)
    return fail(TLSGPU_EHIP, "the gather kernels are not linked into this library");
  HIPCHK(hipSetDevice(t->eng->device));
  hipStream_t s = stream ? (hipStream_t)stream : t->eng->stream;
  // one destination offset per record slot, "no copy" until the plan says otherwise
  uint64_t* dst = (uint64_t*)pre_scratch(t->eng, s, sizeof(uint64_t) * (size_t)max_records);
  if (!dst) return fail(TLSGPU_ENOMEM, "gather scratch (%u records)", max_records);
  if (max_records) HIPCHK(hipMemsetAsync(dst, 0xFF, sizeof(uint64_t) * (size_t)max_records, s));
  if (launch_wire_gather_plan(d_streams, d_results, n_streams, d_recs, d_status, max_records,
                              wire_bytes, d_reads, app_bytes, dst, d_read_results, s))
    return fail(TLSGPU_EHIP, "wire gather plan launch: %s", hipGetErrorString(hipGetLastError()));
  if (launch_wire_gather_copy(d_recs, d_status, max_records, d_wire, wire_bytes, dst, d_app,
                              app_bytes, gather_piece(wire_bytes, max_records), s))
    return fail(TLSGPU_EHIP, "wire gather copy launch: %s", hipGetErrorString(hipGetLastError()));
  return TLSGPU_OK;
}

// tlsgpu_read_wire (include/tlsgpu.h "One-call wire read path"; DESIGN.md
// §4.6e): tlsgpu_open_wire's framing, a plan that gives every record its place in
// its stream's application run, the open out of place from d_wire into d_app, and
// the two finishes.  The destinations travel in the descriptors: no scratch of
// this call's own lives across run_batch.  The plan's and the read finish's
// launchers are weak references for the reason the gather's are (above).
namespace tg {
__attribute__((weak)) int launch_wire_read_plan(
    const tlsgpu_wire_stream* streams, uint32_t n_streams, const DevSession* sessions,
    uint32_t n_sessions, uint32_t max_records, uint64_t wire_bytes,
    const tlsgpu_read_stream* reads, uint64_t app_bytes, tlsgpu_record* recs,
    tlsgpu_wire_result* results, tlsgpu_read_result* out, hipStream_t s);
__attribute__((weak)) int launch_wire_read_finish(
    const tlsgpu_wire_stream* streams, const tlsgpu_wire_result* results, uint32_t n_streams,
    const tlsgpu_record* recs, const int32_t* status, uint32_t max_records,
    tlsgpu_read_result* out, hipStream_t s);
}  // namespace tg

extern "C" int tlsgpu_read_wire(tlsgpu_sessions* t, const tlsgpu_wire_stream* d_streams,
                                uint32_t n_streams, const uint8_t* d_wire, size_t wire_bytes,
                                uint32_t max_records, tlsgpu_record* d_recs, int32_t* d_status,
                                tlsgpu_wire_result* d_results, uint32_t* d_total,
                                const tlsgpu_read_stream* d_reads, uint8_t* d_app,
                                size_t app_bytes, tlsgpu_read_result* d_read_results,
                                void* stream) {
  if (!t || !d_total ||
      (n_streams && (!d_streams || !d_wire || !d_results || !d_reads || !d_app ||
                     !d_read_results)) ||
      (max_records && (!d_recs || !d_status)))
    return fail(TLSGPU_EINVAL, "bad arguments");
  // the open reads d_wire while it writes d_app: the two may not share a byte
  const uintptr_t w0 = (uintptr_t)d_wire, a0 = (uintptr_t)d_app;
  if (d_wire && d_app && a0 < w0 + wire_bytes && w0 < a0 + app_bytes)
    return fail(TLSGPU_EINVAL, "d_app overlaps d_wire");
  // a TLS 1.3 record's content length and inner type exist only after the open
  if (t->generation == 13)
    return fail(TLSGPU_EINVAL, "tlsgpu_read_wire takes TLS 1.2 session tables: read TLS 1.3 "
                               "streams with tlsgpu_open_wire + tlsgpu_gather_wire");
  if (!launch_wire_read_plan || !launch_wire_read_finish)
    return fail(TLSGPU_EHIP, "the read kernels are not linked into this library");
  HIPCHK(hipSetDevice(t->eng->device));
  hipStream_t s = stream ? (hipStream_t)stream : t->eng->stream;
  HIPCHK(hipMemsetAsync(d_total, 0, sizeof(uint32_t), s));
  if (n_streams == 0) return TLSGPU_OK;
  // unused record slots name no session (0xFFFFFFFF): the open kernels skip them
  if (max_records) HIPCHK(hipMemsetAsync(d_recs, 0xFF, sizeof(tlsgpu_record) * (size_t)max_records, s));
  if (launch_wire_frame(d_streams, n_streams, d_wire, t->d_sess, t->capacity, max_records, d_recs,
                        d_results, d_total, s))
    return fail(TLSGPU_EHIP, "wire frame launch: %s", hipGetErrorString(hipGetLastError()));
  // before anything is opened: where each record's plaintext goes, and where each stream ends
  if (launch_wire_read_plan(d_streams, n_streams, t->d_sess, t->capacity, max_records, wire_bytes,
                            d_reads, app_bytes, d_recs, d_results, d_read_results, s))
    return fail(TLSGPU_EHIP, "wire read plan launch: %s", hipGetErrorString(hipGetLastError()));
  if (max_records) {
    const Bounds b = {wire_bytes, app_bytes};
    int rc = run_batch(t, d_recs, max_records, d_wire, d_app, d_status, s, false, false, &b);
    if (rc != TLSGPU_OK) return rc;
  }
  if (launch_wire_finish(n_streams, d_results, d_status, s))
    return fail(TLSGPU_EHIP, "wire finish launch: %s", hipGetErrorString(hipGetLastError()));
  if (launch_wire_read_finish(d_streams, d_results, n_streams, d_recs, d_status, max_records,
                              d_read_results, s))
    return fail(TLSGPU_EHIP, "wire read finish launch: %s", hipGetErrorString(hipGetLastError()));
  return TLSGPU_OK;
}

extern "C" int tlsgpu_seal_wire(tlsgpu_sessions* t, const tlsgpu_write_stream* d_streams,
                                uint32_t n_streams, const uint8_t* d_data, size_t data_bytes,
                                uint8_t* d_wire, size_t wire_bytes, uint32_t max_records,
                                tlsgpu_record* d_recs, int32_t* d_status,
                                tlsgpu_write_result* d_results, uint32_t* d_total, void* stream) {
  if (!t || !d_total || (n_streams && (!d_streams || !d_data || !d_wire || !d_results)) ||
      (max_records && (!d_recs || !d_status)))
    return fail(TLSGPU_EINVAL, "bad arguments");
  HIPCHK(hipSetDevice(t->eng->device));
  hipStream_t s = stream ? (hipStream_t)stream : t->eng->stream;
  HIPCHK(hipMemsetAsync(d_total, 0, sizeof(uint32_t), s));
  if (n_streams == 0) return TLSGPU_OK;
  // unused record slots name no session (0xFFFFFFFF): the seal kernels skip them
  if (max_records) HIPCHK(hipMemsetAsync(d_recs, 0xFF, sizeof(tlsgpu_record) * (size_t)max_records, s));
  if (launch_wire_seal_frame(d_streams, n_streams, t->d_sess, t->capacity, d_wire, wire_bytes,
                             max_records, d_recs, d_results, d_total, s))
    return fail(TLSGPU_EHIP, "wire seal frame launch: %s", hipGetErrorString(hipGetLastError()));
  if (max_records) {
    const Bounds b = {data_bytes, wire_bytes};
    return run_batch(t, d_recs, max_records, d_data, d_wire, d_status, s, true, false, &b);
  }
  return TLSGPU_OK;
}

extern "C" uint64_t tlsgpu_seal_wire_size(int aead, uint32_t data_len, uint32_t max_fragment,
                                          uint32_t tag_len) {
  const uint32_t frag = max_fragment == 0 || max_fragment > 16384 ? 16384 : max_fragment;
  const uint64_t nrec = ((uint64_t)data_len + frag - 1) / frag;
  const uint64_t eiv = aead == TLSGPU_AES_128_GCM || aead == TLSGPU_AES_256_GCM ? 8 : 0;
  // the TLS 1.3 ChaCha kind: header || content || inner type || tag(16), whatever the version
  if (aead == TLSGPU_CHACHA20_POLY1305_TLS13) return data_len + nrec * (5 + 1 + 16);
  return data_len + nrec * (5 + eiv + (tag_len ? tag_len : 16));
}

extern "C" uint64_t tlsgpu_seal_wire_size_v(int aead, uint16_t version, uint32_t data_len,
                                            uint32_t max_fragment, uint32_t tag_len) {
  return tlsgpu_seal_wire_size_p(aead, version, data_len, max_fragment, tag_len, 0);
}

extern "C" uint64_t tlsgpu_seal_wire_size_p(int aead, uint16_t version, uint32_t data_len,
                                            uint32_t max_fragment, uint32_t tag_len,
                                            uint32_t pad_block) {
  const bool gcm = aead == TLSGPU_AES_128_GCM || aead == TLSGPU_AES_256_GCM;
  const bool cc13 = aead == TLSGPU_CHACHA20_POLY1305_TLS13;
  // pad_block as an install reads it: TLS 1.3 sessions only, a power of two up to 16384
  const bool padded = version == kTls13Version && (gcm || cc13) && pad_block > 1 &&
                      pad_block <= 16384 && (pad_block & (pad_block - 1)) == 0;
  if (!padded) {
    if (version != kTls13Version || !gcm)  // (the TLS 1.3 ChaCha kind: TLS 1.3 framing there too)
      return tlsgpu_seal_wire_size(aead, data_len, max_fragment, tag_len);
    // TLS 1.3: header(5) || content || inner type(1) || tag(16) per record, no explicit nonce
    const uint32_t frag = max_fragment == 0 || max_fragment > 16384 ? 16384 : max_fragment;
    const uint64_t nrec = ((uint64_t)data_len + frag - 1) / frag;
    return data_len + nrec * (5 + 1 + 16);
  }
  // header(5) || padded inner plaintext || tag(16): every record but the last
  // holds frag bytes, the last the remainder
  const uint32_t frag = max_fragment == 0 || max_fragment > 16384 ? 16384 : max_fragment;
  const uint32_t mask = pad_block - 1;
  const uint64_t full = data_len / frag, rest = data_len % frag;
  return full * (5 + (uint64_t)tls13_inner_len(frag, mask) + 16) +
         (rest ? 5 + (uint64_t)tls13_inner_len((uint32_t)rest, mask) + 16 : 0);
}

extern "C" int tlsgpu_fill_synthetic(tlsgpu_engine* e, uint8_t* d_out, uint64_t stride,
                                     uint32_t span_len, uint32_t n, uint64_t seed,
                                     uint64_t index0, void* stream) {
  if (!e || (!d_out && n)) return fail(TLSGPU_EINVAL, "bad arguments");
  HIPCHK(hipSetDevice(e->device));
  if (launch_fill_synthetic(d_out, stride, span_len, n, seed, index0,
                            stream ? (hipStream_t)stream : e->stream))
    return fail(TLSGPU_EHIP, "fill launch: %s", hipGetErrorString(hipGetLastError()));
  return TLSGPU_OK;
}

extern "C" int tlsgpu_fill_synthetic_spans(tlsgpu_engine* e, uint8_t* d_out,
                                           const uint64_t* d_offsets, const uint32_t* d_lengths,
                                           uint32_t n, uint64_t seed, uint64_t index0,
                                           void* stream) {
  if (!e || (n && (!d_out || !d_offsets || !d_lengths))) return fail(TLSGPU_EINVAL, "bad arguments");
  HIPCHK(hipSetDevice(e->device));
  if (launch_fill_synthetic_spans(d_out, d_offsets, d_lengths, n, seed, index0,
                                  stream ? (hipStream_t)stream : e->stream))
    return fail(TLSGPU_EHIP, "fill launch: %s", hipGetErrorString(hipGetLastError()));
  return TLSGPU_OK;
}
