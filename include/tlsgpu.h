/*
 * tlsgpu.h — MI355X-native TLS record bulk-cipher engine: batch C ABI
 * (TLS 1.2 AEAD records as LibreSSL 2.4.1 protects them, and TLS 1.3 AES-GCM
 * and ChaCha20-Poly1305 records, RFC 8446 5.2-5.4: see "TLS 1.3 sessions"
 * below).
 *
 * This is the GPU extension that sits beside the drop-in EVP_AEAD ABI
 * (include/tlsgpu_evp.h).  It has no reference counterpart; it batches the
 * per-record work that LibreSSL 2.4.1 does one record at a time in
 *   tls1_enc() AEAD branch            ssl/t1_enc.c:832-975
 *     -> EVP_AEAD_CTX_seal / _open    crypto/evp/evp_aead.c:89-144
 *       -> aead_aes_gcm_seal / _open  crypto/evp/e_aes.c:1424-1510
 *       -> aead_chacha20_poly1305_*   crypto/evp/e_chacha20poly1305.c:124-286
 * and moves the per-direction key install of
 *   tls1_change_cipher_state_aead()   ssl/t1_enc.c:444-495
 * into a device session table.
 *
 * All pointers named d_* are device (HBM) pointers; the API never touches
 * torch or any framework type.  Streams are hipStream_t passed as void*.
 * Every function returns TLSGPU_OK (0) or a negative TLSGPU_E* code.
 */
#ifndef TLSGPU_H
#define TLSGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TLSGPU_ABI_VERSION 2	/* 2: batch calls take buffer sizes */

/* AEAD kinds (crypto/evp/e_aes.c:1512-1546, e_chacha20poly1305.c:288-322). */
enum tlsgpu_aead {
	TLSGPU_AES_128_GCM = 1,
	TLSGPU_AES_256_GCM = 2,
	TLSGPU_CHACHA20_POLY1305 = 3,	/* RFC 7539/7905, 12-byte nonce */
	TLSGPU_CHACHA20_POLY1305_OLD = 4,	/* draft-agl, 8-byte nonce */
	/* TLS_CHACHA20_POLY1305_SHA256 in the TLS 1.3 record layout (RFC 8446
	 * 5.2-5.4): the cipher and the nonce are kind 3's, the record layout is
	 * not.  The layout is carried by the kind, not by the version alone: _OLD
	 * already names a record layout rather than a cipher, the ChaCha kernels
	 * dispatch on the session's kind, and a caller who only bumps a TLS 1.2
	 * ChaCha session's version to 0x0304 gets TLSGPU_EINVAL, not silently
	 * different AAD.  Valid only with version 0x0304. */
	TLSGPU_CHACHA20_POLY1305_TLS13 = 5
};

/* Return codes. */
#define TLSGPU_OK 0
#define TLSGPU_EINVAL (-1)
#define TLSGPU_ENOMEM (-2)
#define TLSGPU_EHIP (-3)	/* HIP runtime error (no GPU, launch failure) */
#define TLSGPU_ERANGE (-4)	/* session id / size out of range */
#define TLSGPU_ETIMEOUT (-5)	/* a bounded wait expired (tlsgpu_evp_shutdown) */

/* Per-record status written by the batch calls (int32 per record).
 *   >= 0  success: plaintext length (open) or record body length (seal)
 *   TLSGPU_REC_BAD_MAC         tls1_enc returns -1 -> bad_record_mac alert
 *                              (s3_pkt.c:450-462); the plaintext region
 *                              [out, out+len) is zero-filled as
 *                              EVP_AEAD_CTX_open does (evp_aead.c:137-143)
 *   TLSGPU_REC_PUBLIC_INVALID  tls1_enc returns 0: record shorter than the
 *                              explicit nonce or the tag (t1_enc.c:930,958)
 */
#define TLSGPU_REC_BAD_MAC (-1)
#define TLSGPU_REC_PUBLIC_INVALID (-2)
/* tlsgpu_open_wire only: an earlier record of the same stream failed, so
 * ssl3_get_record would never have returned this one (not delivered). */
#define TLSGPU_REC_SKIPPED (-3)
/* tlsgpu_open_wire only: plaintext longer than SSL3_RT_MAX_PLAIN_LENGTH
 * (s3_pkt.c:465-469) -> record_overflow alert, not delivered. */
#define TLSGPU_REC_OVERFLOW (-4)
/* tlsgpu_open_batch / _seal_batch: the record's input span (in_off, length) or
 * output span (out_off, plaintext / fragment length) leaves d_in / d_out as
 * sized by the caller; nothing of the record was read or written. */
#define TLSGPU_REC_OUT_OF_BOUNDS (-5)
/* TLS 1.3 open only: the tag verified but the decrypted TLSInnerPlaintext is
 * empty or all zero, so it carries no content type (RFC 8446 5.4:
 * unexpected_message).  The output region stays as decrypted. */
#define TLSGPU_REC_NO_CONTENT_TYPE (-6)

/* Largest plaintext per record the AES-GCM batch kernels accept: 65534 AES
 * blocks, so GCM counters 2..nb+1 stay below 2^16 (TLS records are <= 16 KiB +
 * 2 KiB, ssl3.h:259-280).  A longer record of an AES-GCM session gets
 * TLSGPU_REC_PUBLIC_INVALID and not a byte of it is written.  The limit is the
 * AES-GCM kinds' alone: the ChaCha20-Poly1305 kernels (TLS 1.2 RFC 7905 and
 * draft suites, and TLSGPU_CHACHA20_POLY1305_TLS13) have a 32-bit block
 * counter, do not check it, and process a longer record like any other, up to
 * the 24 bits of the descriptor's length (tests/test_gpu_record_limit.py pins
 * both).  In every kind the 16-bit length in the additional data of a record
 * above 65535 bytes is the length's low 16 bits. */
#define TLSGPU_MAX_RECORD (65534u * 16u)

/* One TLS record, 32 bytes, device-resident array.
 * open: in_off -> record fragment after the 5-byte header
 *       (GCM: explicit nonce(8) || ct || tag(16); ChaCha: ct || tag(16)),
 *       length = fragment length; plaintext written at out_off
 *       (the TLS layer passes out = fragment + 8 for GCM, t1_enc.c:951-955).
 * seal: in_off -> plaintext, length = plaintext length; the fragment
 *       (explicit nonce || ct || tag) is written at out_off (t1_enc.c:898-914).
 * seq is the record's 64-bit sequence number (read_sequence/write_sequence
 * before tls1_record_sequence_increment, t1_enc.c:258-266,841-847).
 *
 * TLS 1.3 sessions (version 0x0304; AES-GCM kinds or
 * TLSGPU_CHACHA20_POLY1305_TLS13; RFC 8446 5.2-5.4).  The record
 * nonce is fixed_iv(12) XOR (0^32 || BE64(seq)), there is no explicit nonce,
 * and the AAD is the record header 0x17 0x03 0x03 BE16(ciphertext length with
 * the tag); the descriptor's type bits do not enter it.
 * seal: in_off / length are the content and the type bits the INNER content
 *       type.  The engine encrypts content || type || zeros, padded to the
 *       session's pad_block (RFC 8446 5.4; OpenSSL's block padding rule):
 *         inner = length + 1                     pad_block <= 1 or length >= 16384
 *         inner = roundup(length + 1, pad_block) otherwise
 *       and writes ciphertext || tag(16), inner + 16 bytes, at out_off; status
 *       = inner + 16 and the AAD's length field is inner + 16.  Without a
 *       padding block that is length + 1 + 16.  The type byte and the zeros
 *       are synthesized: d_in is never read past in_off + length.
 * open: length is the fragment, ciphertext || tag.  The decrypted
 *       TLSInnerPlaintext (length - 16 bytes, its zero padding included) is
 *       written at out_off (in place: out_off = in_off).  status = the CONTENT
 *       length, i.e. the index of the last non-zero byte; the inner content
 *       type is the byte at out_off + status.  TLSGPU_REC_NO_CONTENT_TYPE: the
 *       tag verified but the inner plaintext is empty or all zero (region as
 *       decrypted).  TLSGPU_REC_BAD_MAC zero-fills all length - 16 bytes;
 *       length < 16 gives TLSGPU_REC_PUBLIC_INVALID.
 * For the AES-GCM kinds TLSGPU_MAX_RECORD bounds the inner plaintext (a seal's
 * content is at most TLSGPU_MAX_RECORD - 1 bytes); TLSGPU_CHACHA20_POLY1305_TLS13
 * has no such limit, as in TLS 1.2.  The bounds rule of TLSGPU_REC_OUT_OF_BOUNDS
 * uses these spans.  All the rest holds for the three TLS 1.3 kinds alike
 * (ChaCha20-Poly1305: RFC 7905's nonce is RFC 8446's).
 * Limits: post-handshake records only (the compatibility ChangeCipherSpec of a
 * handshake is the caller's to skip). */
typedef struct tlsgpu_record {
	uint64_t in_off;
	uint64_t out_off;
	uint64_t seq;
	uint32_t session;
	uint32_t len_type;	/* bits 0-23: length; bits 24-31: content type */
} tlsgpu_record;

#define TLSGPU_LEN_TYPE(len, type) (((uint32_t)(type) << 24) | ((uint32_t)(len) & 0xFFFFFFu))

/* Session parameters as installed at ChangeCipherSpec
 * (t1_enc.c:444-495; nonce lengths from s3_lib.c cipher table). */
typedef struct tlsgpu_session_params {
	int32_t aead;			/* enum tlsgpu_aead */
	uint32_t key_len;		/* 16 or 32 */
	uint8_t key[32];
	uint32_t fixed_iv_len;		/* 4 (GCM), 12 (ChaCha, every TLS 1.3 kind), 0 (ChaCha old) */
	uint8_t fixed_iv[12];
	uint32_t tag_len;		/* 0 = default 16 (EVP_AEAD_DEFAULT_TAG_LENGTH) */
	uint16_t version;		/* s->version, e.g. 0x0303; 0x0304: a TLS 1.3 session */
	uint16_t pad_block;		/* version 0x0304 only (ignored otherwise): seal pads
					 * the inner plaintext to a multiple of this; 0, 1 =
					 * no padding, else a power of two, 2..16384 */
} tlsgpu_session_params;
/* A TLS 1.3 session is aead = TLSGPU_AES_128_GCM / _256_GCM /
 * TLSGPU_CHACHA20_POLY1305_TLS13, version = 0x0304, fixed_iv_len = 12 (the
 * traffic secret's write IV; the key is its write key, and seq starts at 0 for
 * every key), tag_len 16 (0 means 16).  0x0304 with any other fixed_iv_len,
 * tag_len or with a TLS 1.2 ChaCha kind (3, 4) is TLSGPU_EINVAL at install, and
 * so is TLSGPU_CHACHA20_POLY1305_TLS13 with any other version, a key_len other
 * than 32, another fixed_iv_len or tag_len.  Every other version behaves as
 * before.  The three TLS 1.3 kinds share tables and batches.
 * pad_block is the session's record padding policy (the rule under "TLS 1.3
 * sessions" above; what OpenSSL's SSL_CTX_set_block_padding / RecordPadding
 * do).  It is read for version 0x0304 only.  Powers of two only, and anything
 * else is TLSGPU_EINVAL at install, is a deliberate limit: the padded length is
 * derived per record in several kernels, and a mask keeps a division out of them.
 * One session table holds one generation: the GCM kernels are compiled once
 * per record layout (carrying the layout as per-session data cost the TLS 1.2
 * queue kernel's pack variants spilled registers), so the
 * first install fixes whether a table is TLS 1.3 or not, and an install of the
 * other generation returns TLSGPU_EINVAL.  A server keeps one table per
 * generation; batches of the two run side by side on their own streams. */

typedef struct tlsgpu_engine tlsgpu_engine;
typedef struct tlsgpu_sessions tlsgpu_sessions;

/* Number of visible GPUs (0 when no device / no driver). */
int tlsgpu_device_count(int *count);

/* Engine = one GPU + one HIP stream + scratch pools. */
int tlsgpu_engine_create(int device, tlsgpu_engine **out);
void tlsgpu_engine_destroy(tlsgpu_engine *e);
/* The engine's stream (hipStream_t) for callers that order their own work. */
void *tlsgpu_engine_stream(tlsgpu_engine *e);
int tlsgpu_engine_sync(tlsgpu_engine *e);
/* Compute units of the engine's device (256 on MI355X). */
int tlsgpu_engine_num_cus(tlsgpu_engine *e);

/* Device session table with room for `capacity` sessions. */
int tlsgpu_sessions_create(tlsgpu_engine *e, uint32_t capacity, tlsgpu_sessions **out);
void tlsgpu_sessions_destroy(tlsgpu_sessions *t);
/* Install n sessions (host params) at ids first..first+n-1.  Key schedule,
 * H = E_K(0^128) and the GHASH power tables are derived on the device. */
int tlsgpu_sessions_install(tlsgpu_sessions *t, uint32_t first, uint32_t n,
    const tlsgpu_session_params *params);

/* ---------------------------------------------------------------------------
 * The TLS 1.3 key schedule behind a traffic secret, on the device (RFC 8446
 * 7.1-7.3).
 *
 * A TLS 1.3 session given as its traffic secret (client/server
 * application_traffic_secret_N).  The hash of the key schedule follows from the
 * suite (RFC 8446 B.4): SHA-256 for TLSGPU_AES_128_GCM and
 * TLSGPU_CHACHA20_POLY1305_TLS13 (secret_len 32), SHA-384 for
 * TLSGPU_AES_256_GCM (secret_len 48).  Any other kind or a secret_len that does
 * not match is TLSGPU_EINVAL.  pad_block as in tlsgpu_session_params.  version
 * is implied (0x0304), tag 16, IV 12. */
typedef struct tlsgpu_secret_params {
	int32_t  aead;
	uint32_t secret_len;
	uint8_t  secret[48];
	uint16_t pad_block;
	uint16_t reserved;     /* 0 */
} tlsgpu_secret_params;    /* 60 bytes */

/* Install n sessions from their traffic secrets at ids first..first+n-1.
 * Synchronous and host-visible like tlsgpu_sessions_install, with its range
 * check, its one-generation-per-table rule (this is a TLS 1.3 install: on a
 * TLS 1.2 table it is TLSGPU_EINVAL) and its pad_block check; everything is
 * checked before the first GPU call.  The device derives
 *   key = HKDF-Expand-Label(secret, "key", "", key_len)
 *   iv  = HKDF-Expand-Label(secret, "iv", "", 12)
 * and installs the slot exactly as tlsgpu_sessions_install would for those
 * bytes; the slot also keeps the secret, which is what lets
 * tlsgpu_sessions_key_update move it on.  The staging copy of the secrets in
 * device memory is zeroed before the call returns, and no key or secret
 * travels as a kernel argument.  A later tlsgpu_sessions_install over the slot
 * clears its secret.  The first call allocates the table's key-schedule scratch
 * (8 MiB and 4 bytes per session of capacity), freed with the table.
 * It must not overlap a tlsgpu_sessions_key_update of the same table that is
 * still running on another stream (the two share the scratch). */
int tlsgpu_sessions_install_secrets(tlsgpu_sessions *t, uint32_t first, uint32_t n,
    const tlsgpu_secret_params *params);

/* KeyUpdate (RFC 8446 4.6.3, 7.2) for n session slots, on the device and
 * asynchronous on `stream` (NULL = engine stream): no host round trip, no
 * allocation, no synchronising call.  d_ids and d_status are device arrays of
 * n.  For each i, slot d_ids[i] moves one generation on:
 *   secret' = HKDF-Expand-Label(secret, "traffic upd", "", Hash.length)
 * the key and IV come from secret' as above, the slot is installed again (key
 * schedule, H, GHASH tables, or the ChaCha key; its kind, padding block and
 * everything else stay) and keeps secret'.
 *   d_status[i] = TLSGPU_OK             the slot was rekeyed
 *                 TLSGPU_REKEY_SKIPPED  d_ids[i] == TLSGPU_SESSION_NONE
 *                 TLSGPU_ERANGE         the id is >= capacity; nothing is touched
 *                 TLSGPU_EINVAL         the slot holds no secret (empty, or installed
 *                                       from a key); not one byte of it changes
 * An id listed several times in one call is rekeyed ONCE (every entry reports
 * TLSGPU_OK): all derivations read the old generation before any install
 * writes.  Slots not listed are not touched.  The host's view of the table does
 * not change (kind and padding stay), so the call takes no lock.
 * A null table, d_ids or d_status with n > 0 is TLSGPU_EINVAL before any GPU
 * call; n == 0 is TLSGPU_OK and launches nothing.
 * Ordering is the caller's, as for installs: the call goes behind the batches
 * that use the old keys and before those that use the new ones (one stream
 * does it).  Two tlsgpu_sessions_key_update calls on one table must be ordered
 * against each other, by using one stream or by waiting for the first: they
 * share the table's scratch.  Sequence numbers restart at 0 under the new keys;
 * that is the caller's `seq`, as ever. */
#define TLSGPU_SESSION_NONE 0xFFFFFFFFu
#define TLSGPU_REKEY_SKIPPED 1
int tlsgpu_sessions_key_update(tlsgpu_sessions *t, const uint32_t *d_ids, uint32_t n,
    int32_t *d_status, void *stream);

/* Batch record decrypt / encrypt (device-resident).  Any record order is
 * correct; grouping each session's records together is fastest.  in_bytes /
 * out_bytes are the sizes of d_in / d_out: records whose spans leave them get
 * TLSGPU_REC_OUT_OF_BOUNDS and are not touched.  d_status: int32 per record.
 * d_in == d_out is allowed (in-place open at out_off = in_off + 8 for GCM,
 * t1_enc.c:951-955).  Asynchronous on `stream` (NULL = engine stream). */
int tlsgpu_open_batch(tlsgpu_sessions *t, const tlsgpu_record *d_recs, uint32_t n,
    const uint8_t *d_in, size_t in_bytes, uint8_t *d_out, size_t out_bytes, int32_t *d_status,
    void *stream);
int tlsgpu_seal_batch(tlsgpu_sessions *t, const tlsgpu_record *d_recs, uint32_t n,
    const uint8_t *d_in, size_t in_bytes, uint8_t *d_out, size_t out_bytes, int32_t *d_status,
    void *stream);

/* Batch-shape hints for the AES-GCM batch calls of this session table
 * (performance only: results never depend on them, any batch stays correct).
 * The default kernel selection happens on the device, so every GCM batch
 * dispatches the long-record kernel, its short-record-pack variant and the
 * per-wave-session kernel, and the two not selected exit at once (~5 us each).
 * A caller that knows its batches rules them out:
 *   TLSGPU_HINT_NO_SHORT_RECORDS  no GCM record of <= 62 blocks (open: length
 *                                 <= 1,016 B with the 8-B explicit nonce and a
 *                                 16-B tag; TLS 1.3: 62 blocks of inner
 *                                 plaintext, open length <= 1,008 B, seal: the
 *                                 PADDED inner plaintext <= 992 B, i.e. length
 *                                 <= 991 B without a padding block and never
 *                                 with pad_block >= 1024): the pack variant is
 *                                 not launched;
 *   TLSGPU_HINT_SESSION_RUNS      records come in session runs of >= 12
 *                                 records on average: the per-wave-session
 *                                 kernel is not launched.
 * A wrong hint costs speed only (short records then take the long-record
 * path, short runs the run-at-a-time queue).  tlsgpu_open_host /
 * tlsgpu_seal_host derive the hints from the host descriptors themselves. */
#define TLSGPU_HINT_NO_SHORT_RECORDS 1u
#define TLSGPU_HINT_SESSION_RUNS 2u
int tlsgpu_sessions_hint(tlsgpu_sessions *t, unsigned hints);

/* ---------------------------------------------------------------------------
 * Host-resident batch open: records that start and end in
 * host memory, as socket buffers do.  Replaces, for a batch of connections,
 * ssl3_read_n's BIO_read into rbuf (ssl/s3_pkt.c:134-267), tls1_enc(s, 0)
 * and the copy of the plaintext to the application buffer (s3_pkt.c:957).
 *
 * h_recs / h_in / h_out / h_status are HOST pointers (pinned memory from
 * tlsgpu_host_alloc for full PCIe rate; pageable memory works, slower).
 * Descriptor offsets are relative to h_in / h_out exactly as for
 * tlsgpu_open_batch; h_out == h_in opens in place.  The engine mirrors the
 * buffers in HBM and pipelines the batch in chunks (H2D of chunk k+1 and D2H
 * of chunk k-1 on their own streams overlap the kernels of chunk k) when
 * the records' in_off and out_off ascend with the record index; otherwise it
 * runs the batch as one chunk.  Synchronous: returns when h_out and h_status
 * are final, and also on every error — no copy into or out of the caller's
 * buffers is still running once it has returned.  Bytes of h_out between the
 * records' plaintext spans (from the first span to the last, or all of
 * out_bytes when the layout does not ascend) come back as zeros out of place;
 * in place, the headers, explicit nonces and tags are written back unchanged.
 * Bytes outside that range are not touched.  TLS 1.3 tables: spans, statuses
 * and the read hook follow the TLS 1.3 rules above (the hook sees the content,
 * status bytes; the inner type follows it in h_out). */
int tlsgpu_open_host(tlsgpu_sessions *t, const tlsgpu_record *h_recs, uint32_t n,
    const uint8_t *h_in, size_t in_bytes, uint8_t *h_out, size_t out_bytes, int32_t *h_status);
/* The write direction: plaintext records in host memory (h_in) sealed into
 * host fragments (h_out, explicit nonce || ciphertext || tag at out_off;
 * headers are the caller's, or use tlsgpu_seal_wire).  Not in place. */
int tlsgpu_seal_host(tlsgpu_sessions *t, const tlsgpu_record *h_recs, uint32_t n,
    const uint8_t *h_in, size_t in_bytes, uint8_t *h_out, size_t out_bytes, int32_t *h_status);

/* TaLoS plaintext-processing hooks.  libtlsgpu implements TaLoS's own
 * interface (include/tlsgpu_talos.h: tls_processing_register_*_cb with the
 * reference signatures, tls_processing_interface.h:23-27), so a TaLoS module
 * registers against the engine unchanged.  The registered read / write
 * callbacks run on host plaintext, with the SSL* the caller associated with
 * the record's session (NULL if none):
 *   write  tlsgpu_seal_host: each record before the batch is copied to the
 *          device, in record order (do_ssl3_write's call, s3_pkt.c.patch:19-33);
 *          the module may rewrite the bytes in place and shorten the record;
 *          tlsgpu_hook_write_streams: each fragment of host application data
 *          that tlsgpu_seal_wire will seal;
 *   read   tlsgpu_open_host and tlsgpu_deliver_host (the batch and wire paths'
 *          host delivery): each delivered record's plaintext once it is in
 *          host memory, in record order (ssl3_read_bytes' call,
 *          s3_pkt.c.patch:39-52); a module that shortens *len shortens the
 *          delivered status.
 * tlsgpu_group_* calls run them per member, in record order within each
 * member's slice. */
int tlsgpu_sessions_set_owner(tlsgpu_sessions *t, uint32_t first, uint32_t n,
    const void *const *owners);
/* Host delivery of a device-resident open (tlsgpu_open_batch, or
 * tlsgpu_open_wire with d_out = d_wire): copies the n descriptors' statuses to
 * h_status and the delivered records' output range [first out_off, last
 * out_off + status) of d_out to the same offsets of h_out (out_bytes = size of
 * d_out / h_out), then runs the read hook on each delivered record.
 * Synchronous on `stream` (NULL = engine stream; order it after the open). */
int tlsgpu_deliver_host(tlsgpu_sessions *t, const tlsgpu_record *d_recs, const int32_t *d_status,
    uint32_t n, const uint8_t *d_out, size_t out_bytes, uint8_t *h_out, int32_t *h_status,
    void *stream);
/* Write hook over host application data before the caller uploads it for
 * tlsgpu_seal_wire: every fragment of every stream (h_streams: host copy of
 * the write streams, offsets into h_data), in place, lengths unchanged. */
struct tlsgpu_write_stream; /* defined below, with tlsgpu_seal_wire */
int tlsgpu_hook_write_streams(tlsgpu_sessions *t, const struct tlsgpu_write_stream *h_streams,
    uint32_t n_streams, uint8_t *h_data, size_t data_bytes);
/* read / write hook invocations since load (from the patched record layer
 * and the engine's paths alike). */
int tlsgpu_talos_hook_stats(uint64_t *read_calls, uint64_t *write_calls);
/* Pipeline shape of tlsgpu_open_host: `streams` compute streams (1..8, default
 * 2; copies in and out have a stream each), chunks of about `chunk_bytes`
 * input bytes (default 32 MiB). */
int tlsgpu_host_pipeline(tlsgpu_engine *e, unsigned streams, size_t chunk_bytes);

/* ---------------------------------------------------------------------------
 * Multi-GPU batch split (BASELINE configs[4]).  Records are
 * independent, so a batch splits into contiguous slices of about equal bytes,
 * one per GPU, with no collective and no xGMI traffic.  A group is one engine
 * per listed device (the same device may be listed twice: two engines, two
 * streams) and one host worker thread per engine; session tables are
 * replicated on every member.  This is what a caller of the per-record
 * tls1_enc (ssl/t1_enc.c:911,964) that batches — a record layer with
 * read-ahead over many connections — binds to use every GPU of the node. */
typedef struct tlsgpu_group tlsgpu_group;
typedef struct tlsgpu_group_sessions tlsgpu_group_sessions;

/* devices == NULL or n == 0: every visible GPU. */
int tlsgpu_group_create(const int *devices, uint32_t n, tlsgpu_group **out);
void tlsgpu_group_destroy(tlsgpu_group *g);
uint32_t tlsgpu_group_size(const tlsgpu_group *g);
tlsgpu_engine *tlsgpu_group_engine(tlsgpu_group *g, uint32_t member);
/* One session table per member, same capacity; install writes every member. */
int tlsgpu_group_sessions_create(tlsgpu_group *g, uint32_t capacity, tlsgpu_group_sessions **out);
void tlsgpu_group_sessions_destroy(tlsgpu_group_sessions *gs);
tlsgpu_sessions *tlsgpu_group_sessions_member(tlsgpu_group_sessions *gs, uint32_t member);
int tlsgpu_group_sessions_install(tlsgpu_group_sessions *gs, uint32_t first, uint32_t n,
    const tlsgpu_session_params *params);
/* tlsgpu_sessions_install_secrets on every member.  There is no group-wide
 * KeyUpdate: run tlsgpu_sessions_key_update on tlsgpu_group_sessions_member(gs, k). */
int tlsgpu_group_sessions_install_secrets(tlsgpu_group_sessions *gs, uint32_t first,
    uint32_t n, const tlsgpu_secret_params *params);

/* Byte-balanced contiguous split of n records into `parts` slices: cuts[0] = 0
 * <= cuts[1] <= ... <= cuts[parts] = n, slice k = records [cuts[k], cuts[k+1]).
 * Cut k is the first record boundary whose prefix of record lengths (len_type
 * bits 0-23) reaches k/parts of the total (integer arithmetic; equal lengths
 * give equal counts).  Host only, no GPU call. */
int tlsgpu_split_by_bytes(const tlsgpu_record *recs, uint32_t n, uint32_t parts, uint32_t *cuts);

/* Host-resident batch over the group: slice k (tlsgpu_split_by_bytes) runs as
 * tlsgpu_open_host / tlsgpu_seal_host on member k, all members at once, each
 * from its own worker thread (its own PCIe link and HBM).  Same buffers,
 * offsets, statuses and synchronous contract as the single-GPU calls; the
 * first member error is returned after every member has finished. */
int tlsgpu_group_open_host(tlsgpu_group_sessions *gs, const tlsgpu_record *h_recs, uint32_t n,
    const uint8_t *h_in, size_t in_bytes, uint8_t *h_out, size_t out_bytes, int32_t *h_status);
int tlsgpu_group_seal_host(tlsgpu_group_sessions *gs, const tlsgpu_record *h_recs, uint32_t n,
    const uint8_t *h_in, size_t in_bytes, uint8_t *h_out, size_t out_bytes, int32_t *h_status);

/* Device-resident batch over the group (per-GPU pools): shards[k] is member
 * k's slice, already in that member's HBM.  Launched on every member's engine
 * stream; asynchronous — tlsgpu_group_sync waits for all members. */
typedef struct tlsgpu_shard {
	const tlsgpu_record *d_recs;
	uint32_t n;
	uint32_t reserved;
	const uint8_t *d_in;
	size_t in_bytes;
	uint8_t *d_out;
	size_t out_bytes;
	int32_t *d_status;
} tlsgpu_shard;
int tlsgpu_group_open_batch(tlsgpu_group_sessions *gs, const tlsgpu_shard *shards);
int tlsgpu_group_seal_batch(tlsgpu_group_sessions *gs, const tlsgpu_shard *shards);
int tlsgpu_group_sync(tlsgpu_group *g);

/* ---------------------------------------------------------------------------
 * Wire-record framing: ssl3_get_record (ssl/s3_pkt.c:279-495)
 * for the AEAD suites over raw read-ahead bytes, many connections at once.
 *
 * Each stream is one connection's read direction: wire_len bytes of TLS
 * records (5-byte header + fragment) at d_wire + wire_off, as ssl3_read_n
 * leaves them in rbuf with read_ahead (s3_pkt.c:134-267).  Per stream, records
 * are framed in order with the header checks of s3_pkt.c:304-341,376:
 *   version != stream version (unless TLSGPU_WIRE_FIRST_PACKET) -> alert
 *   protocol_version (70); major != 3 -> error without alert (alert = -1);
 *   length > rbuf_len - 5 (rbuf_len 0 = the reference's 16712) or
 *   length > SSL3_RT_MAX_ENCRYPTED_LENGTH (16704) -> record_overflow (22);
 *   a record whose fragment is not complete ends the stream's batch (the
 *   caller keeps the bytes from `consumed` on for the next call).
 * Framed records get descriptors (written to d_recs, grouped by stream, seq =
 * stream seq + index) and are opened IN PLACE like tls1_enc(s, 0)
 * (t1_enc.c:951-955: plaintext at fragment + explicit nonce length).  Then,
 * in order, the first record with an AEAD failure or a plaintext longer than
 * 16384 B ends the stream: bad_record_mac (20) for TLSGPU_REC_BAD_MAC,
 * decryption_failed (21) for TLSGPU_REC_PUBLIC_INVALID, record_overflow (22)
 * for TLSGPU_REC_OVERFLOW; later records of that stream get
 * TLSGPU_REC_SKIPPED.  Zero-length plaintexts are delivered with status 0 (the
 * reference reads on, s3_pkt.c:486-488).
 *
 * max_records bounds d_recs / d_status; streams whose records do not fit are
 * truncated at a record boundary (their `records`/`consumed` say how far; a
 * truncated stream reaches no header alert, and its delivered / alert /
 * alert_record come from the records it kept).  A stream's slots are one
 * contiguous range, but the ranges are handed out in no fixed order once the
 * call has more than four streams: read `first`, do not compute it.  A stream
 * without records reports first = 0.
 * d_total receives the number of records the streams framed, whether or not
 * their descriptors fit: it may exceed max_records, and then min(d_total,
 * max_records) descriptors were written.  Slots no stream got hold all-ones
 * descriptors and the status TLSGPU_REC_PUBLIC_INVALID.
 * d_wire: the call writes plaintext spans only (fragment + explicit nonce, the
 * fragment's length minus explicit nonce and tag): the plaintext of a record
 * the AEAD accepted (one above 16384 B too), zeros for TLSGPU_REC_BAD_MAC.
 * The plaintext span of a TLSGPU_REC_SKIPPED record is unspecified (opened,
 * zeroed or untouched); every other byte of d_wire (headers, explicit nonces,
 * tags, incomplete tails, the bytes between streams) is never written.
 * Asynchronous.
 *
 * Streams of a TLS 1.3 table, AES-GCM and ChaCha20-Poly1305 sessions alike
 * (the caller passes version = 0x0303, the legacy
 * record version): the outer type must be 23, else unexpected_message (10); a
 * fragment above 16384 + 256 B gives record_overflow (22), one below 16 B
 * decryption_failed (21); records are opened in place at the fragment start.
 * Then, in order: TLSGPU_REC_NO_CONTENT_TYPE ends the stream with alert 10, a
 * content length above 16384 with TLSGPU_REC_OVERFLOW and alert 22; for
 * delivered records the inner content type replaces the type bits of
 * d_recs[i].len_type, so alerts and handshake records look as in TLS 1.2. */
#define TLSGPU_WIRE_FIRST_PACKET 1u	/* s->first_packet: accept any version */
typedef struct tlsgpu_wire_stream {
	uint64_t wire_off;	/* first byte of the stream in d_wire */
	uint32_t wire_len;	/* bytes available */
	uint32_t session;	/* read-direction session id */
	uint64_t seq;		/* read sequence number of the first record */
	uint16_t version;	/* s->version, e.g. 0x0303 */
	uint16_t flags;		/* TLSGPU_WIRE_* */
	uint32_t rbuf_len;	/* read buffer size for the overflow check; 0 = 16712 */
} tlsgpu_wire_stream;

typedef struct tlsgpu_wire_result {
	uint32_t first;		/* index of the stream's first record in d_recs / d_status; 0 if none */
	uint32_t records;	/* records framed (descriptors written) */
	uint32_t delivered;	/* records before the first failure */
	uint32_t consumed;	/* bytes of the framed records (header + fragment) */
	int32_t alert;		/* 0, a fatal TLS AlertDescription, or -1 (error, no alert) */
	uint32_t alert_record;	/* index within the stream of the record that failed */
	uint32_t key_update;	/* TLSGPU_WIRE_KU_* (tlsgpu_sessions_wire_key_update); else 0 */
	uint32_t reserved;
} tlsgpu_wire_result;

/* ---------------------------------------------------------------------------
 * KeyUpdate on the wire read path (RFC 8446 4.6.3, 7.2).  Every record behind a
 * KeyUpdate is protected under the next traffic keys with the sequence number
 * back at 0, so a read-ahead that holds one cannot be opened under one session:
 * the records behind it would fail their tags and be zero-filled in d_wire.
 *
 * tlsgpu_sessions_wire_key_update(t, 1) makes tlsgpu_open_wire cut a stream at
 * a KeyUpdate BEFORE anything behind it is opened.  A per-table switch, off by
 * default; it is not a hint, results depend on it.  It acts on tlsgpu_open_wire
 * only, and there only on streams whose session is a TLS 1.3 session; on a
 * TLS 1.2 table it is accepted and changes nothing.  A null table is
 * TLSGPU_EINVAL.  With the switch off tlsgpu_open_wire is what it was, and
 * key_update is always TLSGPU_WIRE_KU_NONE (as it is for TLS 1.2 streams and
 * streams of unknown sessions with the switch on).
 *
 * The rule.  Between framing and the open, the engine decrypts the first
 * min(16, inner length) bytes of every framed record (one cipher block, no
 * authentication) and takes the first record of the stream whose
 * TLSInnerPlaintext begins 18 00 00 01 rr 16 (rr <= 1) with only zeros up to
 * byte 15 as the candidate: a KeyUpdate handshake message alone in its record.
 * The stream is cut after the candidate:
 *   records = the candidate's index + 1, consumed ends with its last byte;
 *   a header-level alert that framing found behind the cut is dropped (alert =
 *   0, alert_record = records; the next call finds it again);
 *   the descriptor slots framing had reserved behind the cut are reset to all
 *   ones like unused slots (d_total still counts them, their statuses are what
 *   the open leaves for unused slots);
 *   not one byte of d_wire from wire_off + consumed on is read by the open or
 *   written by anyone.
 * The peek is unauthenticated, so it decides only where the batch is cut, never
 * what the caller is told: a look-alike or a forgery costs the stream a shorter
 * batch and nothing else.  key_update is set after the normal open, from the
 * verified record:
 *   TLSGPU_WIRE_KU_UPDATE            record records - 1 was delivered, is of inner
 *                                    type 22 and its content is exactly 18 00 00 01 00;
 *   TLSGPU_WIRE_KU_UPDATE_REQUESTED  the same with 18 00 00 01 01: the caller also
 *                                    owes the peer a KeyUpdate of its own;
 *   TLSGPU_WIRE_KU_HELD              the stream was cut after record records - 1, but
 *                                    that record is no KeyUpdate: it failed its tag
 *                                    (`alert` says so as usual), or it verified with
 *                                    another type or other content.  Go on from
 *                                    `consumed` under the same keys with seq +
 *                                    records, unless `alert` ended the stream.
 * After TLSGPU_WIRE_KU_UPDATE*: the stream's read session slot moves to
 * application_traffic_secret_N+1 = HKDF-Expand-Label(secret_N, "traffic upd",
 * "", Hash.length) and its key and IV, and the next call starts at wire_off +
 * consumed with seq = 0.  For a slot installed from its traffic secret
 * (tlsgpu_sessions_install_secrets) the device does it, behind the open on the
 * same stream and with nothing read back first:
 *   tlsgpu_open_wire -> tlsgpu_wire_key_update_ids -> tlsgpu_sessions_key_update
 * (the host still reads `consumed` and key_update before it builds the next
 * call's streams; it may do so after queuing the rekey).  For a slot installed
 * from a key the caller derives the next secret, key and IV on the host and
 * installs them (tlsgpu_sessions_install, between batches as always).
 * tlsgpu_gather_wire stops at the KeyUpdate record with
 * TLSGPU_READ_NOT_APP_DATA, stop_type 22, stop_len 5.
 * Limits: a KeyUpdate that follows another handshake message inside one record,
 * or one split over two records, is not seen by the peek; such a stream behaves
 * as with the switch off.  There is no second session per stream: the bytes
 * behind the cut are never opened in the same call (under pre-installed next
 * keys a look-alike would destroy the connection).  The engine derives the
 * generations that follow an installed traffic secret and nothing before it
 * (no handshake secrets, no application_traffic_secret_0 from the master
 * secret), and it sends no KeyUpdate by itself: the write side is a
 * tlsgpu_seal_wire stream of type 22 with the 5-byte message, then
 * tlsgpu_sessions_key_update of the write slot on the same stream (or a
 * reinstall of a slot installed from a key). */
#define TLSGPU_WIRE_KU_NONE 0
#define TLSGPU_WIRE_KU_UPDATE 1
#define TLSGPU_WIRE_KU_UPDATE_REQUESTED 2
#define TLSGPU_WIRE_KU_HELD 3
int tlsgpu_sessions_wire_key_update(tlsgpu_sessions *t, int on);

int tlsgpu_open_wire(tlsgpu_sessions *t, const tlsgpu_wire_stream *d_streams,
    uint32_t n_streams, uint8_t *d_wire, uint32_t max_records, tlsgpu_record *d_recs,
    int32_t *d_status, tlsgpu_wire_result *d_results, uint32_t *d_total, void *stream);

/* The id list tlsgpu_sessions_key_update takes, from the results of a
 * tlsgpu_open_wire with the KeyUpdate switch on; asynchronous on `stream`,
 * ordered behind that open.  For each stream i:
 *   d_ids[i] = d_streams[i].session  d_results[i].key_update is
 *                                    TLSGPU_WIRE_KU_UPDATE or _UPDATE_REQUESTED
 *   d_ids[i] = TLSGPU_SESSION_NONE   otherwise (TLSGPU_WIRE_KU_NONE, _HELD)
 * d_ids is a device array of n_streams.  A null argument with n_streams > 0 is
 * TLSGPU_EINVAL; n_streams == 0 is TLSGPU_OK and launches nothing. */
int tlsgpu_wire_key_update_ids(tlsgpu_sessions *t, const tlsgpu_wire_stream *d_streams,
    const tlsgpu_wire_result *d_results, uint32_t n_streams, uint32_t *d_ids, void *stream);

/* ---------------------------------------------------------------------------
 * Wire read path: ssl3_read_bytes (ssl/s3_pkt.c:840-1130) for many connections.
 * tlsgpu_open_wire leaves each delivered record's plaintext where it was opened,
 * with headers, explicit nonces, tags and (TLS 1.3) inner type bytes and padding
 * between one record's plaintext and the next.  tlsgpu_gather_wire hands each
 * stream's application bytes over in order as one contiguous run, and stops
 * where a record is not application data (s3_pkt.c:938, :973-: anything else
 * is the caller's to handle — an alert, a handshake message, change_cipher_spec).
 *
 * Ordered after a tlsgpu_open_wire of the same d_streams, d_recs, d_status,
 * d_results and d_wire; asynchronous on `stream`.  It reads those five and
 * d_reads and writes only d_app and d_read_results: d_wire is never written.
 *
 * Per stream i (d_reads[i] / d_read_results[i] go with d_streams[i]) it walks the
 * records start .. delivered - 1 of the stream's wire result, in order; records
 * at or past `delivered` (the failing one and the TLSGPU_REC_SKIPPED ones) are
 * never looked at, and the caller reads `alert` from the wire result as before.
 *   An application-data record (type 23 in the type bits of its descriptor's
 *   len_type; under TLS 1.3 that is the inner type) is consumed: its `status`
 *   bytes at out_off are appended to the stream's bytes at d_app + app_off.  An
 *   empty one is consumed and contributes nothing (s3_pkt.c:486-488).
 *   Any other type stops the stream with TLSGPU_READ_NOT_APP_DATA; the record
 *   is not consumed and is described by stop_type and stop_len.
 *   A record whose content does not fit the room left stops the stream with
 *   TLSGPU_READ_FULL.  The room is min(app_cap, app_bytes - app_off), 0 when
 *   app_off > app_bytes.  Records are consumed whole: unlike ssl3_read_bytes
 *   (s3_pkt.c:952-960) there is no partial read of a record, and app_cap =
 *   wire_len never meets the limit.
 *   TLSGPU_READ_OUT_OF_BOUNDS: start > delivered or first + delivered >
 *   max_records (nothing is consumed, next = start, consumed = 0), or a record
 *   with a negative status or with [out_off, out_off + status) outside
 *   wire_bytes (the stream stops before it; stop_type and stop_len are 0).
 * Bytes of d_app outside [app_off, app_off + app_len) of each stream are not
 * touched.  To go on after a stop, handle the record `next` and gather again
 * with start = next + 1.
 *
 * TLSGPU_EINVAL before any GPU call: a null argument (d_recs / d_status may be
 * null when max_records is 0), or d_app overlapping [d_wire, d_wire +
 * wire_bytes).  n_streams == 0: TLSGPU_OK, nothing is launched.
 * The TaLoS read hook does not run here (it is per record and may shorten one):
 * callers that register one deliver with tlsgpu_deliver_host. */
#define TLSGPU_READ_END 0		/* every delivered record from `start` on was consumed */
#define TLSGPU_READ_NOT_APP_DATA 1	/* stopped before a delivered record whose type is not 23 */
#define TLSGPU_READ_FULL 2		/* the next record's content does not fit what is left of app_cap */
#define TLSGPU_READ_OUT_OF_BOUNDS 3	/* start > delivered, the stream's record slots leave max_records,
					   or a record's plaintext span leaves wire_bytes: nothing copied
					   from that record on */

typedef struct tlsgpu_read_stream {	/* 16 bytes, one per wire stream, same index */
	uint64_t app_off;	/* the stream's application bytes go to d_app + app_off */
	uint32_t app_cap;	/* room there (SSL_read's len); wire_len always suffices */
	uint32_t start;		/* first record of the stream to look at, index within the stream:
				   0, or `next + 1` of an earlier gather once the caller has dealt
				   with the record that stopped it */
} tlsgpu_read_stream;

typedef struct tlsgpu_read_result {	/* 32 bytes */
	uint32_t app_len;	/* bytes written at app_off */
	uint32_t records;	/* records consumed (application data; empty ones count) */
	uint32_t next;		/* start + records: the record that stopped the stream, == delivered at END */
	uint32_t consumed;	/* wire bytes from the stream's first byte through record next - 1 (0 if next == 0) */
	int32_t stop;		/* TLSGPU_READ_* */
	uint32_t stop_type;	/* NOT_APP_DATA / FULL: that record's content type (TLS 1.3: the inner type) */
	uint32_t stop_len;	/* NOT_APP_DATA / FULL: its plaintext length; it lies at its descriptor's out_off in d_wire */
	uint32_t reserved;
} tlsgpu_read_result;

int tlsgpu_gather_wire(tlsgpu_sessions *t,
    const tlsgpu_wire_stream *d_streams, const tlsgpu_wire_result *d_results, uint32_t n_streams,
    const tlsgpu_record *d_recs, const int32_t *d_status, uint32_t max_records,
    const uint8_t *d_wire, size_t wire_bytes,
    const tlsgpu_read_stream *d_reads, uint8_t *d_app, size_t app_bytes,
    tlsgpu_read_result *d_read_results, void *stream);

/* ---------------------------------------------------------------------------
 * One-call wire read path for TLS 1.2 tables: tlsgpu_open_wire and
 * tlsgpu_gather_wire in one call that moves every application byte once.  Under
 * TLS 1.2 a record's plaintext length (fragment - explicit nonce - tag) and its
 * content type stand in its header, so each record's place in its stream's run
 * at d_app + app_off is known before anything is opened, and the open writes it
 * there, out of place.  The structs and the TLSGPU_READ_* codes are the ones
 * above; `start` must be 0.  Asynchronous on `stream`.
 *
 * The rule, per stream (d_reads[i] / d_read_results[i] go with d_streams[i]):
 * 1. Framing is tlsgpu_open_wire's: the same header checks, slot reservation,
 *    max_records truncation and d_total, all-ones descriptors in unused slots.
 * 2. The plan walks the framed records in order.  For record i: eiv = 8 for the
 *    AES-GCM kinds, 0 for both ChaCha kinds; tag = the session's tag length
 *    (truncated tags count); both 0 for an unknown session;
 *    p_i = max(0, len_i - eiv - tag); T = the sum of p over the records placed so
 *    far (64 bits); room = min(app_cap, app_bytes - app_off), 0 when app_off >
 *    app_bytes.  Tested in this order:
 *      start != 0: TLSGPU_READ_OUT_OF_BOUNDS, the stream is cut to nothing
 *        (records = 0, consumed = 0);
 *      the fragment [in_off, in_off + len_i) is not inside wire_bytes: the stream
 *        is cut before record i with TLSGPU_READ_OUT_OF_BOUNDS, stop_type and
 *        stop_len 0;
 *      the header's type is not 23: cut before record i with
 *        TLSGPU_READ_NOT_APP_DATA, stop_type = the header's type, stop_len = p_i;
 *      T + p_i > room: cut before record i with TLSGPU_READ_FULL, stop_type 23,
 *        stop_len = p_i;
 *      otherwise the record is placed: its descriptor's out_off = app_off + T,
 *        and T += p_i.  An empty record is placed and adds nothing; a fragment
 *        shorter than eiv + tag has p_i = 0, is placed, fails the open with
 *        TLSGPU_REC_PUBLIC_INVALID and ends the stream like any failure.  (With
 *        app_off > app_bytes there is no room, so only empty records are placed:
 *        their out_off is app_bytes, the buffer's end, not a byte outside it.)
 *    stop_type and stop_len of a cut come from the record's UNVERIFIED header:
 *    they say where the batch ends and nothing else, a forged type only shortens
 *    it (as with the KeyUpdate peek above).  The type is part of the AAD, so
 *    whoever opens the record next authenticates it.
 *    A cut before record i is the KeyUpdate cut: the wire result's records,
 *    delivered and alert_record become i, consumed ends with record i - 1's last
 *    byte, a header-level alert that framing found behind the cut is dropped
 *    (alert = 0; the next call finds it again), the descriptors from i on go
 *    back to all ones (d_total still counts them; `first` stays what framing
 *    reported, also for a stream cut to nothing), and not one byte of d_wire
 *    from wire_off + consumed on is read by the open.
 * 3. The open runs over d_recs from d_wire into d_app, bounded by wire_bytes and
 *    app_bytes, with the cipher kernels of tlsgpu_open_batch.
 * 4. The finish is tlsgpu_open_wire's: delivered, alert, alert_record,
 *    TLSGPU_REC_SKIPPED, TLSGPU_REC_OVERFLOW.
 * 5. The read result, with D = delivered: records = next = D; app_len = the sum
 *    of the statuses of records 0 .. D - 1; consumed runs through record D - 1.
 *    If D is below the stream's kept `records` (an AEAD failure or an over-long
 *    plaintext ended it), stop = TLSGPU_READ_END and stop_type = stop_len = 0:
 *    the wire result's alert says why, as ever.  Otherwise stop, stop_type and
 *    stop_len are the plan's (TLSGPU_READ_END when it cut nothing).
 *
 * Memory.  d_wire is never written: a stream can be tried again.  A record that
 * is not application data stays ciphertext at wire_off + consumed.  In d_app,
 * bytes outside every stream's [app_off, app_off + room) are never written;
 * [app_off, app_off + app_len) are the application bytes; from app_off + app_len
 * up to app_off + T the bytes are unspecified (the failing record's zero-fill,
 * the records behind it, an over-long record's plaintext); from app_off + T to
 * the end of the room nothing is written.  To go on after a stop, build a stream
 * at wire_off + consumed with seq + next and give it to tlsgpu_open_wire or to
 * the caller's own record layer.
 *
 * TLSGPU_EINVAL before any GPU call: a null argument (tlsgpu_open_wire's and
 * tlsgpu_gather_wire's rules together), d_app overlapping [d_wire, d_wire +
 * wire_bytes), or a TLS 1.3 table (there the content length and the inner type
 * exist only after the open: use tlsgpu_open_wire + tlsgpu_gather_wire).
 * n_streams == 0 clears d_total and launches nothing more.  The KeyUpdate switch
 * has no part in it (TLS 1.2), and the TaLoS read hook does not run here. */
int tlsgpu_read_wire(tlsgpu_sessions *t,
    const tlsgpu_wire_stream *d_streams, uint32_t n_streams,
    const uint8_t *d_wire, size_t wire_bytes,
    uint32_t max_records, tlsgpu_record *d_recs, int32_t *d_status,
    tlsgpu_wire_result *d_results, uint32_t *d_total,
    const tlsgpu_read_stream *d_reads, uint8_t *d_app, size_t app_bytes,
    tlsgpu_read_result *d_read_results, void *stream);

/* ---------------------------------------------------------------------------
 * Write-side framing: ssl3_write_bytes + do_ssl3_write
 * (ssl/s3_pkt.c:501-557, 560-762) for the AEAD suites, many connections at
 * once.  Each stream is one connection's SSL_write: data_len bytes of
 * application data at d_data + data_off, split into records of at most
 * max_fragment bytes (max_send_fragment, s3_pkt.c:531-536; a zero-length
 * write sends nothing, :593-594), each written to d_wire as the 5-byte header
 * (type, version, length = explicit nonce + ciphertext + tag, :662-677, :733)
 * followed by tls1_enc(s, 1)'s fragment (explicit nonce = sequence number for
 * GCM, t1_enc.c:887-914), back to back from d_wire + wire_off.  Sequence
 * numbers run seq, seq + 1, ... (t1_enc.c:258-266).  The sealed records also
 * get descriptors in d_recs (slots reserved per stream, like tlsgpu_open_wire;
 * streams that do not fit max_records are cut at a record boundary) and a
 * status each (explicit nonce + fragment + tag bytes for a sealed record).
 * d_total receives the number of record slots the streams asked for, each
 * stream's count first capped at max_records: it may exceed max_records, and
 * then min(d_total, max_records) descriptors were written.  The ranges are
 * handed out in no fixed order once the call has more than 64 streams; a
 * stream without records (data_len 0, an unknown or never-installed session,
 * or cut to nothing: then not a byte of it is written, wire_len is 0 and
 * next_seq is seq) reports first = 0.  Slots no stream got hold all-ones
 * descriptors and the status TLSGPU_REC_PUBLIC_INVALID.
 * data_bytes / wire_bytes bound the buffers, per record: a record's header is
 * written iff header and fragment lie inside wire_bytes; its fragment is
 * written iff they do and its plaintext lies inside data_bytes, otherwise the
 * record's status is TLSGPU_REC_OUT_OF_BOUNDS and not a byte of the fragment
 * changes.  `records`, wire_len and next_seq count such a record all the same,
 * so the stream's later records keep their places.  Offsets are 64-bit and do
 * not wrap: a descriptor offset that would pass 2^64 - 1 stays there (outside
 * every buffer).  tlsgpu_seal_wire_size gives a stream's wire bytes.
 * Asynchronous.
 * A TLS 1.3 session of any kind: each fragment (<= max_fragment <= 16384) goes out as the
 * header 17 03 03 BE16(inner + 16) and ciphertext(content || type || zeros) ||
 * tag, inner = the fragment's padded inner plaintext under the session's
 * pad_block (len + 1 without one), with stream.type as the inner type;
 * next_seq and wire_len follow that framing (tlsgpu_seal_wire_size_p). */
typedef struct tlsgpu_write_stream {
	uint64_t data_off;	/* application data at d_data + data_off */
	uint64_t wire_off;	/* the stream's records go to d_wire + wire_off */
	uint64_t seq;		/* write sequence number of the first record */
	uint32_t data_len;	/* bytes to send (ssl3_write_bytes' len) */
	uint32_t session;	/* write-direction session id */
	uint16_t version;	/* s->version, e.g. 0x0303 */
	uint8_t type;		/* content type, 23 = application data */
	uint8_t reserved;
	uint32_t max_fragment;	/* s->max_send_fragment; 0 = 16384 */
} tlsgpu_write_stream;

typedef struct tlsgpu_write_result {
	uint32_t first;		/* index of the stream's first record in d_recs / d_status; 0 if none */
	uint32_t records;	/* records written */
	uint64_t wire_len;	/* bytes written from wire_off (headers + fragments) */
	uint64_t next_seq;	/* the write sequence number after the last record */
	uint64_t reserved;
} tlsgpu_write_result;

int tlsgpu_seal_wire(tlsgpu_sessions *t, const tlsgpu_write_stream *d_streams,
    uint32_t n_streams, const uint8_t *d_data, size_t data_bytes, uint8_t *d_wire,
    size_t wire_bytes, uint32_t max_records, tlsgpu_record *d_recs, int32_t *d_status,
    tlsgpu_write_result *d_results, uint32_t *d_total, void *stream);
/* Wire bytes of one stream: ceil(len / frag) records of 5 + explicit nonce
 * (8 for GCM, 0 for ChaCha) + fragment + tag_len bytes (0 when len == 0).
 * TLSGPU_CHACHA20_POLY1305_TLS13 exists in TLS 1.3 only, so it gets the TLS 1.3
 * framing of tlsgpu_seal_wire_size_v here too. */
uint64_t tlsgpu_seal_wire_size(int aead, uint32_t data_len, uint32_t max_fragment,
    uint32_t tag_len);
/* The same for a session of `version`: 0x0304 with an AES-GCM kind, and
 * TLSGPU_CHACHA20_POLY1305_TLS13 with any version, is TLS 1.3 framing,
 * ceil(len / frag) records of 5 + fragment + 1 (inner type) + 16; anything
 * else is tlsgpu_seal_wire_size (TLSGPU_CHACHA20_POLY1305 with 0x0304, which
 * no install accepts, keeps the TLS 1.2 arithmetic). */
uint64_t tlsgpu_seal_wire_size_v(int aead, uint16_t version, uint32_t data_len,
    uint32_t max_fragment, uint32_t tag_len);
/* The same for a session installed with `pad_block`: under TLS 1.3 framing each
 * record is 5 + inner + 16 with the fragment's padded inner plaintext length.
 * Equal to tlsgpu_seal_wire_size_v for pad_block <= 1 and for any session that
 * is not TLS 1.3 (pad_block is ignored there, as at install). */
uint64_t tlsgpu_seal_wire_size_p(int aead, uint16_t version, uint32_t data_len,
    uint32_t max_fragment, uint32_t tag_len, uint32_t pad_block);

/* GCM TLS batch kernel selection (process-wide; results are identical).
 * TLSGPU_GCM_AUTO (default): TLSGPU_GCM_SPLIT for batches of at most two
 * records per CU of the device, TLSGPU_GCM_QUEUE for larger ones.
 * TLSGPU_GCM_SPLIT: one record per 16-wave workgroup, the record's blocks split
 * over the waves (latency: a 16 KiB record in ~20 us instead of one wave's
 * serial pass).
 * TLSGPU_GCM_QUEUE: a prep pass computes every record's E_K(J0) and
 * round-1/2 constants, then 16 T-table waves per CU (AES rounds as LDS
 * lookups) pull records from a per-session-run queue.  Records of <= 62
 * blocks share a wave in packs (environment TLSGPU_PACK=0 turns packs off).
 * TLSGPU_GCM_TTABLE: T-table waves with in-kernel constants, static split.
 * TLSGPU_GCM_HYBRID: 4 bitsliced waves (AES-CTR on the VALU, pairs of
 * 16-byte-aligned records of >= 16 KiB) beside 4 T-table waves per CU.
 * TLSGPU_GCM_BITSLICE: 8 bitsliced waves per CU.
 * TLSGPU_GCM_FUSED: 8 waves per CU, each running a bitsliced record pair with
 * a T-table record interleaved into its AES rounds.
 * The environment variable TLSGPU_GCM_IMPL=auto|split|queue|ttable|hybrid|bitslice|fused
 * sets the initial value.  The per-call EVP path always uses the split kernel
 * on its raw jobs. */
enum tlsgpu_gcm_impl {
  TLSGPU_GCM_BITSLICE = 0, TLSGPU_GCM_TTABLE = 1, TLSGPU_GCM_HYBRID = 2, TLSGPU_GCM_QUEUE = 3,
  TLSGPU_GCM_FUSED = 4, TLSGPU_GCM_SPLIT = 5, TLSGPU_GCM_AUTO = 6
};
int tlsgpu_set_gcm_impl(int impl);
int tlsgpu_get_gcm_impl(void);

/* EVP coalescing queue.  Turns on batching for the per-call
 * EVP_AEAD_* drop-in: contexts initialised afterwards take a slot of one shared
 * device session pool (pool_sessions, default 1024; contexts beyond it keep a
 * private table and the per-call path), and their seal/open calls are queued;
 * a dispatcher thread runs everything that arrives within window_us (or
 * max_jobs, default 4096) as one raw batch per direction and wakes the callers.
 * Outputs, return values and zero-fill are those of the per-call path.  Calling
 * it again adjusts window_us / max_jobs.  The environment variables
 * TLSGPU_EVP_BATCH_US / TLSGPU_EVP_POOL do the same at library load.
 * tlsgpu_evp_batch_stats: batches run and jobs served so far. */
int tlsgpu_evp_set_batching(unsigned window_us, unsigned max_jobs, unsigned pool_sessions);
int tlsgpu_evp_batch_stats(uint64_t *batches, uint64_t *jobs);
/* EVP_AEAD_CTX_seal / _open calls whose cipher work ran on the GPU (per-call
 * or queued; authentication failures included, argument-check rejections
 * not), process-wide since load.  Lets a caller that interposed the library
 * under an unchanged libssl check that every TLS record went through it. */
int tlsgpu_evp_call_stats(uint64_t *seal_calls, uint64_t *open_calls);
/* Doorbell server for per-call EVP calls (round 4).  groups > 0 keeps up to
 * that many 1024-thread server workgroups (one CU each, one per calling thread)
 * resident on every EVP device while calls arrive: a calling thread posts its
 * job (the same zero-copy RawJob the launched path builds) in a slot of pinned
 * host memory and spins on the answer, so a synchronous EVP_AEAD_CTX_seal /
 * _open on an AES-GCM, RFC 7539 or draft ChaCha20-Poly1305 context costs one
 * PCIe round trip instead of a kernel launch + stream sync.  Each server
 * instance exits after lifetime_ms (0 = 5 ms) and is relaunched by the next
 * call, so an idle process leaves nothing running.  Threads beyond
 * 8 * groups per device and pooled (queued) contexts use the other paths.
 * Same as
 * TLSGPU_EVP_DOORBELL=<groups> (TLSGPU_EVP_DOORBELL_MS=<lifetime>) at load;
 * on by default with 64 groups (round 5; 0 turns it off); must be called
 * before the first EVP call.  With it on, EVP_AEAD_CTX_init launches nothing
 * (the session image is built on the host and installed by the context's
 * first call) and EVP_AEAD_CTX_cleanup scrubs the slot through the server.
 * tlsgpu_evp_doorbell_stats: jobs served and instances launched so far.
 * tlsgpu_evp_doorbell_scrub_stats (round 6): scrub jobs served, and times a
 * server workgroup other than the scrubbing one zeroed its LDS copy of a
 * scrubbed key (the scrub ring). */
int tlsgpu_evp_set_doorbell(unsigned groups, unsigned lifetime_ms);
int tlsgpu_evp_doorbell_stats(uint64_t *jobs, uint64_t *launches);
int tlsgpu_evp_doorbell_scrub_stats(uint64_t *scrubs, uint64_t *flushes);
/* tlsgpu_evp_doorbell_warm: launch a server instance now on every EVP device
 * whose queued instance would stop polling within half a lifetime (what the
 * next call would do), e.g. before a burst of calls.  No-op with the doorbell
 * off or after shutdown.
 * tlsgpu_evp_shutdown: the doorbell's shutdown contract.  Stops every server,
 * then waits until every instance ever launched — running or still queued
 * behind other work — has left, reading pinned memory only (no HIP call);
 * later EVP calls take the launched path.  TLSGPU_ETIMEOUT if an instance is
 * still running after TLSGPU_EVP_SHUTDOWN_MS (default 60 s).  Idempotent.
 * The library runs it itself first thing at process exit (the main thread's
 * thread-local destructors run before the HIP runtime's exit-time teardown),
 * from an atexit handler and from its destructor; an application that tears
 * the runtime down itself (hipDeviceReset) calls it before. */
int tlsgpu_evp_doorbell_warm(void);
/* Test support: the device image of one session as EVP_AEAD_CTX_init builds it
 * on the host (DevSession, 1 KiB, then the GCM tables: basis, Shoup tables of
 * H^1..H^65, bitsliced masks; zero for ChaCha) into out[0..n), n >= 27,392.
 * tests/test_session_image.py checks it against the device install kernel. */
int tlsgpu_session_image(const tlsgpu_session_params *p, uint8_t *out, size_t n);
int tlsgpu_evp_shutdown(void);
/* Test support.  tlsgpu_evp_context_slot: the session table and slot that hold
 * a live EVP context's device key material.  tlsgpu_sessions_debug_read: after
 * every queued install / scrub of `slot` has finished, copy its first n bytes
 * (DevSession, then the GCM tables) to host memory — EVP_AEAD_CTX_cleanup
 * scrubs the slot asynchronously, and this shows the scrub happened.  (The key
 * also travels to the install kernel as a kernel argument, in the HIP
 * runtime's argument buffer, which later launches overwrite but nothing
 * zeroes: DESIGN.md §4.7.) */
struct evp_aead_ctx_st; /* EVP_AEAD_CTX, include/tlsgpu_evp.h */
int tlsgpu_evp_context_slot(const struct evp_aead_ctx_st *ctx, tlsgpu_sessions **sessions,
    uint32_t *slot);
int tlsgpu_sessions_debug_read(tlsgpu_sessions *t, uint32_t slot, uint8_t *out, size_t n);
/* The EVP surface's GPUs.  TLSGPU_DEVICES=a,b,... (a device may repeat: two
 * engines on one GPU) or TLSGPU_DEVICE=d pin them; by default every visible
 * GPU.  EVP_AEAD_CTX_init gives new contexts (and EVP_CIPHER contexts their
 * first key) to these devices in turn; each device has its own engine, call
 * streams and, with batching on, its own coalescing queue and session pool
 * (pool_sessions each).  tlsgpu_evp_device_stats(k, ...): device ordinal,
 * contexts created and EVP calls run on the k-th of them. */
uint32_t tlsgpu_evp_device_count(void);
int tlsgpu_evp_device_stats(uint32_t k, int *device, uint64_t *contexts, uint64_t *calls);
/* GPU programs run by the EVP_aes_{128,256}_gcm EVP_CIPHER objects
 * (include/tlsgpu_evp.h), process-wide since load. */
int tlsgpu_evp_cipher_stats(uint64_t *programs);

/* Diagnostic: hybrid-kernel phase timing.  With TLSGPU_PHASE_STATS=1 in the
 * environment, the first call allocates 32 device counters (shader cycles and
 * event counts per phase, summed over waves) that later hybrid launches fill;
 * each call synchronizes the device, copies them to out32 (may be NULL) and
 * optionally resets them.  Fails when the variable is not set. */
int tlsgpu_debug_phase_stats(tlsgpu_engine *e, unsigned long long *out32, int reset);

/* Diagnostic: per-workgroup timing of the queue kernel.  With
 * TLSGPU_WG_TIMES=1 in the environment every queue launch writes, per
 * workgroup g, out[4g..4g+3] = {start, end (100 MHz s_memrealtime ticks),
 * records, work (payload bytes + 256 per record)} of the records it ran; this
 * call synchronizes the device and copies the first `groups` (<= 1024)
 * entries of the last launch.  Fails when the
 * variable is not set or before the first launch. */
int tlsgpu_debug_wg_times(tlsgpu_engine *e, unsigned long long *out, unsigned groups);

/* Diagnostic: ECB-encrypt nblocks 16-byte blocks (device memory) under the
 * AES key of GCM session `session` with the bitsliced AES core. */
int tlsgpu_aes_ecb_bitsliced(tlsgpu_sessions *t, uint32_t session, const uint8_t *d_in,
    uint8_t *d_out, uint32_t nblocks, void *stream);

/* Deterministic synthetic bytes, counter-based SplitMix64 keyed by
 * (seed, index0 + i) for each of n spans of span_len bytes at d_out + i*stride
 * (same stream as the oracle's oracle_fill_bytes; used by bench/tests). */
int tlsgpu_fill_synthetic(tlsgpu_engine *e, uint8_t *d_out, uint64_t stride,
    uint32_t span_len, uint32_t n, uint64_t seed, uint64_t index0, void *stream);
/* The same stream for n variable-length spans in one launch: span i covers
 * d_lengths[i] bytes at d_out + d_offsets[i] (device arrays) and is keyed
 * (seed, index0 + i). */
int tlsgpu_fill_synthetic_spans(tlsgpu_engine *e, uint8_t *d_out, const uint64_t *d_offsets,
    const uint32_t *d_lengths, uint32_t n, uint64_t seed, uint64_t index0, void *stream);

/* Device / pinned-host memory, copies and events on the engine's device, so
 * callers need no other GPU runtime (the bench and tests use only these). */
int tlsgpu_malloc(tlsgpu_engine *e, size_t bytes, void **d_ptr);
int tlsgpu_free(tlsgpu_engine *e, void *d_ptr);
int tlsgpu_host_alloc(tlsgpu_engine *e, size_t bytes, void **h_ptr);	/* pinned */
int tlsgpu_host_free(tlsgpu_engine *e, void *h_ptr);
/* Async copy in any direction (hipMemcpyDefault) on `stream` (NULL = engine). */
int tlsgpu_memcpy(tlsgpu_engine *e, void *dst, const void *src, size_t bytes, void *stream);
int tlsgpu_memset(tlsgpu_engine *e, void *d_ptr, int value, size_t bytes, void *stream);
int tlsgpu_stream_create(tlsgpu_engine *e, void **stream);
int tlsgpu_stream_destroy(tlsgpu_engine *e, void *stream);
int tlsgpu_stream_sync(tlsgpu_engine *e, void *stream);
int tlsgpu_event_create(tlsgpu_engine *e, void **event);
int tlsgpu_event_destroy(tlsgpu_engine *e, void *event);
int tlsgpu_event_record(tlsgpu_engine *e, void *event, void *stream);
/* Milliseconds between two recorded events (waits for `end`). */
int tlsgpu_event_elapsed_ms(tlsgpu_engine *e, void *start, void *end, float *ms);

/* Human-readable last error of this thread. */
const char *tlsgpu_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
