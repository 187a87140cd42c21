/*
 * uvhttp_tls_amd.h — batched TLS record open (AES-GCM, ChaCha20-Poly1305) on MI355X, ahead of
 * the WebSocket decoder.
 *
 * What it replaces.  For a TLS connection the reference's WebSocket read callback decrypts
 * with mbedtls before framing: on_websocket_read (src/uvhttp_connection.c:1122-1159) calls
 * mbedtls_ssl_read into read_buffer until WANT_READ, hands every decrypted chunk to
 * uvhttp_ws_process_data (:1152-1153), closes the WebSocket on PEER_CLOSE_NOTIFY (:1136-1138)
 * and on any other negative return (:1139-1144).  mbedtls (an un-vendored submodule,
 * .gitmodules; absent here) opens each record with the negotiated AEAD — for the TLS 1.2/1.3
 * AEAD suites, AES-128/256-GCM (NIST SP 800-38D, RFC 5288) and ChaCha20-Poly1305 (RFC 8439,
 * RFC 7905), TLS 1.3 (RFC 8446 §5.2-5.3) and TLS 1.2.  This surface
 * opens the application-data records of many connections in one device call and leaves each
 * connection's plaintext contiguous in device memory, where uvhttp_ws_gpu_decode_streams
 * (include/uvhttp_ws_amd.h) takes it as its wire stream.
 *
 * Division of labour with mbedtls.  The handshake, alerts, post-handshake handshake messages
 * (KeyUpdate, NewSessionTicket) and renegotiation stay in mbedtls on the host.  The device
 * opens records while they are authenticated application data and stops a connection at the
 * first record that is not (status UVHTTP_TLS_REC_CONTROL, or an error): the host advances
 * mbedtls's read sequence number by n_delivered and feeds it the remaining ciphertext from
 * consumed_bytes on.  Keys come from the host (mbedtls's key-export callback:
 * TLS 1.3 traffic secret -> HKDF-Expand-Label key/iv, TLS 1.2 key block), one slot per
 * connection direction.
 *
 * Batch contract (the parity contract, restated by oracle/tls_oracle.c).  Connection s owns
 * the ciphertext bytes wire[begin, begin + len).  Records are walked from begin (5-byte header:
 * type, version, big-endian length).  The walk stops
 *   - with fewer than 5 bytes left, or fewer than 5 + length (incomplete: not an error, the
 *     bytes wait for the next read, like MBEDTLS_ERR_SSL_WANT_READ);
 *   - at a record whose header fails a check, in this order (the record is counted, with its
 *     status): version != 0x0303 (ERR_VERSION); type not application_data (TLS 1.3) / not
 *     alert, handshake or application_data (TLS 1.2) (ERR_BAD_TYPE); length over the limit
 *     (ERR_OVERFLOW: 2^14 content bytes (+ 1 inner type byte for TLS 1.3) + the AEAD
 *     overhead); length below the AEAD overhead (ERR_BAD_MAC).  The overhead is the 16-byte
 *     tag, plus the 8-byte explicit nonce of TLS 1.2 AES-GCM.
 * Counted record k of connection s is opened with sequence number seq + k.  Nonce: iv XOR
 * (0^32 || be64(seq)) for TLS 1.3 and for TLS 1.2 ChaCha20-Poly1305 (RFC 7905); iv[0..3] ||
 * the 8 explicit-nonce bytes after the header for TLS 1.2 AES-GCM (RFC 5288).  AAD: the 5
 * header bytes (TLS 1.3); be64(seq) || type || 0x03 0x03 || be16(plaintext length) (TLS 1.2).
 * TLS 1.3 inner plaintext = content || type || zero padding (type = last non-zero byte; none
 * = ERR_EMPTY).  A record is delivered if it authenticates (else
 * ERR_BAD_MAC) and its (inner) type is application_data (23), else it is CONTROL.  The first
 * record not delivered stops the connection; the records after it are SKIPPED.
 *
 * Output.  Connection s's delivered content is contiguous at out[out_off, out_off + plain_len)
 * in record order.  out_off is the connection's base in a layout where every counted record
 * reserves its largest possible content (length - overhead, - 1 more for TLS 1.3, never
 * below 0), connections in index order from 0; out_cap >= the total wire bytes of the
 * connections always suffices.  Bytes of out outside the delivered ranges are unspecified
 * and MAY HOLD UNAUTHENTICATED PLAINTEXT: records are decrypted in parallel, so a record whose
 * tag fails, and records after a connection's first undelivered record, may have had their
 * plaintext written to their reservation before the verdict.  Read only
 * [out_off, out_off + plain_len) of a connection (and the records' [out_off, + content_len)).
 * The ciphertext in wire is not modified.
 *
 * A connection's reservation is ws_prefix bytes followed by its records' reservations; its
 * plaintext starts at out_off = reservation start + ws_prefix.
 */
#ifndef UVHTTP_TLS_AMD_H
#define UVHTTP_TLS_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UVHTTP_TLS_VERSION_12 0x0303u
#define UVHTTP_TLS_VERSION_13 0x0304u
#define UVHTTP_TLS_CONTENT_ALERT 21u
#define UVHTTP_TLS_CONTENT_HANDSHAKE 22u
#define UVHTTP_TLS_CONTENT_APPLICATION_DATA 23u

/* Return codes (same values as the WebSocket device surface). */
#define UVHTTP_TLS_GPU_OK 0
#define UVHTTP_TLS_GPU_EINVAL (-1)
#define UVHTTP_TLS_GPU_ENODEV (-2)
#define UVHTTP_TLS_GPU_ENOMEM (-3)
#define UVHTTP_TLS_GPU_ELAUNCH (-4)

/* Per-record status. */
#define UVHTTP_TLS_REC_OK 0               /* authenticated application data, delivered */
#define UVHTTP_TLS_REC_SKIPPED 2          /* after the connection's first undelivered record */
#define UVHTTP_TLS_REC_CONTROL 3          /* authenticated alert / handshake: host (mbedtls) */
#define UVHTTP_TLS_REC_ERR_OVERFLOW (-1)  /* record_overflow (RFC 8446 §5.2, RFC 5246 §6.2.3) */
#define UVHTTP_TLS_REC_ERR_BAD_MAC (-2)   /* tag mismatch, or too short for nonce + tag */
#define UVHTTP_TLS_REC_ERR_BAD_TYPE (-3)  /* outer content type not allowed */
#define UVHTTP_TLS_REC_ERR_VERSION (-4)   /* legacy_record_version != 0x0303 */
#define UVHTTP_TLS_REC_ERR_EMPTY (-5)     /* TLS 1.3 inner plaintext has no content type */
#define UVHTTP_TLS_REC_ERR_CAPACITY (-6)  /* records / layout exceed records[] or out_cap */
#define UVHTTP_TLS_REC_ERR_KEY (-7)       /* key slot out of range, or key_len / version / cipher invalid
                                             (connection result only; no record counted) */
#define UVHTTP_TLS_REC_ERR_RANGE (-8)     /* a send's frames lie outside frame_off[] / frames[] */

/* AEAD of a key slot (uvhttp_tls_key_t.cipher). */
#define UVHTTP_TLS_CIPHER_AES_GCM 0u            /* AES-128/256-GCM (key_len 16 / 32) */
#define UVHTTP_TLS_CIPHER_CHACHA20_POLY1305 1u  /* RFC 8439 (key_len 32) */

/* Keys of one connection direction (64 bytes). */
typedef struct {
    uint8_t key[32];   /* key_len bytes used */
    uint8_t iv[12];    /* TLS 1.3 and TLS 1.2 ChaCha20-Poly1305: the write iv (nonce = iv XOR
                          seq); TLS 1.2 AES-GCM: salt = iv[0..3], rest ignored */
    uint32_t key_len;  /* 16 or 32 (AES-GCM), 32 (ChaCha20-Poly1305) */
    uint32_t version;  /* UVHTTP_TLS_VERSION_12 or UVHTTP_TLS_VERSION_13 */
    uint32_t cipher;   /* UVHTTP_TLS_CIPHER_* (0 = AES-GCM) */
    uint32_t reserved[2];
} uvhttp_tls_key_t;

/* One connection's buffered ciphertext (32 bytes). */
typedef struct {
    uint64_t begin;     /* offset in wire */
    uint64_t len;       /* bytes */
    uint64_t seq;       /* read sequence number of the first record */
    uint32_t key;       /* key slot */
    uint32_t ws_prefix; /* bytes reserved in out directly before the plaintext (out_off -
                           ws_prefix ...): room for what the connection's WebSocket decoder
                           already buffers (recv_buffer[0, recv_buffer_pos)), so the decoded
                           stream is contiguous; 0 = none */
} uvhttp_tls_stream_t;

/* One counted record (device-written, 32 bytes). */
typedef struct {
    uint64_t rec_off;      /* record start (header) in wire */
    uint64_t out_off;      /* delivered content start in out (0 if not delivered) */
    uint32_t content_len;  /* content bytes (0 unless opened) */
    uint32_t stream;       /* connection index */
    uint8_t type;          /* inner (TLS 1.3) / outer (TLS 1.2) content type once opened */
    int8_t status;         /* UVHTTP_TLS_REC_* */
    uint16_t reserved;
    uint32_t reserved2;
} uvhttp_tls_record_t;

/* One connection's result (device-written, 64 bytes). */
typedef struct {
    uint32_t first_record;    /* index of its first record in records[] */
    uint32_t n_records;       /* counted records */
    uint32_t n_delivered;     /* records delivered before the first stop */
    int32_t status;           /* 0, or -1 if the stop is an error (the reference closes) */
    int32_t first_status;     /* status of record n_delivered (0 if all delivered) */
    uint32_t reserved;
    uint64_t consumed_bytes;  /* ciphertext bytes of the delivered records */
    uint64_t next_seq;        /* seq + n_delivered */
    uint64_t out_off;         /* base of the connection's plaintext in out */
    uint64_t plain_len;       /* delivered content bytes */
    uint64_t reserved3;
} uvhttp_tls_result_t;

/* One record to seal (32 bytes). */
typedef struct {
    uint64_t src_off;    /* plaintext content in src */
    uint64_t out_off;    /* record start in out */
    uint64_t seq;        /* write sequence number */
    uint32_t plain_len;  /* content bytes, <= 2^14 */
    uint16_t key;        /* key slot */
    uint8_t type;        /* content type */
    uint8_t reserved;
} uvhttp_tls_seal_t;

/* One send: frames [first_frame, first_frame + n_frames) of a build_frames output, to one
 * connection direction (32 bytes). */
typedef struct {
    uint64_t seq;          /* write sequence number of the send's first record */
    uint32_t first_frame;
    uint32_t n_frames;
    uint32_t key;          /* key slot */
    uint8_t type;          /* content type (23) */
    uint8_t reserved[3];
    uint64_t reserved2;
} uvhttp_tls_send_t;

/* One send's result (device-written, 48 bytes). */
typedef struct {
    uint64_t out_off;       /* start of the send's records in out */
    uint64_t out_len;       /* bytes of its records: what one uv_write sends */
    uint64_t next_seq;      /* seq + n_records */
    uint32_t first_record;  /* index in records[] */
    uint32_t n_records;
    int32_t status;         /* 0, UVHTTP_TLS_REC_ERR_KEY / _RANGE / _CAPACITY */
    uint32_t reserved;
    uint64_t plain_len;     /* frame bytes sealed */
} uvhttp_tls_send_result_t;

/* Totals of one seal_frames call (device-written, 32 bytes). */
typedef struct {
    uint64_t out_bytes;  /* bytes of out the call needs */
    uint32_t n_records;  /* records the call needs (saturates at 2^32 - 1) */
    uint32_t n_failed;   /* sends whose status is not 0 */
    uint64_t reserved[2];
} uvhttp_tls_send_summary_t;

#ifdef __cplusplus
static_assert(sizeof(uvhttp_tls_send_t) == 32 && sizeof(uvhttp_tls_send_result_t) == 48 &&
              sizeof(uvhttp_tls_send_summary_t) == 32, "send-side struct sizes");
#else
_Static_assert(sizeof(uvhttp_tls_send_t) == 32 && sizeof(uvhttp_tls_send_result_t) == 48 &&
               sizeof(uvhttp_tls_send_summary_t) == 32, "send-side struct sizes");
#endif

typedef struct uvhttp_tls_gpu_engine uvhttp_tls_gpu_engine_t;

/* UVHTTP_TLS_GPU_ENODEV without a gfx950 device (there is no CPU fallback). */
int uvhttp_tls_gpu_engine_create(int device, uvhttp_tls_gpu_engine_t** out);
void uvhttp_tls_gpu_engine_free(uvhttp_tls_gpu_engine_t* eng);
const char* uvhttp_tls_gpu_engine_last_error(const uvhttp_tls_gpu_engine_t* eng);
/* HIP-event time of the record-crypto kernel over the calls since the last read. */
int uvhttp_tls_gpu_engine_set_timing(uvhttp_tls_gpu_engine_t* eng, int enable);
int uvhttp_tls_gpu_engine_kernel_time(uvhttp_tls_gpu_engine_t* eng, double* ms,
                                      uint64_t* launches);

/* Open the records of n_streams connections.  Device pointers: wire[wire_len], keys[n_keys],
 * streams[n_streams], records[max_records], results[n_streams], out[out_cap].  Asynchronous
 * on `stream` (a hipStream_t; NULL = default stream).  If the records do not fit records[] or
 * the layout does not fit out, every connection reports UVHTTP_TLS_REC_ERR_CAPACITY and
 * nothing is delivered. */
int uvhttp_tls_gpu_open_records(uvhttp_tls_gpu_engine_t* eng, const uint8_t* wire,
                                uint64_t wire_len, const uvhttp_tls_key_t* keys, uint32_t n_keys,
                                const uvhttp_tls_stream_t* streams, uint32_t n_streams,
                                uvhttp_tls_record_t* records, uint32_t max_records,
                                uvhttp_tls_result_t* results, uint8_t* out, uint64_t out_cap,
                                void* stream);

/* Seal records (the send side, and the bench's input generator).  Record i: header (type 23
 * for TLS 1.3, `type` for TLS 1.2), TLS 1.2 AES-GCM explicit nonce = be64(seq), ciphertext, tag; the
 * TLS 1.3 inner plaintext is content || type with no padding.  Device pointers throughout;
 * records must not overlap src, with one exception: src = out and src_off = out_off + 5 (+ 8 for
 * the explicit nonce of TLS 1.2 AES-GCM) for every record seals in place, the content lying where
 * its ciphertext will (uvhttp_tls_gpu_seal_parts_coalesced rests on this). */
/* The TLS -> WebSocket hand-off on the device.  For every connection s: the ws_prefix bytes
 * at prefix_src[prefix_off[s]] (its recv_buffer[0, recv_buffer_pos), staged by the caller;
 * prefix_src may be NULL when every ws_prefix is 0) are copied to out[out_off - ws_prefix,
 * out_off), and ws_streams[s] (the caller filled the connection state with
 * uvhttp_ws_stream_init) gets begin = out_off - ws_prefix, len = ws_prefix + plain_len and
 * one process_data call per delivered record:
 * first_read = first_record, n_reads = n_delivered, read_end[first_record + k] = ws_prefix +
 * the content of records 0..k — exactly the chunks on_websocket_read hands to process_data,
 * one per mbedtls_ssl_read (src/uvhttp_connection.c:1128-1159; a read returns one record's
 * content when read_buffer_size >= 16384, the reference default).  read_end has max_records
 * entries.  Connections whose result is ERR_CAPACITY or ERR_KEY must not be decoded. */
int uvhttp_tls_gpu_ws_streams(uvhttp_tls_gpu_engine_t* eng, const uvhttp_tls_result_t* results,
                              const uvhttp_tls_record_t* records, uint32_t n_streams,
                              const uvhttp_tls_stream_t* streams, const uint8_t* prefix_src,
                              const uint64_t* prefix_off, uint8_t* out, void* ws_streams,
                              uint64_t* read_end, void* stream);

int uvhttp_tls_gpu_seal_records(uvhttp_tls_gpu_engine_t* eng, const uint8_t* src,
                                uint64_t src_len, const uvhttp_tls_seal_t* recs,
                                uint32_t n_records, const uvhttp_tls_key_t* keys,
                                uint32_t n_keys, uint8_t* out, uint64_t out_cap, void* stream);

/* Seal built WebSocket frames into the TLS records of many connections: the hand-off
 * uvhttp_ws_gpu_build_frames -> sealed records, the mirror of uvhttp_tls_gpu_ws_streams.  What it
 * replaces: on a TLS connection uvhttp_ws_send_frame (src/uvhttp_websocket.c:543-575) hands every
 * built frame to mbedtls_ssl_write in a loop, one record of at most 16 384 content bytes per
 * call.  Here `frames` / `frame_off` are build_frames' d_out / d_out_off (n_frames_total + 1
 * offsets) as they lie on the device, and a send names a run of those frames, a key slot and the
 * write sequence number of its first record; the record plan is made on the device, so nothing
 * is read back between the two calls.  All pointers are device pointers; the call is
 * asynchronous on `stream` and does not synchronise with the host.
 *
 * Cutting.  Frame f has F = frame_off[f + 1] - frame_off[f] bytes and is cut on its own, as the
 * mbedtls_ssl_write loop cuts it: ceil(F / max_fragment) records, every one of max_fragment
 * content bytes except the last; a record never holds bytes of two frames; F = 0 gives no
 * record.  max_fragment is 1..16384 (0 = 16384).
 *
 * Numbering and layout.  A send's records are numbered seq, seq + 1, ... across its frames in
 * order.  Records lie back to back in out, sends in index order and a send's records in order,
 * so out[out_off, out_off + out_len) of a send is one contiguous write.  The bytes of a record
 * are exactly uvhttp_tls_gpu_seal_records' for the same (key, seq, type, content).  records[]
 * receives one uvhttp_tls_seal_t per record (src_off into frames, out_off, seq, plain_len, key,
 * type), send s's at [first_record, first_record + n_records); after the call it is a valid
 * input to uvhttp_tls_gpu_seal_records (src = frames).
 *
 * Broadcast.  Sends may name the same or overlapping frame ranges: one built frame, N sends with
 * N keys.  Sends are independent; two sends with the same key slot get the sequence numbers the
 * caller gave them.
 *
 * Per-send failures (status set, 0 records, out_len 0, next_seq = seq; the other sends are not
 * affected), checked in this order:
 *   ERR_KEY    the key slot is >= n_keys, the slot's key is invalid, or the slot is above 65 535
 *              (uvhttp_tls_seal_t carries a 16-bit slot);
 *   ERR_RANGE  first_frame + n_frames > n_frames_total, or a frame of the send has frame_off[f] >
 *              frame_off[f + 1] or frame_off[f + 1] > frames_len.  With frames_len = the out_cap
 *              build_frames was given, this also catches every send that reaches into what a
 *              build_frames wrote nothing of because that out_cap was too small.
 * A failed send's out_off and first_record are where its records would have begun.  A send with
 * n_frames = 0 (and first_frame <= n_frames_total) succeeds with no record.
 *
 * Capacity.  If the records of the sends without an error of their own exceed max_records, or
 * their bytes exceed out_cap, every such send reports ERR_CAPACITY, every result has out_off,
 * out_len, first_record, n_records and plain_len 0, nothing is written to out or records, and
 * summary still holds the totals needed, so the caller can size and call again.  n_failed is
 * then n_sends.
 *
 * Returns EINVAL for a null pointer with a non-zero count (summary is always required), for
 * max_fragment > 16384, and for more than 2^26 sends, 2^28 frames or 2^28 records; ENODEV
 * for a null engine where there is no device.  n_sends = 0 returns OK with a zeroed summary.
 * The call is the one-part case of uvhttp_tls_gpu_seal_parts and is planned as such: one part of
 * base 0 and len frames_len whose runs points at &sends[0].first_frame with run_stride = 32
 * (sizeof(uvhttp_tls_send_t)) expresses it; only the argument checks above are its own. */
int uvhttp_tls_gpu_seal_frames(uvhttp_tls_gpu_engine_t* eng, const uint8_t* frames,
                               uint64_t frames_len, const uint64_t* frame_off,
                               uint32_t n_frames_total, const uvhttp_tls_send_t* sends,
                               uint32_t n_sends, const uvhttp_tls_key_t* keys, uint32_t n_keys,
                               uint32_t max_fragment, uvhttp_tls_seal_t* records,
                               uint32_t max_records, uvhttp_tls_send_result_t* results,
                               uvhttp_tls_send_summary_t* summary, uint8_t* out, uint64_t out_cap,
                               void* stream);

/* Seal several parts per send: one numbered, contiguous send per connection out of the frames
 * several builders left (uvhttp_ws_gpu_echo_messages_streams or _relay_, _control_replies_,
 * _close_frames_streams), each with its own frame table and its own per-connection run.  No frame
 * byte is copied: `frames` is ONE device buffer, the send arena, and the caller hands sub-ranges
 * of it to the builders as their d_out; part p says where its builder wrote (base, len = that
 * builder's out_cap), where its offsets lie (frame_off: n_frames + 1 entries relative to base, a
 * builder's d_out_off as it lies) and where send s's run (first_frame, n_frames: two uint32_t)
 * lies, at (char*)runs + s * run_stride — the builders' d_runs / run_stride convention.  The part
 * table itself is host memory, passed by value; the pointers inside are device pointers.
 *
 * Semantics.  Send s is the frame sequence part 0's run, then part 1's run, ...  sends[s] supplies
 * seq, key and type; its first_frame / n_frames are ignored.  Everything else is seal_frames':
 * every frame is cut on its own into ceil(F / max_fragment) records, a record never holds bytes of
 * two frames (and so never of two parts), an empty frame gives no record, the records are numbered
 * seq, seq + 1, ... across all parts and lie back to back in out, sends in index order; results
 * and summary are seal_frames' structs with plain_len the sum over the parts; records[r].src_off
 * = base_p + frame_off_p[f] + cut, so records[] is a valid uvhttp_tls_gpu_seal_records input with
 * src = frames.  Parts may overlap and the same table may be listed twice with two run tables: a
 * relay without the sender is the relay's table once with the frames before the sender's own and
 * once with those after.
 *
 * Per-send failures, in seal_frames' order: ERR_KEY as there; ERR_RANGE if any part's run has
 * first_frame + n_frames > that part's n_frames, or a frame of the run has decreasing offsets or
 * frame_off[f + 1] > len.  A failed send has 0 records and next_seq = seq; the others are not
 * affected, and a bad frame outside every run harms nobody.  Capacity: exactly seal_frames' rule.
 *
 * EINVAL: n_parts 0 or above UVHTTP_TLS_MAX_PARTS; a part with base + len > frames_len, a null
 * or misaligned frame_off (8) or runs (4), run_stride < 8 or not a multiple of 4; the null
 * pointers seal_frames refuses; max_fragment > 16384; more than 2^26 sends, 2^28 frames over all
 * parts or 2^28 records.  n_sends = 0 returns OK with a zeroed summary.  Asynchronous on `stream`,
 * no host synchronisation, scratch in the engine (12 bytes per frame table entry, 44 per send):
 * graph-capturable after one uncaptured call of the same or a larger shape. */
#define UVHTTP_TLS_MAX_PARTS 8
typedef struct {
    uint64_t base;             /* the part's frames start at frames + base */
    uint64_t len;              /* bytes its builder was given (its out_cap); base + len <= frames_len */
    const uint64_t* frame_off; /* n_frames + 1 offsets relative to base, as d_out_off lies */
    const uint32_t* runs;      /* send s: (first_frame, n_frames) at (char*)runs + s * run_stride */
    uint32_t run_stride;       /* >= 8, a multiple of 4 */
    uint32_t n_frames;         /* entries of the table (max_replies, max_echoes, ...) */
} uvhttp_tls_part_t;

int uvhttp_tls_gpu_seal_parts(uvhttp_tls_gpu_engine_t* eng, const uint8_t* frames,
                              uint64_t frames_len, const uvhttp_tls_part_t* parts, uint32_t n_parts,
                              const uvhttp_tls_send_t* sends, uint32_t n_sends,
                              const uvhttp_tls_key_t* keys, uint32_t n_keys, uint32_t max_fragment,
                              uvhttp_tls_seal_t* records, uint32_t max_records,
                              uvhttp_tls_send_result_t* results,
                              uvhttp_tls_send_summary_t* summary, uint8_t* out, uint64_t out_cap,
                              void* stream);

/* Seal several parts per send with the frames COALESCED into full records: what a server that
 * corks its writes puts on the wire.  TLS carries a byte stream, so a receiver cannot tell where
 * the sender's write calls ended; seal_frames and seal_parts cut every frame on its own because
 * the reference's mbedtls_ssl_write loop does, this call does not.  The arguments are seal_parts',
 * argument for argument (frames = the send arena, parts in host memory with device pointers
 * inside, sends[s] supplies seq, key and type and its first_frame / n_frames are ignored).
 *
 * Stream.  Send s's stream is the bytes of part 0's run, then part 1's run, ...  A run whose
 * offsets do not decrease is the one range frames[base_p + frame_off_p[first], base_p +
 * frame_off_p[first + n]), so a stream has at most n_parts segments; empty frames and empty runs
 * contribute nothing.  Frame boundaries mean nothing to the cutting: a record may hold many
 * frames, and a frame (its header too) may lie across two records.
 *
 * Cutting, numbering, layout.  With B the stream's length the send gets ceil(B / max_fragment)
 * records, every one of max_fragment content bytes except the last (max_fragment 1..16384, 0 =
 * 16384); B = 0 gives no record and status 0.  The records are numbered seq, seq + 1, ... and lie
 * back to back in out, sends in index order.  results[s] and summary are seal_frames' structs with
 * seal_frames' meaning: plain_len = B, next_seq = seq + n_records.  The bytes of a record are
 * exactly uvhttp_tls_gpu_seal_records' for the same (key, seq, type, content).
 *
 * records[r] describes record r with src_off = out_off + 5 + the key's explicit-nonce length (8
 * for TLS 1.2 AES-GCM, otherwise 0): the place in `out` where the content was gathered before it
 * was sealed, and where its ciphertext now lies.  So records[] is a valid
 * uvhttp_tls_gpu_seal_records input over any buffer that holds the streams at those offsets (the
 * plaintext is no longer in out after the call).
 *
 * Per-send failures: ERR_KEY, then ERR_RANGE, exactly as seal_parts defines them.  A failed send
 * has 0 records and next_seq = seq, not a byte of out is written for it, and the other sends are
 * not affected; a bad frame outside every run harms nobody.  Capacity: seal_frames' rule.  If the
 * records or bytes of the sends without an error of their own exceed max_records / out_cap, every
 * such send reports ERR_CAPACITY, nothing is written to out or records (no content is gathered
 * either), and summary holds the sizes to call again with.
 *
 * Overlap and broadcast.  Parts may overlap, the same table may be listed twice and sends may name
 * the same frames under N keys: frames is only read.  out is written and then sealed in place, so
 * it may not overlap frames.
 *
 * EINVAL: everything seal_parts refuses, and [out, out + out_cap) intersecting [frames, frames +
 * frames_len).  n_sends = 0 returns OK with a zeroed summary.  Asynchronous on `stream`, no host
 * synchronisation, scratch in the engine (seal_parts' plus 128 bytes of segment table per send and
 * 16 bytes per entry of records[]): graph-capturable after one uncaptured call of the same or a
 * larger shape.  There is no seal_frames-shaped variant: one part whose runs points at
 * &sends[0].first_frame with run_stride = 32 (sizeof(uvhttp_tls_send_t)) expresses it. */
int uvhttp_tls_gpu_seal_parts_coalesced(uvhttp_tls_gpu_engine_t* eng, const uint8_t* frames,
                                        uint64_t frames_len, const uvhttp_tls_part_t* parts,
                                        uint32_t n_parts, const uvhttp_tls_send_t* sends,
                                        uint32_t n_sends, const uvhttp_tls_key_t* keys,
                                        uint32_t n_keys, uint32_t max_fragment,
                                        uvhttp_tls_seal_t* records, uint32_t max_records,
                                        uvhttp_tls_send_result_t* results,
                                        uvhttp_tls_send_summary_t* summary, uint8_t* out,
                                        uint64_t out_cap, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* UVHTTP_TLS_AMD_H */
