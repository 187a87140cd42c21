/*
 * uvhttp_ws_amd.h — C ABI of the MI355X-native WebSocket frame-decode / unmask path.
 *
 * Two surfaces live here:
 *
 *  1. The DROP-IN decode surface of the reference header include/uvhttp_websocket.h
 *     (adam-ikari/uvhttp v2.7.0).  Same symbol names, same argument meaning, same
 *     struct layouts (x86-64: uvhttp_ws_frame_header_t 16 B, uvhttp_ws_frame_t 48 B,
 *     uvhttp_ws_connection_t 248 B), same error convention (UVHTTP_OK = 0, every decode
 *     failure UVHTTP_ERROR_INVALID_PARAM = -1).  When the reference header has already
 *     been included (UVHTTP_WEBSOCKET_H defined) its own type definitions are used and
 *     only the function prototypes below are re-stated.
 *
 *  2. The BATCHED DEVICE surface (new): many masked frames resident in MI355X HBM are
 *     header-parsed, validated, fragment-checked and unmasked by hand-written gfx950
 *     kernels.  Plain pointers and sizes only; the stream is an opaque hipStream_t.
 *     These entry points never compute on the CPU: with no usable GPU they return
 *     UVHTTP_WS_GPU_ENODEV.
 *
 * Batch semantics (the parity contract, checked against the oracle in tests/):
 *   a batch of n frames laid out back to back is decoded exactly as the reference's
 *   uvhttp_ws_process_data (src/uvhttp_websocket.c:825-1097) decodes the same bytes when
 *   it is called once per frame with exactly that frame's wire bytes on a fresh server
 *   connection with the given limits: frames before the first failing frame are
 *   delivered (unmasked), the first failing frame and everything after it are left
 *   untouched, and the failure reason is reported per frame.
 */
#ifndef UVHTTP_WS_AMD_H
#define UVHTTP_WS_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------ */
/* 1. Drop-in types (ABI-identical to the reference; only when its header is absent)    */
/* ------------------------------------------------------------------------------------ */
#ifndef UVHTTP_WEBSOCKET_H

#ifndef UVHTTP_ERROR_H
/* include/uvhttp_error.h:16-20 — only the two codes the decode path returns. */
typedef int uvhttp_error_t;
#define UVHTTP_OK 0
#define UVHTTP_ERROR_INVALID_PARAM (-1)
#endif

#ifndef UVHTTP_CONFIG_H
/* include/uvhttp_config.h — full layout kept so uvhttp_ws_connection_create can read
 * websocket_* at the reference offsets (64..79). */
typedef struct {
    int max_connections;
    int read_buffer_size;
    int backlog;
    int keepalive_timeout;
    int request_timeout;
    int connection_timeout;
    size_t max_body_size;
    size_t max_header_size;
    size_t max_url_size;
    size_t max_file_size;
    int max_requests_per_connection;
    int rate_limit_window;
    int websocket_max_frame_size;
    int websocket_max_message_size;
    int websocket_ping_interval;
    int websocket_ping_timeout;
    int tcp_keepalive_timeout;
    int sendfile_timeout_ms;
    int sendfile_max_retry;
    int cache_default_max_entries;
    int cache_default_ttl;
    int lru_cache_batch_eviction_size;
    int rate_limit_max_requests;
    int rate_limit_max_window_seconds;
    int rate_limit_min_timeout_seconds;
} uvhttp_config_t;
#endif

/* mbedtls is never touched on the decode path; the pointer is carried opaquely. */
typedef struct mbedtls_ssl_context mbedtls_ssl_context;

/* include/uvhttp_websocket.h:24-31 */
typedef enum {
    UVHTTP_WS_OPCODE_CONTINUATION = 0x0,
    UVHTTP_WS_OPCODE_TEXT = 0x1,
    UVHTTP_WS_OPCODE_BINARY = 0x2,
    UVHTTP_WS_OPCODE_CLOSE = 0x8,
    UVHTTP_WS_OPCODE_PING = 0x9,
    UVHTTP_WS_OPCODE_PONG = 0xA
} uvhttp_ws_opcode_t;

/* include/uvhttp_websocket.h:34-39 */
typedef enum {
    UVHTTP_WS_STATE_CONNECTING = 0,
    UVHTTP_WS_STATE_OPEN = 1,
    UVHTTP_WS_STATE_CLOSING = 2,
    UVHTTP_WS_STATE_CLOSED = 3
} uvhttp_ws_state_t;

/* include/uvhttp_websocket.h:42-51 — 16 bytes, payload_length at offset 8. */
typedef struct {
    uint8_t fin : 1;
    uint8_t rsv1 : 1;
    uint8_t rsv2 : 1;
    uint8_t rsv3 : 1;
    uint8_t opcode : 4;
    uint8_t mask : 1;
    uint8_t payload_len : 7;  /* raw 7-bit length code (0..127) */
    uint64_t payload_length;  /* decoded length */
} uvhttp_ws_frame_header_t;

/* include/uvhttp_websocket.h:54-60 — 48 bytes. */
typedef struct {
    uvhttp_ws_frame_header_t header;
    uint64_t payload_length;
    uint8_t masking_key[4];
    uint8_t* payload;
    size_t payload_size;
} uvhttp_ws_frame_t;

/* include/uvhttp_websocket.h:63-69 */
typedef struct {
    int max_frame_size;
    int max_message_size;
    int ping_interval;
    int ping_timeout;
    int enable_compression;
} uvhttp_ws_config_t;

struct uvhttp_ws_connection;

/* include/uvhttp_websocket.h:75-82 */
typedef int (*uvhttp_ws_on_message_callback)(struct uvhttp_ws_connection* conn,
                                             const char* data, size_t len, int opcode);
typedef int (*uvhttp_ws_on_close_callback)(struct uvhttp_ws_connection* conn, int code,
                                           const char* reason);
typedef int (*uvhttp_ws_on_error_callback)(struct uvhttp_ws_connection* conn,
                                           int error_code, const char* error_msg);

/* include/uvhttp_websocket.h:85-121 — 248 bytes. */
typedef struct uvhttp_ws_connection {
    int fd;
    uvhttp_ws_state_t state;
    uvhttp_ws_config_t config;
    mbedtls_ssl_context* ssl;
    int is_server;
    char client_key[64];
    uint8_t* recv_buffer;
    size_t recv_buffer_size;
    size_t recv_buffer_pos;
    uint8_t* send_buffer;
    size_t send_buffer_size;
    uint8_t* fragmented_message;
    size_t fragmented_size;
    size_t fragmented_capacity;
    uvhttp_ws_opcode_t fragmented_opcode;
    uvhttp_ws_on_message_callback on_message;
    uvhttp_ws_on_close_callback on_close;
    uvhttp_ws_on_error_callback on_error;
    void* user_data;
    uint64_t bytes_sent;
    uint64_t bytes_received;
    uint64_t frames_sent;
    uint64_t frames_received;
} uvhttp_ws_connection_t;

#endif /* !UVHTTP_WEBSOCKET_H */

/* Reference defaults (include/uvhttp_defaults.h:171-207). */
#define UVHTTP_WS_AMD_DEFAULT_MAX_FRAME_SIZE (16 * 1024 * 1024)
#define UVHTTP_WS_AMD_DEFAULT_MAX_MESSAGE_SIZE (64 * 1024 * 1024)
#define UVHTTP_WS_AMD_DEFAULT_RECV_BUFFER_SIZE (64 * 1024)
#define UVHTTP_WS_AMD_DEFAULT_PING_INTERVAL 30
#define UVHTTP_WS_AMD_DEFAULT_PING_TIMEOUT 10

/* ------------------------------------------------------------------------------------ */
/* 1b. Drop-in decode functions (replace the reference symbols of the same name)        */
/* ------------------------------------------------------------------------------------ */

/* replaces src/uvhttp_websocket.c:71-109 (decl include/uvhttp_websocket.h:128-130) */
struct uvhttp_ws_connection* uvhttp_ws_connection_create(int fd, mbedtls_ssl_context* ssl,
                                                         int is_server,
                                                         const uvhttp_config_t* config);
/* replaces src/uvhttp_websocket.c:112-130 (decl include/uvhttp_websocket.h:135) */
void uvhttp_ws_connection_free(struct uvhttp_ws_connection* conn);
/* replaces src/uvhttp_websocket.c:1100-1111 (decl include/uvhttp_websocket.h:217-220) */
void uvhttp_ws_set_callbacks(struct uvhttp_ws_connection* conn,
                             uvhttp_ws_on_message_callback on_message,
                             uvhttp_ws_on_close_callback on_close,
                             uvhttp_ws_on_error_callback on_error);
/* replaces src/uvhttp_websocket.c:133-185 (decl include/uvhttp_websocket.h:228-230) */
uvhttp_error_t uvhttp_ws_parse_frame_header(const uint8_t* data, size_t len,
                                            uvhttp_ws_frame_header_t* header,
                                            size_t* header_size);
/* replaces src/uvhttp_websocket.c:188-197 (decl include/uvhttp_websocket.h:250-251) */
void uvhttp_ws_apply_mask(uint8_t* data, size_t len, const uint8_t* masking_key);
/* replaces src/uvhttp_websocket.c:825-1097 (decl include/uvhttp_websocket.h:212-213) */
uvhttp_error_t uvhttp_ws_process_data(struct uvhttp_ws_connection* conn, const uint8_t* data,
                                      size_t len);

/* Control-frame hooks (new).  The reference answers PING with uvhttp_ws_send_pong and
 * echoes CLOSE with uvhttp_ws_send_frame through the server context reached from the
 * wrapper in conn->user_data (src/uvhttp_websocket.c:1028-1084); for CLOSE it captures that
 * context BEFORE calling on_close (which frees the wrapper) and sends AFTER.  The send side
 * lives outside this library, so the integration layer registers:
 *   resolver(conn) -> the server context (wrapper->conn->server->context) or NULL; called
 *                     only when conn->user_data != NULL, at the point the reference reads it;
 *   sink(ctx, conn, opcode, payload, len) -> send; called only with a non-NULL ctx.
 * opcode is UVHTTP_WS_OPCODE_PONG (payload = the ping payload) or UVHTTP_WS_OPCODE_CLOSE
 * (payload = code + reason truncated to 125 B, empty when the close had < 2 bytes). */
typedef void* (*uvhttp_ws_amd_context_resolver)(struct uvhttp_ws_connection* conn);
typedef void (*uvhttp_ws_amd_control_sink)(void* ctx, struct uvhttp_ws_connection* conn,
                                           int opcode, const uint8_t* payload, size_t len);
void uvhttp_ws_amd_set_control_hooks(uvhttp_ws_amd_context_resolver resolver,
                                     uvhttp_ws_amd_control_sink sink);

/* ------------------------------------------------------------------------------------ */
/* 2. Batched device surface (MI355X / gfx950)                                          */
/* ------------------------------------------------------------------------------------ */

/* Return codes of the device surface (0 = OK; negative = failure, nothing launched). */
#define UVHTTP_WS_GPU_OK 0
#define UVHTTP_WS_GPU_EINVAL (-1)  /* bad argument (NULL, misaligned, sizes) */
#define UVHTTP_WS_GPU_ENODEV (-2)  /* no usable MI355X / HIP runtime error at setup */
#define UVHTTP_WS_GPU_ENOMEM (-3)  /* device workspace allocation failed */
#define UVHTTP_WS_GPU_ELAUNCH (-4) /* kernel launch / HIP call failed */

/* Per-frame status (uvhttp_ws_frame_desc_t.status).  Negative values are the reasons
 * uvhttp_ws_process_data returns UVHTTP_ERROR_INVALID_PARAM, with the reference check
 * that raises each one. */
#define UVHTTP_WS_FRAME_OK 0
#define UVHTTP_WS_FRAME_INCOMPLETE 1        /* last frame not fully present (need more data, :925-932) */
#define UVHTTP_WS_FRAME_SKIPPED 2           /* after the first failing frame: not processed */
#define UVHTTP_WS_FRAME_ERR_PARSE (-1)      /* 64-bit length with MSB set (:178-180) */
#define UVHTTP_WS_FRAME_ERR_RSV (-2)        /* RSV1-3 set (:895-897) */
#define UVHTTP_WS_FRAME_ERR_CONTROL (-3)    /* control frame > 125 B or FIN=0 (:902-906) */
#define UVHTTP_WS_FRAME_ERR_UNMASKED (-4)   /* server got an unmasked frame (:910-912) */
#define UVHTTP_WS_FRAME_ERR_TOO_BIG (-5)    /* payload > max_frame_size (:919-921) */
#define UVHTTP_WS_FRAME_ERR_BUFFER (-6)     /* wire bytes exceed recv-buffer cap (:851-857) */
#define UVHTTP_WS_FRAME_ERR_FRAGMENT (-7)   /* CONT with no start / data inside fragment (:964-996) */
#define UVHTTP_WS_FRAME_ERR_MESSAGE (-8)    /* fragments exceed max_message_size (:786-791) */
#define UVHTTP_WS_FRAME_ERR_LAYOUT (-9)     /* offset table disagrees with the frame lengths */
#define UVHTTP_WS_FRAME_ERR_CAPACITY (-10)  /* stream decode: more frames than the desc array holds */
#define UVHTTP_WS_FRAME_ERR_DEVICE (-11)    /* the device could not complete the call (a bounded
                                               wait in the single-pass scan gave up): nothing was
                                               decoded; uvhttp_ws_gpu_engine_sync reports ELAUNCH */

/* Frame flags (uvhttp_ws_frame_desc_t.flags). */
#define UVHTTP_WS_FLAG_FIN 0x01u
#define UVHTTP_WS_FLAG_MASK 0x02u
#define UVHTTP_WS_FLAG_RSV1 0x04u
#define UVHTTP_WS_FLAG_RSV2 0x08u
#define UVHTTP_WS_FLAG_RSV3 0x10u
#define UVHTTP_WS_FLAG_MSG_END 0x20u  /* this frame completes a data message (on_message fires) */

/* One decoded frame (device-written, 32 bytes). */
typedef struct {
    uint64_t payload_off;  /* byte offset of the unmasked payload: in the wire buffer
                              (in-place decode, and control frames of a compact decode)
                              or in the message arena (data frames of a compact decode) */
    uint64_t payload_len;  /* header.payload_length */
    uint32_t masking_key;  /* key bytes k0..k3 as a little-endian word (k0 = low byte) */
    uint32_t message;      /* index of the message this data frame belongs to (compact) */
    uint8_t opcode;        /* header.opcode */
    uint8_t flags;         /* UVHTTP_WS_FLAG_* */
    uint8_t header_size;   /* 2 / 4 / 10 (mask key excluded, as parse_frame_header) */
    int8_t status;         /* UVHTTP_WS_FRAME_* */
    uint32_t wire_len;     /* header + key + payload bytes (saturated at 2^32-1) */
} uvhttp_ws_frame_desc_t;

/* One complete data message (compact decode only, 32 bytes).  The payload handed to
 * on_message is arena[arena_off, arena_off + len); the opcode is the first frame's.  When the
 * summary reports pending_bytes != 0, entry [n_messages] describes the message still open
 * after the last delivered frame (its bytes so far, last_frame = the latest fragment) and
 * `reserved` holds its first fragment's payload length; otherwise reserved is 0. */
typedef struct {
    uint64_t arena_off;
    uint64_t len;
    uint32_t first_frame;
    uint32_t last_frame;
    int32_t opcode;
    uint32_t reserved;
} uvhttp_ws_message_desc_t;

/* Batch summary (device-written; copy back after the stream completes). */
typedef struct {
    uint32_t n_frames;        /* frames in the batch */
    uint32_t n_delivered;     /* frames processed before the first failing frame */
    int32_t status;           /* UVHTTP_OK, or UVHTTP_ERROR_INVALID_PARAM on a failing frame */
    int32_t first_status;     /* status of frame n_delivered (0 if all delivered) */
    uint64_t consumed_bytes;  /* wire bytes of the delivered frames (recv-buffer drain) */
    uint64_t payload_bytes;   /* sum of delivered payload bytes */
    uint32_t n_messages;      /* complete data messages among the delivered frames */
    uint32_t state_closed;    /* 1 if a delivered CLOSE frame set state = CLOSED */
    uint64_t arena_bytes;     /* compact: arena bytes written */
    uint64_t pending_bytes;   /* bytes of a fragmented message still open at the end */
} uvhttp_ws_batch_summary_t;

/* A batch of frames resident in device memory. */
typedef struct {
    uint8_t* wire;             /* device pointer, 16-byte aligned; frames back to back */
    uint64_t wire_len;         /* bytes readable at wire */
    const uint64_t* frame_off; /* device pointer: n_frames start offsets, or NULL */
    uint64_t frame_stride;     /* when frame_off == NULL: frame i starts at i*stride */
    uint32_t n_frames;
    int32_t max_frame_size;    /* uvhttp_ws_config_t.max_frame_size */
    int32_t max_message_size;  /* uvhttp_ws_config_t.max_message_size */
    int32_t is_server;         /* 1: unmasked frames are rejected (reference server) */
} uvhttp_ws_batch_t;

typedef struct uvhttp_ws_gpu_engine uvhttp_ws_gpu_engine_t;

/* Create an engine bound to HIP device `device` (owns the scratch workspace). */
int uvhttp_ws_gpu_engine_create(int device, uvhttp_ws_gpu_engine_t** out);
void uvhttp_ws_gpu_engine_free(uvhttp_ws_gpu_engine_t* eng);
/* Pre-size the workspace so later decode calls never allocate (hipGraph capture). */
int uvhttp_ws_gpu_engine_reserve(uvhttp_ws_gpu_engine_t* eng, uint32_t max_frames,
                                 uint64_t max_wire_bytes, uint64_t max_arena_bytes);
/* Payload-kernel workgroup shape: `block` threads x `vectors_per_lane` 16-byte vectors per
 * workgroup tile; (0, 0) = automatic (by average frame size).  Supported: 64x1, 64x2, 64x4,
 * 128x1, 128x2, 256x1, 256x2, 256x4.  A tuning knob only: results are identical. */
int uvhttp_ws_gpu_engine_set_tile(uvhttp_ws_gpu_engine_t* eng, int block, int vectors_per_lane);
/* Kernel timing: with enable = k >= 1, HIP events bracket the dominant (payload) kernel of
 * every k-th call (k = 1: every call) on its stream — each timed marker idles the device a few
 * microseconds, so sampling keeps that cost off most calls; 0 disables.  kernel_time returns
 * the summed milliseconds and the number of bracketed launches completed so far
 * (synchronises on the last event). */
int uvhttp_ws_gpu_engine_set_timing(uvhttp_ws_gpu_engine_t* eng, int enable);
int uvhttp_ws_gpu_engine_kernel_time(uvhttp_ws_gpu_engine_t* eng, double* ms,
                                     uint64_t* launches);
const char* uvhttp_ws_gpu_engine_last_error(const uvhttp_ws_gpu_engine_t* eng);
/* Wait for `stream` and report device-side failures of the calls made since the previous
 * sync: UVHTTP_WS_GPU_ELAUNCH if any of them flagged UVHTTP_WS_FRAME_ERR_DEVICE (their
 * summaries / results say so too, and nothing of them was unmasked), else OK. */
int uvhttp_ws_gpu_engine_sync(uvhttp_ws_gpu_engine_t* eng, void* stream);

/* Device-side kernel stamps (diagnostics).  With stamps on, every kernel of a decode call
 * records on the GPU's constant wall clock when its first workgroups started and when its
 * last wave ended, so the time between the kernels of a call — and between one call's last
 * kernel and the next call's first — is read off the device timeline rather than inferred
 * from host events.  The engine keeps the last 128 calls (71 MB of device memory, allocated
 * when stamps are first turned on); read_stamps returns one record per (call, kernel) it holds,
 * in call then start order, and clears them.  While on, each kernel's first 256 workgroups and
 * a sample of its waves store a word each (plain stores; C3 0.2 %, C4 1 % slower); off (the
 * default) it costs one untaken branch per kernel.  Calls made while their stream is captured
 * are not stamped.  The payload kernel of a compact decode of large frames (k_gather_compact)
 * is not stamped. */
#define UVHTTP_WS_STAMP_WALK 0        /* k_swalk_lane / k_swalk_wave (frame discovery) */
#define UVHTTP_WS_STAMP_WALK_SCAN 1   /* k_swalk_scan (first frame per connection) */
#define UVHTTP_WS_STAMP_WALK2 2       /* second walk (two-pass mode) */
#define UVHTTP_WS_STAMP_STREAM_DESC 3 /* k_stream_desc / k_stream_desc_lane */
#define UVHTTP_WS_STAMP_CLAIMS 4      /* (k_stream_claims until round 5: unused) */
#define UVHTTP_WS_STAMP_PAYLOAD 5     /* the payload kernel (unmask / scatter / gather) */
#define UVHTTP_WS_STAMP_PLAN 6        /* k_plan; in-place stride batches of large frames: k_large_fix,
                                         the launch behind the payload pass that takes its place (it
                                         plans nothing: tests/test_gpu_stamps.py asks such a call for
                                         a "plan" record; once that test names the kernels per path,
                                         k_large_fix should get a kind of its own after SPEC_PLAN) */
#define UVHTTP_WS_STAMP_FIXUP 7       /* k_fixup (fused stride path) */
#define UVHTTP_WS_STAMP_FINALIZE 8    /* k_finalize; summary-only compact: k_sum_msgs */
#define UVHTTP_WS_STAMP_BUILD_SIZE 9  /* send side: kb_size (the emit kernels stamp as PAYLOAD) */
#define UVHTTP_WS_STAMP_BUILD_SCAN 10 /* kb_scan_one / kb_scan_groups */
#define UVHTTP_WS_STAMP_BUILD_SCAN2 11 /* kb_scan_top */
#define UVHTTP_WS_STAMP_BUILD_OFFSETS 12 /* kb_offsets (tile emit only) */
#define UVHTTP_WS_STAMP_DESC_EMIT 13  /* k_desc_emit (stride batches with descriptors) */
#define UVHTTP_WS_STAMP_SUM_SCAN 14   /* k_sum_scan ahead of k_desc_emit (the summary-only
                                         decodes' k_sum_scan stamps as PLAN) */
#define UVHTTP_WS_STAMP_SPEC_PLAN 15  /* k_sspec_plan (speculative stream decode; its pass
                                         stamps as PAYLOAD, k_sspec_emit as STREAM_DESC) */
typedef struct {
    uint32_t call;      /* the call's tag: 1 .. 2^24 - 1, one more per decode call (after
                           2^24 - 1 wraps to 1); records come oldest call first */
    uint32_t kernel;    /* UVHTTP_WS_STAMP_* */
    uint64_t begin_ns;  /* device wall clock, ns: earliest sampled workgroup start */
    uint64_t end_ns;    /* latest wave end */
} uvhttp_ws_gpu_stamp_t;
int uvhttp_ws_gpu_engine_set_stamps(uvhttp_ws_gpu_engine_t* eng, int enable);
/* Waits for the device; *n_out = records written (at most cap).  A pass launched as several
 * dispatch pieces (over 2^24 workgroups, e.g. a C5 pass) reads as one record spanning all of
 * them: begin = the first piece's start, end = the latest wave end of any piece. */
int uvhttp_ws_gpu_engine_read_stamps(uvhttp_ws_gpu_engine_t* eng, uvhttp_ws_gpu_stamp_t* out,
                                     uint32_t cap, uint32_t* n_out);
/* Host-only pieces of the stamp ring (no device needed; tests drive them):
 * ring_words = the ring's size in 64-bit words; stamps_reduce = read_stamps's reduction of a
 * ring copy (epoch = the engine's latest call, khz = wall-clock rate); stamp_simulate writes
 * what one launch piece of `blocks` workgroups starting at pass index `base` stores, with the
 * kernels' own slot mapping (workgroup i starts at t_begin + i (t_end - t_begin) / blocks and
 * ends dur ticks later). */
uint64_t uvhttp_ws_gpu_stamp_ring_words(void);
int uvhttp_ws_gpu_stamps_reduce(const uint64_t* ring, uint32_t epoch, uint32_t khz,
                                uvhttp_ws_gpu_stamp_t* out, uint32_t cap, uint32_t* n_out);
int uvhttp_ws_gpu_stamp_simulate(uint64_t* ring, uint32_t epoch, uint32_t kind, uint64_t base,
                                 uint32_t blocks, uint32_t waves, uint64_t t_begin, uint64_t t_end,
                                 uint64_t dur);

/* Streams and graphs.  An engine owns one workspace, so its calls must execute one after
 * another: when a call names a different stream than the previous call, the engine makes the
 * new stream wait for the work already queued on the old one (an event), so calls from
 * several streams serialise on the device instead of corrupting each other.  For concurrency
 * use one engine per stream (the pipelines do).
 * A call made while its stream is being captured (hipStreamBeginCapture) is graph-safe: its
 * kernels take their epoch tag from device memory, bumped by a small kernel at the start of
 * every replay, so replays of the same graph over changing frame bytes never accept tags a
 * previous replay left behind.  Reserve the workspace before capturing (engine_reserve;
 * stream decode: one uncaptured call of the same or larger shape) — a captured call that
 * would allocate fails with EINVAL.  A graph holds the addresses of the engine's scratch as of
 * its capture (among them every block the epoch kernel clears when the device epochs wrap),
 * so make the engine's largest calls of every kind, or reserve, before capturing: a later
 * uncaptured call that grows a scratch block invalidates the graphs captured before it.
 * Kernel timing is not recorded inside a capture. */

/* In-place decode: parse + validate every frame, run the fragment state machine, then
 * unmask the payload of every delivered frame in place in batch->wire (the reference
 * unmasks inside recv_buffer, src/uvhttp_websocket.c:937-947).  d_desc (n_frames
 * entries) and d_summary are device pointers.  Asynchronous on `stream`.
 * d_desc may be NULL (summary-only decode): the wire and d_summary come out exactly as with
 * descriptors, and no per-frame output is written.  A fixed-stride batch of small frames
 * (stride >= 140 bytes, every frame able to fit the message limit) then runs as one payload
 * pass writing an info byte per frame plus two short kernels (fragment state machine and
 * summary; after a failure the frames from it on are masked again); any other batch is decoded
 * into descriptors in engine scratch (grown on demand, so reserve or run one uncaptured call
 * of the shape before capturing a graph).  For a caller that only needs "every frame delivered"
 * or the first failure, e.g. a server that re-walks delivered frames on the host. */
int uvhttp_ws_gpu_decode_inplace(uvhttp_ws_gpu_engine_t* eng, const uvhttp_ws_batch_t* batch,
                                 uvhttp_ws_frame_desc_t* d_desc,
                                 uvhttp_ws_batch_summary_t* d_summary, void* stream);

/* Compact decode: as above, but data-frame payloads are unmasked out of place into
 * d_arena at the exclusive prefix sum of data payload lengths, so every message —
 * including a fragmented one (uvhttp_ws_fragment_append, :781-822) — is one contiguous
 * arena range described by d_msgs.  Control-frame payloads are unmasked in place in the
 * wire.  d_msgs needs room for n_frames entries; arena_cap must cover the data payload.
 * Arena bytes past summary->arena_bytes (up to arena_cap) are scratch: a fixed-stride batch is
 * decoded speculatively, and when it fails part-way the payloads of frames after the failure
 * may have been written there.  d_desc may be NULL (descriptors then go to engine scratch;
 * the arena, d_msgs and d_summary are the same). */
int uvhttp_ws_gpu_decode_compact(uvhttp_ws_gpu_engine_t* eng, const uvhttp_ws_batch_t* batch,
                                 uint8_t* d_arena, uint64_t arena_cap,
                                 uvhttp_ws_frame_desc_t* d_desc,
                                 uvhttp_ws_message_desc_t* d_msgs,
                                 uvhttp_ws_batch_summary_t* d_summary, void* stream);

/* ---- UTF-8 validation of TEXT messages (RFC 6455 §5.6, §8.1) --------------------------- */
/* The reference never checks that a TEXT message is UTF-8; a conforming endpoint must fail the
 * connection with close code 1007 when it is not.  This is a separate, opt-in call made after a
 * compact decode (every message, a fragmented one included, is then one contiguous arena
 * range): it reads each arena byte once and writes one 4-byte verdict per message plus a
 * 16-byte summary.  No decode or deliver call changes what it delivers; the caller looks at the
 * verdicts and closes with 1007. */
#define UVHTTP_WS_UTF8_VALID     0  /* complete TEXT message, well-formed UTF-8 (RFC 3629) */
#define UVHTTP_WS_UTF8_INVALID   1  /* not UTF-8: overlong, surrogate, > U+10FFFF, stray or missing
                                       continuation, truncated at the message end */
#define UVHTTP_WS_UTF8_NOT_TEXT  2  /* opcode != 1: not examined */
#define UVHTTP_WS_UTF8_PREFIX    3  /* the open message only: valid so far; `tail` bytes (0..3) at its
                                       end start a sequence that some continuation can complete */
#define UVHTTP_WS_UTF8_BAD_RANGE 4  /* [arena_off, arena_off+len) not inside data_len: not read */

typedef struct { uint8_t status; uint8_t tail; uint16_t reserved; } uvhttp_ws_utf8_verdict_t;   /* 4 B */
typedef struct {
    uint32_t n_text;         /* TEXT messages judged (the open one included) */
    uint32_t n_invalid;      /* of them INVALID or BAD_RANGE */
    uint32_t first_invalid;  /* lowest such message index, 0xFFFFFFFF if none */
    uint32_t open_verdict;   /* status | tail << 8 of the open message's entry, 0 if none */
} uvhttp_ws_utf8_summary_t;                                                                    /* 16 B */

/* All pointers are device pointers (d_data 16-byte aligned, d_msgs 8, the others 4); asynchronous
 * on `stream`, under the engine's rule for calls from different streams (above).
 *   After a compact decode: d_data = d_arena, data_len = arena_cap (or any bound >= the
 *   summary's arena_bytes), d_msgs and d_batch_summary = the decode's d_msgs and d_summary;
 *   n_msgs is ignored.  The kernels read n_messages and pending_bytes from device memory, so no
 *   host sync sits between decode and validation.  Entries [0, n_messages) are judged as
 *   complete messages; when pending_bytes != 0, entry [n_messages] (the open message) is judged
 *   as a prefix: PREFIX with `tail`, or INVALID as soon as no continuation could make it valid
 *   (ED A0, F4 90, E0 9F are invalid at once; E0, F0 9F 98, C2 are PREFIX with tail 1, 3, 1).  A
 *   failed batch judges exactly the messages its summary counts.  Entries past max_msgs are
 *   neither read nor judged.
 *   Generic form: d_batch_summary == NULL; the caller's own table of n_msgs complete messages is
 *   judged (opcode 1 where a check is wanted).  Ranges must ascend in arena_off and must not
 *   overlap; gaps are allowed.  A table that breaks the rule gets unspecified verdicts, but
 *   nothing outside [0, data_len) is read.
 * max_msgs is the capacity of d_verdict (entries); nothing past it is read or written.  EINVAL
 * for NULL or misaligned arguments and for n_msgs > max_msgs.  Graph-capturable: no allocation,
 * no epoch-tagged scratch.  A zero-length TEXT message is VALID.  To continue an open message
 * on the host, seed uvhttp_ws_utf8_feed's state with the last `tail` bytes of its arena range. */
int uvhttp_ws_gpu_validate_utf8(uvhttp_ws_gpu_engine_t* eng, const uint8_t* d_data, uint64_t data_len,
                                const uvhttp_ws_message_desc_t* d_msgs, uint32_t max_msgs,
                                const uvhttp_ws_batch_summary_t* d_batch_summary, uint32_t n_msgs,
                                uvhttp_ws_utf8_verdict_t* d_verdict,
                                uvhttp_ws_utf8_summary_t* d_utf8_summary, void* stream);

/* Host UTF-8 check (plain C, incremental): for drop-in users who stay on
 * uvhttp_ws_process_data, and to continue an open message after the device judged its prefix.
 * A zeroed state is the start of a message.  feed returns 0, or -1 as soon as the bytes fed so
 * far cannot be extended to valid UTF-8 (fail-fast, the same rule as the device's PREFIX
 * verdicts); the state is then unspecified.  finish returns 0 iff no sequence is open (the
 * message may end here).  After feed, pend[0, n) are the bytes of the open sequence — so the
 * state after a device PREFIX verdict is n = tail, pend = the last `tail` bytes of the
 * message's arena range. */
typedef struct { uint8_t pend[3]; uint8_t n; } uvhttp_ws_utf8_state_t;   /* zero = start of message */
int uvhttp_ws_utf8_feed(uvhttp_ws_utf8_state_t* st, const uint8_t* data, size_t len);
int uvhttp_ws_utf8_finish(const uvhttp_ws_utf8_state_t* st);

/* Unmask only (no framing): data[i] ^= key[i % 4] for a device buffer — the batched form
 * of uvhttp_ws_apply_mask for callers that parsed headers themselves. */
int uvhttp_ws_gpu_apply_mask(uvhttp_ws_gpu_engine_t* eng, uint8_t* d_data, uint64_t len,
                             const uint8_t masking_key[4], void* stream);

/* Synthetic masked-frame generator (bench / parity inputs; not on the decode path).
 * Writes n_frames frames of payload_len bytes back to back at d_wire (stride =
 * header + 4 + payload_len).  Frame i: opcode = (i == 0 || !fragmented) ? opcode0 :
 * CONTINUATION; FIN = !fragmented || i == n_frames - 1; key = splitmix64(seed ^ i)
 * low 32 bits (frames 0 and 1 forced to 0x00000000 / 0xFFFFFFFF when force_keys);
 * plaintext byte b = byte (b & 7) of splitmix64(seed + ((uint64)i << 32) + (b >> 3)).
 * Same definition as oracle/ws_oracle.c:oracle_gen_frames. */
uint64_t uvhttp_ws_gen_frame_stride(uint64_t payload_len);
int uvhttp_ws_gpu_gen_frames(uvhttp_ws_gpu_engine_t* eng, uint8_t* d_wire, uint32_t n_frames,
                             uint64_t payload_len, uint64_t seed, int opcode0, int fragmented,
                             int force_keys, void* stream);
/* Frames [first, first + count) of that n_frames batch, written from d_wire on (the bench's
 * ranks: rank r's shard is frames [first, ...) of the whole configuration, as
 * oracle_gen_frames(first, count, n_frames) writes them). */
int uvhttp_ws_gpu_gen_frames_range(uvhttp_ws_gpu_engine_t* eng, uint8_t* d_wire, uint32_t first,
                                   uint32_t count, uint32_t n_frames, uint64_t payload_len,
                                   uint64_t seed, int opcode0, int fragmented, int force_keys,
                                   void* stream);

/* ---- batched stateful stream decode (many connections per launch) --------------------- */
/* One entry per connection: the bytes uvhttp_ws_process_data would hold after appending the
 * new reads (recv_buffer[0, recv_buffer_pos) followed by the reads), placed at wire[begin,
 * begin + len), plus the connection state the decoder reads.  Streams must be ordered by
 * `begin` and must not overlap.  Frame boundaries are found on the device (one lane or wave
 * walks each connection's headers), so no offset table is needed.
 *
 * Reads.  n_reads == 0: the bytes are ONE process_data call.  n_reads > 0: they are n_reads
 * consecutive calls, read k ending at stream offset read_end[first_read + k] (relative to
 * begin; non-decreasing; the last equals len; the buffered prefix belongs to call 0).  The
 * device applies process_data's per-call rules exactly as the reference meets them when
 * on_websocket_read feeds one libuv read or one mbedtls_ssl_read chunk per call
 * (src/uvhttp_connection.c:1128-1164): the recv-buffer growth and its max_frame_size cap at
 * the start of every call (src/uvhttp_websocket.c:832-857), a frame is delivered by the call
 * that completes it, a frame whose header fails a check fails the call in which its header
 * bytes arrive, and the calls after a failing call never run (the caller closes). */
typedef struct {
    uint64_t begin;             /* offset of the connection's bytes in the batch wire */
    uint64_t len;               /* recv_buffer_pos + new bytes */
    uint64_t recv_buffer_size;  /* conn->recv_buffer_size before the first call */
    uint64_t pending_bytes;     /* conn->fragmented_size if conn->fragmented_message, else 0 */
    int32_t pending_opcode;     /* conn->fragmented_opcode */
    int32_t max_frame_size;     /* conn->config.max_frame_size */
    int32_t max_message_size;   /* conn->config.max_message_size */
    int32_t is_server;          /* conn->is_server */
    uint32_t first_read;        /* this connection's reads: read_end[first_read, +n_reads) */
    uint32_t n_reads;           /* 0 = one call with all len bytes */
    uint64_t reserved;
} uvhttp_ws_stream_t;           /* 64 bytes */

/* Per-connection outcome: exactly what the process_data calls return and leave behind
 * (src/uvhttp_websocket.c:825-1097). */
typedef struct {
    uint32_t first_frame;        /* this connection's frames start at desc[first_frame] */
    uint32_t n_frames;           /* frames found: delivered + (if it failed) the failing one */
    uint32_t n_delivered;
    int32_t status;              /* the last call's return: UVHTTP_OK or ..._INVALID_PARAM */
    int32_t first_status;        /* UVHTTP_WS_FRAME_* of the failure (0 if none) */
    uint32_t calls;              /* process_data calls that ran (a failing call included) */
    uint64_t consumed_bytes;     /* complete frames drained from the front of the stream */
    uint64_t recv_buffer_size;   /* after the last call that ran (the buffer may have grown) */
    uint64_t pending_bytes;      /* open fragmented message after the calls (0 = none) */
    uint64_t buffered_end;       /* stream bytes [consumed_bytes, buffered_end) are what
                                    recv_buffer holds afterwards (0 when the first call failed
                                    its growth check: recv_buffer is then untouched) */
    uint64_t reserved;
} uvhttp_ws_stream_result_t;     /* 64 bytes */

/* Decode every connection's frames in one set of launches, in place (delivered payloads
 * unmasked inside wire).  d_desc has room for max_frames; if the streams hold more frames
 * every result reports UVHTTP_WS_FRAME_ERR_CAPACITY and nothing is unmasked. */
int uvhttp_ws_gpu_decode_streams(uvhttp_ws_gpu_engine_t* eng, uint8_t* d_wire, uint64_t wire_len,
                                 const uvhttp_ws_stream_t* d_streams, uint32_t n_streams,
                                 uint32_t max_frames, uvhttp_ws_frame_desc_t* d_desc,
                                 uvhttp_ws_stream_result_t* d_results, void* stream);
/* As decode_streams, with several process_data calls per connection: d_read_end (device,
 * n_reads_total entries) holds the read boundaries the streams' first_read / n_reads index.
 * A connection whose read table is malformed (out of range, decreasing, last != len) reports
 * UVHTTP_WS_FRAME_ERR_LAYOUT and is not decoded.  decode_streams == decode_reads with no
 * read table (every stream must then have n_reads == 0). */
int uvhttp_ws_gpu_decode_reads(uvhttp_ws_gpu_engine_t* eng, uint8_t* d_wire, uint64_t wire_len,
                               const uvhttp_ws_stream_t* d_streams, uint32_t n_streams,
                               const uint64_t* d_read_end, uint32_t n_reads_total,
                               uint32_t max_frames, uvhttp_ws_frame_desc_t* d_desc,
                               uvhttp_ws_stream_result_t* d_results, void* stream);

/* Host side of the stream decode.  stream_init fills a descriptor from a live connection
 * (the caller copies recv_buffer[0, recv_buffer_pos) and the new reads to wire[begin, ...);
 * n_reads = 0, set first_read / n_reads for several calls); deliver_stream then applies a
 * decoded result to the connection exactly as the process_data calls would have: recv buffer
 * growth, on_message / on_close / control hooks for the delivered frames (fragments
 * reassembled in conn->fragmented_message), the bytes left in recv_buffer — including a
 * failing data frame the reference had already unmasked before its fragment check rejected
 * it (src/uvhttp_websocket.c:944 before :964-1000) — and the fragment state that check left.
 * `wire` and `desc` are host copies of the decoded batch. */
void uvhttp_ws_stream_init(const struct uvhttp_ws_connection* conn, uint64_t begin,
                           uint64_t len, uvhttp_ws_stream_t* out);
uvhttp_error_t uvhttp_ws_deliver_stream(struct uvhttp_ws_connection* conn, const uint8_t* wire,
                                        const uvhttp_ws_frame_desc_t* desc,
                                        const uvhttp_ws_stream_t* s,
                                        const uvhttp_ws_stream_result_t* r);

/* ---- UTF-8 validation of TEXT frames after an in-place or stream decode ------------------ */
/* uvhttp_ws_gpu_validate_utf8 (above) needs a compact decode.  These calls judge the TEXT
 * messages where an in-place decode (decode_inplace, the pipelines' submit / wait) or a stream
 * decode (decode_streams / decode_reads, the batcher) left them: as unmasked payloads inside
 * the wire, a message's bytes split over frames with headers, control frames and other
 * connections' bytes in between, and possibly open across calls.  Opt-in, made after the
 * decode; no decode, deliver, pipeline or batcher call changes what it does.
 *
 * Which frames are judged.  Connection s: desc[first_frame, first_frame + n_delivered).  The
 * streams form reads first_frame and n_delivered from d_results[s] on the device, the in-place
 * form n_delivered from d_batch_summary (one connection, first_frame 0, nothing carried in), so
 * no host sync sits between decode and validation.  Failing, SKIPPED and INCOMPLETE frames and
 * everything after a connection's first failure are neither read nor judged; nor is a
 * descriptor at or past max_frames (n_frames).  A connection whose result is ERR_CAPACITY or
 * ERR_LAYOUT judges nothing and is VALID.
 *
 * Message membership follows the decoder: a delivered frame with opcode 1 or 2 starts a
 * message; a delivered CONTINUATION belongs to the message the nearest earlier delivered start
 * frame of the connection began, or, when there is none, to the carried-in message — opcode
 * d_streams[s].pending_opcode when pending_bytes != 0, with d_state_in[s] its open sequence
 * (used only when that opcode is TEXT; d_state_in == NULL means all zero).  FIN ends the
 * message.  Control frames in between contribute nothing.  Only bytes of TEXT messages are
 * examined; BINARY payloads may hold anything.
 *
 * Verdict, per connection.  Take a TEXT message's bytes in frame order, the carried-in pend
 * first.  first_invalid is the first frame after which they can no longer be extended to valid
 * UTF-8 (the fail-fast rule of uvhttp_ws_utf8_feed: ED A0, F4 90, E0 9F and a stray
 * continuation byte are invalid at the byte that shows it), or the FIN frame of a message that
 * ends inside a sequence (a zero-length FIN CONTINUATION included).  INVALID is sticky: later
 * frames do not change first_invalid.  PREFIX: no violation, and a TEXT message is still open
 * after the last delivered frame; `state` holds its open sequence (0-3 bytes, gathered across
 * frames when the fragments are tiny).  Passing that state back as d_state_in[s] with the next
 * call (whose d_streams[s] carries the decoder's pending_opcode / pending_bytes) gives the
 * verdicts one call over all the bytes would.  VALID otherwise.  n_text_frames counts every
 * delivered data frame of a TEXT message, those after first_invalid included.
 * UVHTTP_WS_UTF8_CHECK_CLOSE (RFC 6455 §5.5.1): bytes [2, len) of a delivered CLOSE frame with
 * payload_len > 2 are judged as one complete message, a violation blames that frame; without
 * the flag CLOSE frames are ignored.
 * BAD_RANGE: a judged frame's payload range is not inside [0, wire_len); first_invalid names
 * it, and it wins over INVALID when it is the earlier frame.  Nothing outside the wire is read.
 * Delivered frames must ascend in payload_off with the descriptor index (every decode writes
 * them so); a table that breaks the rule gets unspecified verdicts, but nothing outside the
 * wire, the descriptors below max_frames and the n_streams entries is read or written.
 *
 * All pointers are device pointers: d_wire 16-byte aligned (as uvhttp_ws_batch_t.wire), d_desc,
 * d_streams, d_results and d_batch_summary 8, the others 4.  EINVAL for NULL (d_state_in
 * excepted) or misaligned arguments, and for max_frames > 2^28 or n_streams > 2^31.
 * Asynchronous on `stream` under the engine's stream rule.  The call keeps per-frame scratch
 * in the engine (36 bytes per descriptor), grown on demand: graph-capturable once one
 * uncaptured call of the same or a larger shape (max_frames, n_streams) has been made; a
 * captured call that would allocate fails with ENOMEM. */
#define UVHTTP_WS_UTF8_CHECK_CLOSE 0x1u   /* flags: also judge CLOSE reasons */

typedef struct {                  /* 16 B, one per connection, device-written */
    uint32_t first_invalid;       /* desc index (absolute) of the first frame at which the
                                     connection's text is certainly not UTF-8 (or whose range is
                                     bad); 0xFFFFFFFF if none */
    uint32_t n_text_frames;       /* delivered data frames of TEXT messages */
    uvhttp_ws_utf8_state_t state; /* PREFIX only: the open sequence's bytes (pend[0, n)), i.e. what
                                     uvhttp_ws_utf8_feed would hold; zero otherwise */
    uint8_t status;               /* UVHTTP_WS_UTF8_VALID / INVALID / PREFIX / BAD_RANGE */
    uint8_t reserved[3];
} uvhttp_ws_utf8_conn_verdict_t;

typedef struct {                  /* 16 B */
    uint32_t n_text_frames;       /* sum over the connections */
    uint32_t n_invalid_conns;     /* connections INVALID or BAD_RANGE */
    uint32_t first_invalid_conn;  /* lowest such connection, 0xFFFFFFFF if none */
    uint32_t n_open_conns;        /* connections PREFIX */
} uvhttp_ws_utf8_frames_summary_t;

int uvhttp_ws_gpu_validate_utf8_streams(uvhttp_ws_gpu_engine_t* eng, const uint8_t* d_wire,
                                        uint64_t wire_len, const uvhttp_ws_frame_desc_t* d_desc,
                                        uint32_t max_frames, const uvhttp_ws_stream_t* d_streams,
                                        const uvhttp_ws_stream_result_t* d_results, uint32_t n_streams,
                                        const uvhttp_ws_utf8_state_t* d_state_in, uint32_t flags,
                                        uvhttp_ws_utf8_conn_verdict_t* d_verdict,
                                        uvhttp_ws_utf8_frames_summary_t* d_summary, void* stream);
int uvhttp_ws_gpu_validate_utf8_inplace(uvhttp_ws_gpu_engine_t* eng, const uint8_t* d_wire,
                                        uint64_t wire_len, const uvhttp_ws_frame_desc_t* d_desc,
                                        uint32_t n_frames,
                                        const uvhttp_ws_batch_summary_t* d_batch_summary,
                                        uint32_t flags, uvhttp_ws_utf8_conn_verdict_t* d_verdict,
                                        uvhttp_ws_utf8_frames_summary_t* d_summary, void* stream);
/* Host twin (plain C, host copies of the wire and descriptors): the same verdict for one
 * connection, desc[first_frame, first_frame + n_delivered), with open_opcode the carried-in
 * message's opcode (0 = none; a stream's pending_opcode when its pending_bytes != 0) and
 * state_in its open sequence (NULL = zero; used only when open_opcode is TEXT).  What a
 * pipeline user calls on wait()'s host copies, and the reference of "device == host".
 * Returns 0, or -1 for NULL arguments (desc may be NULL when n_delivered is 0). */
int uvhttp_ws_utf8_judge_frames(const uint8_t* wire, uint64_t wire_len,
                                const uvhttp_ws_frame_desc_t* desc, uint32_t first_frame,
                                uint32_t n_delivered, int open_opcode,
                                const uvhttp_ws_utf8_state_t* state_in, uint32_t flags,
                                uvhttp_ws_utf8_conn_verdict_t* out);

/* ---- batched send-side framing ---------------------------------------------------------- */
/* One frame to build: uvhttp_ws_build_frame(ctx, buf, size, payload, len, opcode, mask, fin)
 * (src/uvhttp_websocket.c:204-285).  The reference draws a client's masking key from the
 * context DRBG (:257-266, host-side mbedtls); here the caller supplies it. */
typedef struct {
    uint64_t payload_off;  /* payload = src[payload_off, payload_off + payload_len) */
    uint64_t payload_len;
    uint32_t masking_key;  /* used when mask != 0; key bytes k0..k3, k0 = low byte */
    uint8_t opcode;        /* written as opcode & 0x0F */
    uint8_t fin;
    uint8_t mask;          /* 0: server frame (no key, payload copied); 1: client frame */
    uint8_t reserved0;
    uint64_t reserved1;
} uvhttp_ws_build_desc_t;  /* 32 bytes */

/* Build n frames back to back into d_out: frame i at d_out_off[i] (exclusive prefix sum of
 * the frame sizes, header 2/4/10 by payload length, +4 key bytes when masked); d_out_off[n]
 * = total bytes.  If the total exceeds out_cap nothing is written to d_out (d_out_off still
 * is, so the caller can size the buffer), like build_frame's buffer_size check. */
int uvhttp_ws_gpu_build_frames(uvhttp_ws_gpu_engine_t* eng, const uint8_t* d_src,
                               uint64_t src_len, const uvhttp_ws_build_desc_t* d_frames,
                               uint32_t n_frames, uint8_t* d_out, uint64_t out_cap,
                               uint64_t* d_out_off, void* stream);

/* ---- control replies: PONG and CLOSE echo built on the device after a decode ------------- */
/* The reply half of uvhttp_ws_process_data (src/uvhttp_websocket.c:1016-1084): every delivered
 * PING is answered with a PONG carrying the same payload, every delivered CLOSE is echoed.  The
 * host path does it one frame at a time through the control sink (uvhttp_ws_deliver_stream /
 * _deliver_batch); these calls build the same frames for a whole decoded batch where it lies in
 * device memory, in a layout uvhttp_tls_gpu_seal_frames takes as it is, so records in ->
 * decoded frames -> sealed replies out needs no host step.  build_frames cannot do it: it takes
 * a host-side frame count, and the number of replies is known only on the device.
 *
 * Which frames get a reply.  Connection s considers desc[first_frame, first_frame +
 * n_delivered), in descriptor order, when d_enable is NULL or d_enable[s] != 0 (d_enable stands
 * for conn->user_data != NULL with a server context behind it).  The streams form reads
 * first_frame and n_delivered from d_results[s] on the device, the in-place form n_delivered
 * from d_batch_summary (one connection, first_frame 0; after decode_inplace or decode_compact,
 * which both leave control payloads unmasked in the wire), so no host sync sits between decode
 * and replies.
 *   PING   a PONG with the ping's unmasked payload (0..125 bytes).
 *   CLOSE  a CLOSE with an empty payload when payload_len < 2, else payload[0, min(payload_len,
 *          127)): the code and the reason, as :1048-1066 copies them.
 *   Everything else gets nothing: data frames, PONG, failing / SKIPPED / INCOMPLETE frames,
 *   frames past a connection's first failure, descriptors at or past max_frames, and every
 *   frame of a connection whose result is ERR_CAPACITY, ERR_LAYOUT or ERR_DEVICE.
 * After a CLOSE.  The reference server's on_close frees the wrapper, so nothing after a
 * connection's first delivered CLOSE is answered: the default.  UVHTTP_WS_REPLY_AFTER_CLOSE
 * answers later PINGs and CLOSEs too (the bare library when on_close leaves user_data alone).
 *
 * Frame bytes.  Each reply is byte for byte what uvhttp_ws_build_frame(..., opcode, mask =
 * !is_server, fin = 1) writes (:204-285): a 2-byte header, and for a stream with is_server == 0
 * four key bytes and a masked payload.  Reply slot j (its index in this call's output) takes
 * its key from d_mask_keys[j] (k0 = low byte, as uvhttp_ws_build_desc_t.masking_key).
 * d_mask_keys (max_replies entries) may be NULL only when every stream is a server: a client
 * stream then gets no replies and status UVHTTP_WS_REPLY_NO_KEYS.
 *
 * Layout.  Replies lie back to back in d_out, connections in index order (as their descriptors
 * lie) and a connection's replies in frame order.  d_out_off[j] is the start of reply j, and
 * every entry from d_out_off[n_replies] to d_out_off[max_replies] equals the total: d_out /
 * d_out_off with n_frames_total = max_replies is a valid uvhttp_tls_gpu_seal_frames input as it
 * lies (frames past the real count have length 0 and give no record).  For connection s the
 * call writes two uint32_t, first_reply and n_replies, at (char*)d_runs + s * run_stride
 * (d_runs may be NULL): with a uvhttp_tls_send_t table whose seq, key and type are pre-filled,
 * pass &sends[0].first_frame and stride 32, then seal_frames with n_sends = n_streams; nothing
 * is read back (a send with n_frames = 0 succeeds with no record).  first_reply is the number of
 * replies of the connections before s, also when s has none.
 *
 * BAD_RANGE.  When a delivered PING or CLOSE of an enabled connection (answered or not) has a
 * reply payload that is not inside [0, wire_len), the connection gets status BAD_RANGE and no
 * replies.  Nothing outside the wire is read.
 *
 * Capacity.  If the replies exceed max_replies or their bytes exceed out_cap, nothing is written
 * to d_out, every d_out_off entry and every run is 0, every per-connection result has
 * first_reply, n_replies and out_len 0 and status ERR_CAPACITY, and the summary holds the totals
 * needed with status ERR_CAPACITY, so the caller can size and call again: the rule of
 * build_frames and seal_frames.
 *
 * All pointers are device pointers: d_wire 16-byte aligned, d_desc, d_streams, d_results,
 * d_batch_summary, d_out_off and d_summary 8, the rest 4 (d_out and d_enable 1).  EINVAL for NULL (d_enable,
 * d_mask_keys and d_runs excepted) or misaligned arguments, run_stride < 8 or not a multiple of 4
 * (with d_runs), max_frames or max_replies > 2^28, n_streams > 2^31 (without a device there is
 * no engine: uvhttp_ws_gpu_engine_create returns ENODEV and nothing is computed on the CPU).
 * Asynchronous on `stream` under the engine's stream rule.  The call keeps scratch in the engine
 * (12 bytes per descriptor, 32 per connection, no epoch tags), grown on demand:
 * graph-capturable once one uncaptured call of the same or a larger shape (max_frames,
 * n_streams) has been made; a captured call that would allocate fails with ENOMEM. */
#define UVHTTP_WS_REPLY_AFTER_CLOSE 0x1u  /* flags: keep answering after a connection's first CLOSE */

#define UVHTTP_WS_REPLY_OK 0
#define UVHTTP_WS_REPLY_ERR_CAPACITY 1  /* the whole call: max_replies or out_cap too small */
#define UVHTTP_WS_REPLY_BAD_RANGE 2     /* a PING / CLOSE payload range outside the wire */
#define UVHTTP_WS_REPLY_NO_KEYS 3       /* a client connection and d_mask_keys == NULL */

typedef struct {            /* 16 B, one per connection, device-written */
    uint32_t first_reply;   /* index of the connection's first reply in d_out_off */
    uint32_t n_replies;
    uint32_t out_len;       /* bytes of its replies (saturates at 2^32 - 1) */
    uint8_t status;         /* UVHTTP_WS_REPLY_* */
    uint8_t closed;         /* a CLOSE was delivered, whether answered or not */
    uint8_t reserved[2];
} uvhttp_ws_reply_conn_t;

typedef struct {            /* 32 B */
    uint64_t out_bytes;     /* bytes of d_out the call needs */
    uint32_t n_replies;     /* replies the call needs */
    uint32_t n_closed_conns;
    int32_t status;         /* UVHTTP_WS_REPLY_OK or UVHTTP_WS_REPLY_ERR_CAPACITY */
    uint32_t reserved[3];
} uvhttp_ws_reply_summary_t;

int uvhttp_ws_gpu_control_replies_streams(uvhttp_ws_gpu_engine_t* eng, const uint8_t* d_wire,
                                          uint64_t wire_len, const uvhttp_ws_frame_desc_t* d_desc,
                                          uint32_t max_frames, const uvhttp_ws_stream_t* d_streams,
                                          const uvhttp_ws_stream_result_t* d_results,
                                          uint32_t n_streams, const uint8_t* d_enable,
                                          const uint32_t* d_mask_keys, uint32_t flags,
                                          uint8_t* d_out, uint64_t out_cap, uint64_t* d_out_off,
                                          uint32_t max_replies, uint32_t* d_runs,
                                          uint32_t run_stride, uvhttp_ws_reply_conn_t* d_conn,
                                          uvhttp_ws_reply_summary_t* d_summary, void* stream);
int uvhttp_ws_gpu_control_replies_inplace(uvhttp_ws_gpu_engine_t* eng, const uint8_t* d_wire,
                                          uint64_t wire_len, const uvhttp_ws_frame_desc_t* d_desc,
                                          uint32_t n_frames,
                                          const uvhttp_ws_batch_summary_t* d_batch_summary,
                                          int32_t is_server, const uint32_t* d_mask_keys,
                                          uint32_t flags, uint8_t* d_out, uint64_t out_cap,
                                          uint64_t* d_out_off, uint32_t max_replies,
                                          uint32_t* d_runs, uint32_t run_stride,
                                          uvhttp_ws_reply_conn_t* d_conn,
                                          uvhttp_ws_reply_summary_t* d_summary, void* stream);
/* Host twin (plain C, host copies of the wire and descriptors): the same bytes and result for
 * one connection, desc[first_frame, first_frame + n_delivered); reply j of the connection
 * takes mask_keys[j] and starts at out_off[j] (out_off[0] = 0, max_replies + 1 entries, the
 * tail filled as above), first_reply is 0.  What a pipeline user calls on wait()'s host copies,
 * and the statement of "device == host".  On capacity nothing is written to out, out_off is
 * all 0 and the result holds the needed n_replies and out_len with status ERR_CAPACITY.
 * Returns 0, or -1 for NULL arguments (desc may be NULL when n_delivered is 0, mask_keys when
 * is_server, out when out_cap is 0). */
int uvhttp_ws_control_replies(const uint8_t* wire, uint64_t wire_len,
                              const uvhttp_ws_frame_desc_t* desc, uint32_t first_frame,
                              uint32_t n_delivered, int is_server, int enable,
                              const uint32_t* mask_keys, uint32_t flags, uint8_t* out,
                              uint64_t out_cap, uint64_t* out_off, uint32_t max_replies,
                              uvhttp_ws_reply_conn_t* conn_result);

/* ---- echo of data messages: the echo server's send built on the device after a decode ---- */
/* The reference's echo server (examples/05_websocket/websocket_echo_server.c) answers every data
 * message with the same bytes: on_message -> uvhttp_server_ws_send -> uvhttp_ws_send_text ->
 * uvhttp_ws_send_frame (src/uvhttp_websocket.c:509-608).  These calls build those frames for a
 * whole decoded batch where it lies in device memory, in the layout the control replies use, so
 * records in -> decoded frames -> sealed echoes out needs no host step.  build_frames cannot do
 * it: its frame count is a host argument and one frame has one contiguous source, while a
 * fragmented message lies in the wire as several payloads with headers, control frames and
 * possibly a read boundary between them, and its earlier bytes may have arrived in an earlier
 * call.
 *
 * Frames considered.  Connection s: desc[first_frame, first_frame + n_delivered), read from
 * d_results[s] on the device; the in-place form takes n_delivered from d_batch_summary (one
 * connection, first_frame 0, nothing carried in).  Frames at or past max_frames are skipped, as
 * is every frame of a connection whose result is ERR_CAPACITY, ERR_LAYOUT or ERR_DEVICE, and a
 * descriptor whose status is not OK.  A connection whose d_enable byte is 0 is skipped as a
 * whole: no echoes, open_len 0, status OK.
 *
 * Message membership is the rule uvhttp_ws_gpu_validate_utf8_streams states: a delivered frame
 * with opcode 1 or 2 starts a message; a delivered CONTINUATION belongs to the message the
 * nearest earlier delivered start frame of the connection began, or, when there is none, to the
 * carried-in message: opcode d_streams[s].pending_opcode, pending_bytes != 0.  FIN ends the
 * message (a CONTINUATION after it and before the next start frame belongs to nothing).  Control
 * frames in between contribute nothing.
 *
 * Which messages are echoed.  A message whose FIN frame is delivered gets ONE frame:
 * uvhttp_ws_build_frame(payload = all the message's bytes in order, carried bytes first, opcode =
 * the message's, mask = !is_server, fin = 1), with a header of 2, 4 or 10 bytes by the total
 * length; an empty message gets an empty frame.  With UVHTTP_WS_ECHO_SERVER_SEND the opcode is
 * always TEXT and an empty message gets nothing (uvhttp_server_ws_send, src/uvhttp_server.c:
 * 1057-1089).  A message whose FIN frame comes after the connection's first delivered CLOSE is
 * not echoed: process_data has set state = CLOSED (:1069) and send_frame refuses (:513).  Echo
 * slot j (its index in this call's output) of a client connection takes key d_mask_keys[j];
 * d_mask_keys (max_echoes entries) may be NULL only when every enabled stream is a server: a
 * client stream then gets status NO_KEYS.
 *
 * Carry.  d_carry_off has n_streams + 1 entries; connection s's carried bytes are
 * d_carry[d_carry_off[s], d_carry_off[s + 1]).  They are usable only when that length equals
 * d_streams[s].pending_bytes and the range lies inside carry_len (d_carry or d_carry_off NULL:
 * nothing is usable).  A connection with pending_bytes != 0 and no usable carry gets status
 * NO_CARRY.  After its last considered frame a connection's message may still be open; its bytes
 * so far — its carry, then its delivered fragments — are written back to back per connection
 * into d_open, connection s at d_open_off[s] (n_streams + 1 entries, the last the total): the
 * carry's own layout, so call k's (d_open, d_open_off, summary.open_bytes) are call k + 1's
 * (d_carry, d_carry_off, carry_len) as they lie, and open_opcode is the next pending_opcode.  A
 * connection that considers no frame passes its carry through.  d_open == NULL: open_len and
 * d_open_off are still written, no bytes are, and open_cap is not tested.  For an enabled
 * connection with status OK whose decode did not fail, open_len equals d_results[s].pending_bytes.
 *
 * Statuses.  NO_KEYS, else NO_CARRY, else BAD_RANGE: a delivered data frame (opcode 0, 1, 2) of
 * the connection with a payload range outside [0, wire_len).  A connection with any of them gets
 * no echoes and open_len 0; for NO_KEYS and NO_CARRY nothing is read for it, and nothing outside
 * the wire or the carry is ever read.
 *
 * Layout.  Echoes lie back to back in d_out, connections in index order and a connection's
 * echoes in frame order of their FIN frames.  d_out_off[j] is the start of echo j, and every
 * entry from d_out_off[n_echoes] to d_out_off[max_echoes] equals the total: d_out / d_out_off
 * with n_frames_total = max_echoes is a valid uvhttp_tls_gpu_seal_frames input as it lies.  For
 * connection s the call writes first_echo and n_echoes at (char*)d_runs + s * run_stride (d_runs
 * may be NULL), as the control replies write their runs; first_echo is the number of echoes of
 * the connections before s.
 *
 * Capacity.  If the echoes exceed max_echoes, their bytes out_cap or (with d_open) the open bytes
 * open_cap, nothing is written to d_out or d_open, every d_out_off and d_open_off entry and
 * every run is 0, every per-connection result is zero but for status ERR_CAPACITY, and the
 * summary holds the three totals needed with status ERR_CAPACITY.
 *
 * After decode_compact data payloads lie in the message arena: pass the arena (and its size) as
 * d_wire / wire_len of the in-place form; payload_off of data frames already points there.
 *
 * Order on one connection.  The reference interleaves echoes and control replies in frame order;
 * echo_messages and control_replies give two runs.  A caller who seals both sends a connection's
 * echo run before its control-reply run, so that a CLOSE echo stays last.  For the reference's
 * own order — one run, every answer where its frame stood — use
 * uvhttp_ws_gpu_answer_messages_streams / _inplace (below).
 *
 * All pointers are device pointers: d_wire, d_out, d_open and d_carry 16-byte aligned, d_desc,
 * d_streams, d_results, d_batch_summary, d_out_off, d_carry_off, d_open_off, d_conn and
 * d_summary 8, the rest 4 (d_enable 1).  EINVAL for NULL (d_enable, d_mask_keys, d_runs, d_carry,
 * d_carry_off and d_open excepted) or misaligned arguments, run_stride < 8 or not a multiple of
 * 4 (with d_runs), max_frames or max_echoes > 2^28, n_streams > 2^31.  Asynchronous on `stream`
 * under the engine's stream rule.  Scratch lives in the engine (28 bytes per descriptor, 120 per
 * connection, 64 per echo slot, 4 per 64 KiB of out_cap and of open_cap, no epoch tags), grown on
 * demand: graph-capturable once one uncaptured call of the same or a larger shape (max_frames,
 * n_streams, max_echoes, out_cap, open_cap) has been made; a captured call that would allocate
 * fails with ENOMEM. */
#define UVHTTP_WS_ECHO_SERVER_SEND 0x1u  /* flags: as uvhttp_server_ws_send: every echo is a TEXT
                                            frame, empty messages get none */
#define UVHTTP_WS_ECHO_OK 0
#define UVHTTP_WS_ECHO_ERR_CAPACITY 1    /* the whole call: max_echoes, out_cap or open_cap too small */
#define UVHTTP_WS_ECHO_BAD_RANGE 2       /* a data payload of the connection lies outside the wire */
#define UVHTTP_WS_ECHO_NO_KEYS 3         /* a client connection and d_mask_keys == NULL */
#define UVHTTP_WS_ECHO_NO_CARRY 4        /* pending_bytes != 0 and no usable carried bytes */

typedef struct {            /* 32 B, one per connection, device-written */
    uint32_t first_echo;    /* index of the connection's first echo in d_out_off */
    uint32_t n_echoes;
    uint64_t out_len;       /* bytes of its echo frames */
    uint64_t open_len;      /* bytes of the message still open after its last considered frame */
    uint8_t status;         /* UVHTTP_WS_ECHO_* */
    uint8_t open_opcode;    /* that message's opcode (0 when open_len is 0) */
    uint8_t reserved[6];
} uvhttp_ws_echo_conn_t;

typedef struct {            /* 32 B */
    uint64_t out_bytes;     /* bytes of d_out the call needs */
    uint64_t open_bytes;    /* bytes of d_open the call needs */
    uint32_t n_echoes;      /* echoes the call needs */
    int32_t status;         /* UVHTTP_WS_ECHO_OK or UVHTTP_WS_ECHO_ERR_CAPACITY */
    uint32_t reserved[2];
} uvhttp_ws_echo_summary_t;

int uvhttp_ws_gpu_echo_messages_streams(uvhttp_ws_gpu_engine_t* eng, const uint8_t* d_wire,
                                        uint64_t wire_len, const uvhttp_ws_frame_desc_t* d_desc,
                                        uint32_t max_frames, const uvhttp_ws_stream_t* d_streams,
                                        const uvhttp_ws_stream_result_t* d_results,
                                        uint32_t n_streams, const uint8_t* d_enable,
                                        const uint32_t* d_mask_keys, uint32_t flags,
                                        const uint8_t* d_carry, uint64_t carry_len,
                                        const uint64_t* d_carry_off, uint8_t* d_out,
                                        uint64_t out_cap, uint64_t* d_out_off, uint32_t max_echoes,
                                        uint32_t* d_runs, uint32_t run_stride, uint8_t* d_open,
                                        uint64_t open_cap, uint64_t* d_open_off,
                                        uvhttp_ws_echo_conn_t* d_conn,
                                        uvhttp_ws_echo_summary_t* d_summary, void* stream);
int uvhttp_ws_gpu_echo_messages_inplace(uvhttp_ws_gpu_engine_t* eng, const uint8_t* d_wire,
                                        uint64_t wire_len, const uvhttp_ws_frame_desc_t* d_desc,
                                        uint32_t n_frames,
                                        const uvhttp_ws_batch_summary_t* d_batch_summary,
                                        int32_t is_server, const uint32_t* d_mask_keys,
                                        uint32_t flags, uint8_t* d_out, uint64_t out_cap,
                                        uint64_t* d_out_off, uint32_t max_echoes, uint32_t* d_runs,
                                        uint32_t run_stride, uint8_t* d_open, uint64_t open_cap,
                                        uint64_t* d_open_off, uvhttp_ws_echo_conn_t* d_conn,
                                        uvhttp_ws_echo_summary_t* d_summary, void* stream);
/* Host twin (plain C, host copies): the same bytes and result for one connection,
 * desc[first_frame, first_frame + n_delivered), with the carried-in message (pending_opcode,
 * pending_bytes) and its bytes carry[0, carry_len), usable when carry_len == pending_bytes.
 * Echo j of the connection takes mask_keys[j] and starts at out_off[j] (max_echoes + 1 entries,
 * the tail filled as above), first_echo is 0; the open message goes to open[0, open_len) (open
 * may be NULL: open_len is still reported, open_cap is not tested).  The statement of the rules:
 * "device == host".  On capacity nothing is written to out or open, out_off is all 0 and the
 * result holds the needed n_echoes, out_len and open_len with status ERR_CAPACITY.  Returns 0,
 * or -1 for NULL arguments (desc may be NULL when n_delivered is 0, mask_keys when is_server,
 * out when out_cap is 0, carry when carry_len is 0). */
int uvhttp_ws_echo_messages(const uint8_t* wire, uint64_t wire_len,
                            const uvhttp_ws_frame_desc_t* desc, uint32_t first_frame,
                            uint32_t n_delivered, int is_server, int enable,
                            const uint32_t* mask_keys, uint32_t flags, int pending_opcode,
                            uint64_t pending_bytes, const uint8_t* carry, uint64_t carry_len,
                            uint8_t* out, uint64_t out_cap, uint64_t* out_off,
                            uint32_t max_echoes, uint8_t* open, uint64_t open_cap,
                            uvhttp_ws_echo_conn_t* conn_result);

/* ---- answers: echoes and control replies of a batch in one run, in frame order -------------- */
/* uvhttp_ws_process_data answers as it goes (src/uvhttp_websocket.c:1016-1084): a PING gets its
 * PONG when it is processed, a message its echo when its FIN frame is, and the CLOSE echo comes
 * where the CLOSE stood.  These calls build that one sequence for a whole decoded batch: a
 * connection's run opens to exactly the bytes uvhttp_ws_send_frame would have been handed, in
 * order.  They take echo_messages_streams' (_inplace's) arguments, argument for argument, with
 * max_answers for max_echoes, the structs below for d_conn and d_summary, and one optional output,
 * d_reply_conn.
 *
 * Rule, per connection.  Over the considered descriptors desc[first_frame, first_frame +
 * n_delivered), clipped and skipped exactly as echo_messages does it, in descriptor order:
 *   the FIN frame of an echoed message gives that message's echo frame: the bytes echo_messages
 *     builds, with its membership, carry, after-first-CLOSE and SERVER_SEND rules;
 *   a delivered PING gives a PONG and a delivered CLOSE its CLOSE echo: the bytes
 *     control_replies builds (an empty CLOSE for payload_len < 2).  Nothing after the first
 *     delivered CLOSE is answered unless UVHTTP_WS_ANSWER_REPLY_AFTER_CLOSE is set;
 *   every other frame gives nothing.
 * A connection's output is therefore the stable merge, by source descriptor index, of the two
 * calls' outputs for it.  Echoes after the first CLOSE are never sent, whatever the flag; by
 * default the CLOSE echo is the connection's last answer.
 *
 * Keys.  Answer slot j (its index in this call's output) of a client connection takes
 * d_mask_keys[j] (max_answers entries; NULL only when every enabled stream is a server).
 *
 * Statuses are the echo's values, checked in this order: NO_KEYS, NO_CARRY, BAD_RANGE — a
 * delivered data frame, or a delivered PING or CLOSE whether answered or not, whose payload range
 * (for a control frame: the reply's payload) lies outside [0, wire_len).  A connection with any of
 * them gets no answers at all and open_len 0, and nothing outside the wire or the carry is read
 * for it.  This is stricter than the two calls run apart: there NO_CARRY or a bad data range
 * leaves the control replies standing, and a bad control range the echoes.
 *
 * Layout: the builders' convention.  Answers lie back to back in d_out, connections in index
 * order; d_out_off has max_answers + 1 entries, the tail filled with the total; (first_answer,
 * n_answers) goes to (char*)d_runs + s * run_stride; the open messages go to d_open / d_open_off
 * as the next call's carry.  Capacity is the echo's rule: nothing is written, all offsets and runs
 * are 0, every per-connection result is zero but for status ERR_CAPACITY, and the summary holds the
 * totals needed (n_answers, n_replies, out_bytes, open_bytes, n_closed_conns).
 *
 * d_reply_conn (may be NULL) receives per connection what close_frames_streams reads, so that it
 * runs after this call unchanged: closed as control_replies defines it (a CLOSE was delivered,
 * answered or not, enabled or not, also on capacity), n_replies, out_len = the bytes of its replies
 * (saturating), first_reply 0, and status REPLY_OK, or ERR_CAPACITY / BAD_RANGE / NO_KEYS when that
 * is the connection's answer status (NO_CARRY reads REPLY_OK with no replies).
 *
 * The in-place form after decode_compact: data payloads lie in the arena and control payloads
 * stay in the wire, and the call takes one d_wire.  Pass the arena only for a batch whose PINGs and
 * CLOSEs carry no payload; otherwise use decode_inplace, or the two calls with a buffer each.
 *
 * EINVAL rules (and flags outside the two below), alignment (d_reply_conn 4), the stream rule and
 * the graph-capture rule are echo_messages'.  Engine scratch is the echo's, sized by max_answers,
 * plus 16 bytes per connection and 8 per 256 descriptors. */
#define UVHTTP_WS_ANSWER_SERVER_SEND 0x1u        /* flags: UVHTTP_WS_ECHO_SERVER_SEND's rule */
#define UVHTTP_WS_ANSWER_REPLY_AFTER_CLOSE 0x2u  /* flags: UVHTTP_WS_REPLY_AFTER_CLOSE's rule */

typedef struct {            /* 32 B, one per connection, device-written */
    uint32_t first_answer;  /* index of the connection's first answer in d_out_off */
    uint32_t n_answers;
    uint64_t out_len;       /* bytes of its answer frames */
    uint64_t open_len;      /* bytes of the message still open after its last considered frame */
    uint8_t status;         /* UVHTTP_WS_ECHO_* */
    uint8_t open_opcode;    /* that message's opcode (0 when open_len is 0) */
    uint8_t closed;         /* a CLOSE was delivered, whether answered or not */
    uint8_t reserved;
    uint32_t n_replies;     /* the PONGs and CLOSE echoes among its answers */
} uvhttp_ws_answer_conn_t;

typedef struct {            /* 32 B */
    uint64_t out_bytes;     /* bytes of d_out the call needs */
    uint64_t open_bytes;    /* bytes of d_open the call needs */
    uint32_t n_answers;     /* answers the call needs */
    uint32_t n_replies;     /* ... of which PONGs and CLOSE echoes */
    uint32_t n_closed_conns;
    int32_t status;         /* UVHTTP_WS_ECHO_OK or UVHTTP_WS_ECHO_ERR_CAPACITY */
} uvhttp_ws_answer_summary_t;

int uvhttp_ws_gpu_answer_messages_streams(uvhttp_ws_gpu_engine_t* eng, const uint8_t* d_wire,
                                          uint64_t wire_len, const uvhttp_ws_frame_desc_t* d_desc,
                                          uint32_t max_frames, const uvhttp_ws_stream_t* d_streams,
                                          const uvhttp_ws_stream_result_t* d_results,
                                          uint32_t n_streams, const uint8_t* d_enable,
                                          const uint32_t* d_mask_keys, uint32_t flags,
                                          const uint8_t* d_carry, uint64_t carry_len,
                                          const uint64_t* d_carry_off, uint8_t* d_out,
                                          uint64_t out_cap, uint64_t* d_out_off, uint32_t max_answers,
                                          uint32_t* d_runs, uint32_t run_stride, uint8_t* d_open,
                                          uint64_t open_cap, uint64_t* d_open_off,
                                          uvhttp_ws_answer_conn_t* d_conn,
                                          uvhttp_ws_answer_summary_t* d_summary,
                                          uvhttp_ws_reply_conn_t* d_reply_conn, void* stream);
int uvhttp_ws_gpu_answer_messages_inplace(uvhttp_ws_gpu_engine_t* eng, const uint8_t* d_wire,
                                          uint64_t wire_len, const uvhttp_ws_frame_desc_t* d_desc,
                                          uint32_t n_frames,
                                          const uvhttp_ws_batch_summary_t* d_batch_summary,
                                          int32_t is_server, const uint32_t* d_mask_keys,
                                          uint32_t flags, uint8_t* d_out, uint64_t out_cap,
                                          uint64_t* d_out_off, uint32_t max_answers, uint32_t* d_runs,
                                          uint32_t run_stride, uint8_t* d_open, uint64_t open_cap,
                                          uint64_t* d_open_off, uvhttp_ws_answer_conn_t* d_conn,
                                          uvhttp_ws_answer_summary_t* d_summary,
                                          uvhttp_ws_reply_conn_t* d_reply_conn, void* stream);
/* Host twin (plain C, host copies): one connection, first_answer 0, answer j takes mask_keys[j];
 * the arguments are uvhttp_ws_echo_messages' with max_answers and the optional reply_conn.  The
 * statement of the rule: "device == host" in every output.  On capacity nothing is written to out
 * or open, out_off is all 0 and the result holds the needed n_answers, n_replies, out_len and
 * open_len with status ERR_CAPACITY.  Returns 0, or -1 for the arguments uvhttp_ws_echo_messages
 * refuses and for unknown flags. */
int uvhttp_ws_answer_messages(const uint8_t* wire, uint64_t wire_len,
                              const uvhttp_ws_frame_desc_t* desc, uint32_t first_frame,
                              uint32_t n_delivered, int is_server, int enable,
                              const uint32_t* mask_keys, uint32_t flags, int pending_opcode,
                              uint64_t pending_bytes, const uint8_t* carry, uint64_t carry_len,
                              uint8_t* out, uint64_t out_cap, uint64_t* out_off,
                              uint32_t max_answers, uint8_t* open, uint64_t open_cap,
                              uvhttp_ws_answer_conn_t* conn_result,
                              uvhttp_ws_reply_conn_t* reply_conn);

/* ---- relay of data messages: the room server's broadcast built on the device after a decode - */
/* The reference's other send path is uvhttp_server_ws_broadcast (src/uvhttp_server.c:1626-1657):
 * every OPEN connection registered on a path gets the message as one TEXT frame; called from
 * on_message it is the chat / pub-sub server.  This call builds, for a whole decoded batch, the
 * frames of all messages completed in the batch grouped by room, and names every receiver its
 * room's run where uvhttp_tls_gpu_seal_frames reads it ("one built frame, N sends with N keys"),
 * so open_records -> ws_streams -> decode_reads -> relay_messages (+ control_replies) ->
 * seal_frames needs no host read.  The fan-out costs no frame bytes: every member of a room names
 * the same run.
 *
 * Frames considered, message membership, carry-in, NO_CARRY, which messages qualify (the FIN
 * frame delivered, and not after the sender's first delivered CLOSE: a peer that sent CLOSE sends
 * no more data, RFC 6455 section 5.5.1, and a room has one frame list), BAD_RANGE, d_enable and
 * UVHTTP_WS_ECHO_SERVER_SEND are uvhttp_ws_gpu_echo_messages_streams' (above).  Under SERVER_SEND
 * every frame is TEXT and an empty message gets none: uvhttp_server_ws_broadcast's send_text and
 * its len == 0 refusal.
 *
 * Server frames.  A relayed frame is uvhttp_ws_build_frame(..., mask = 0, fin = 1), one per
 * message, with a header of 2, 4 or 10 bytes; the sender's is_server plays no part, there is no
 * key table and no NO_KEYS.
 *
 * Open messages.  d_open / d_open_off / open_len / open_opcode are per sender in connection
 * index order, byte for byte what the echo writes: call k's open buffer is call k + 1's carry,
 * whatever the rooms are.
 *
 * Rooms.  d_room[s] < n_rooms is sender s's room.  An enabled connection with d_room[s] >=
 * n_rooms gets status UVHTTP_WS_RELAY_BAD_ROOM: no frames, open_len 0, counted in n_bad_rooms.
 * The statuses rank NO_CARRY, else BAD_ROOM, else BAD_RANGE.
 *
 * Order.  Frames lie back to back in d_out ordered by (room, sender's connection index, frame
 * order of the FIN frames).  d_out_off[j] starts frame j, and every entry from d_out_off[n_frames]
 * to d_out_off[max_frames_out] equals the total: d_out / d_out_off with n_frames_total =
 * max_frames_out is a valid uvhttp_tls_gpu_seal_frames input as it lies.  d_rooms[r] holds room
 * r's run and byte range; a room with no frame gets n_frames 0, first_frame = the frames of the
 * rooms before it, out_off = their bytes, out_len 0.  d_conn[s].first_echo / n_echoes / out_len
 * name sender s's own frames inside that order; a connection with no frame gets first_echo = the
 * frames before its place when all connections are ordered by (min(d_room[s], n_rooms), s).
 *
 * Receivers.  Receiver k gets d_rooms[d_recv_room[k]].first_frame and .n_frames at (char*)d_sends
 * + k * send_stride: &sends[0].first_frame with stride sizeof(uvhttp_tls_send_t).  Every member
 * is named, the sender included, as the reference's broadcast does; receivers need not be senders
 * and senders need not be receivers.  d_recv_room[k] >= n_rooms gives (0, 0) and counts in
 * n_bad_receivers.  d_sends and d_recv_room may be NULL with n_receivers = 0.
 *
 * Capacity, as for the echo: if the frames exceed max_frames_out, their bytes out_cap or (with
 * d_open) the open bytes open_cap, nothing is written to d_out or d_open, all offsets, room
 * entries and receiver runs are 0, every per-connection result is zero but for status
 * ERR_CAPACITY, and the summary holds the three totals needed with status ERR_CAPACITY
 * (n_bad_rooms and n_bad_receivers are counted either way).
 *
 * Pointers and alignment as for the echo; d_room, d_recv_room and d_sends 4, d_rooms 8.  EINVAL
 * for NULL (d_enable, d_carry, d_carry_off and d_open excepted; d_rooms only with n_rooms = 0) or
 * misaligned arguments, max_frames or max_frames_out > 2^28, n_streams > 2^31, n_rooms > 2^28,
 * send_stride < 8 or not a multiple of 4; ENODEV without a device.  Asynchronous on `stream`
 * under the engine's stream rule.  Scratch lives in the engine, shared with the echo (28 bytes
 * per descriptor, 168 per connection, none per room, 64 per output slot, 4 per 64 KiB of out_cap
 * and of open_cap, no epoch tags), grown on demand: graph-capturable once one uncaptured call of
 * the same or a larger shape has been made; a captured call that would allocate fails with
 * ENOMEM.  There is no in-place form: one connection has nobody to relay to. */
#define UVHTTP_WS_RELAY_BAD_ROOM 5       /* per connection, beside UVHTTP_WS_ECHO_*: d_room[s] >= n_rooms */

typedef struct {            /* 32 B, one per room, device-written */
    uint32_t first_frame;   /* index of the room's first frame in d_out_off */
    uint32_t n_frames;
    uint64_t out_off;       /* its frames are d_out[out_off, out_off + out_len) */
    uint64_t out_len;
    uint64_t reserved;
} uvhttp_ws_relay_room_t;

typedef struct {            /* 32 B */
    uint64_t out_bytes;     /* bytes of d_out the call needs */
    uint64_t open_bytes;    /* bytes of d_open the call needs */
    uint32_t n_frames;      /* frames the call needs */
    int32_t status;         /* UVHTTP_WS_ECHO_OK or UVHTTP_WS_ECHO_ERR_CAPACITY */
    uint32_t n_bad_rooms;   /* enabled connections with status BAD_ROOM */
    uint32_t n_bad_receivers;
} uvhttp_ws_relay_summary_t;

int uvhttp_ws_gpu_relay_messages_streams(uvhttp_ws_gpu_engine_t* eng, const uint8_t* d_wire,
                                         uint64_t wire_len, const uvhttp_ws_frame_desc_t* d_desc,
                                         uint32_t max_frames, const uvhttp_ws_stream_t* d_streams,
                                         const uvhttp_ws_stream_result_t* d_results,
                                         uint32_t n_streams, const uint8_t* d_enable,
                                         const uint32_t* d_room, uint32_t n_rooms, uint32_t flags,
                                         const uint8_t* d_carry, uint64_t carry_len,
                                         const uint64_t* d_carry_off, uint8_t* d_out,
                                         uint64_t out_cap, uint64_t* d_out_off,
                                         uint32_t max_frames_out, uvhttp_ws_relay_room_t* d_rooms,
                                         const uint32_t* d_recv_room, uint32_t n_receivers,
                                         uint32_t* d_sends, uint32_t send_stride, uint8_t* d_open,
                                         uint64_t open_cap, uint64_t* d_open_off,
                                         uvhttp_ws_echo_conn_t* d_conn,
                                         uvhttp_ws_relay_summary_t* d_summary, void* stream);
/* Host twin (plain C, host copies of the same tables): all connections of the call at once and
 * the same outputs, byte for byte; the statement of the rules.  Returns 0, or -1 for NULL
 * arguments (as above; desc may be NULL when max_frames is 0, out when out_cap is 0) or when it
 * cannot allocate its temporaries. */
int uvhttp_ws_relay_messages(const uint8_t* wire, uint64_t wire_len,
                             const uvhttp_ws_frame_desc_t* desc, uint32_t max_frames,
                             const uvhttp_ws_stream_t* streams,
                             const uvhttp_ws_stream_result_t* results, uint32_t n_streams,
                             const uint8_t* enable, const uint32_t* room, uint32_t n_rooms,
                             uint32_t flags, const uint8_t* carry, uint64_t carry_len,
                             const uint64_t* carry_off, uint8_t* out, uint64_t out_cap,
                             uint64_t* out_off, uint32_t max_frames_out,
                             uvhttp_ws_relay_room_t* rooms, const uint32_t* recv_room,
                             uint32_t n_receivers, uint32_t* sends, uint32_t send_stride,
                             uint8_t* open, uint64_t open_cap, uint64_t* open_off,
                             uvhttp_ws_echo_conn_t* conn, uvhttp_ws_relay_summary_t* summary);

/* ---- the server's own CLOSE frames: 1002 after a failed decode, 1007 after invalid UTF-8 ---- */
/* When a process_data call fails, on_websocket_read closes the WebSocket itself:
 * uvhttp_ws_close(NULL, ws_conn, 1002, "protocol error") (src/uvhttp_connection.c:1166-1174,
 * src/uvhttp_websocket.c:627-666), one CLOSE frame built by uvhttp_ws_build_frame(opcode 8, mask =
 * !is_server, fin 1).  This pass builds those frames for a whole decoded batch, and the 1007
 * close the UTF-8 verdicts exist for (RFC 6455 §7.4.1, §8.1), in the layout of the control
 * replies, so they are one more part of the batch's send (uvhttp_tls_gpu_seal_parts) and a CLOSE
 * is the last frame of its connection's send by construction.  One lane per connection; no
 * descriptor and no wire byte is read.
 *
 * Rule, per connection s.  No frame if d_enable is given and d_enable[s] == 0; if
 * d_results[s].first_status is ERR_CAPACITY, ERR_LAYOUT or ERR_DEVICE (the call failed, not the
 * peer); or if d_reply_conn is given and d_reply_conn[s].closed is set (the reference's send_frame
 * refuses once the state has left OPEN, and the CLOSE echo already closes the connection).
 * Otherwise, if d_verdict is given and d_verdict[s].status is UVHTTP_WS_UTF8_INVALID: code 1007
 * with an empty reason — this project's choice, the reference never checks; it wins over a decode
 * failure, because first_invalid is a delivered frame and so precedes the failing one.  Otherwise,
 * if first_status < 0: code 1002 with the reason "protocol error", byte for byte the reference's
 * frame.  Everything else (BAD_RANGE included: a caller error) gives no frame.  A client stream
 * (is_server == 0) masks its frame with d_mask_keys[s] (k0 = low byte); when d_mask_keys is NULL
 * it gets no frame and status UVHTTP_WS_CLOSE_NO_KEYS.
 *
 * Layout.  Frames lie back to back in d_out in connection order; d_out_off has n_streams + 1
 * entries, d_out_off[j] the start of frame j and every entry from the frame count on the total:
 * a valid frame table with n_frames = n_streams.  Connection s's run (closes of the connections
 * before it, then 0 or 1) goes to (char*)d_runs + s * run_stride (d_runs may be NULL).
 *
 * d_clear_runs (a host array of n_clear <= 4 device pointers, strides clear_stride[k]): for a
 * connection that gets the 1007 close the pass writes n_frames = 0 into the second word of its
 * run in each of those tables.  Pass the connection's echo and reply runs and it is failed per RFC
 * 6455 §7.1.7 with nothing but the close.  Stream order: the pass must run after the passes that
 * write those tables, and before the seal that reads them.
 *
 * Capacity, the replies' rule: if the bytes exceed out_cap nothing is written to d_out, every
 * d_out_off entry and run is 0, no run is cleared, every per-connection result is zero but for
 * status ERR_CAPACITY, and the summary holds the totals needed with status ERR_CAPACITY.
 *
 * Device pointers: d_streams, d_results, d_out_off and d_summary 8-byte aligned, the others 4
 * (d_out, d_enable 1).  EINVAL for NULL (d_verdict, d_reply_conn, d_enable, d_mask_keys, d_runs
 * and d_clear_runs excepted) or misaligned arguments, a run or clear stride < 8 or not a multiple
 * of 4, n_clear > 4, flags != 0, n_streams > 2^31.  Asynchronous on `stream` under the engine's
 * stream rule; 16 bytes of engine scratch per 256 connections, grown on demand: graph-capturable
 * once one uncaptured call of the same or a larger n_streams has been made. */
#define UVHTTP_WS_CLOSE_OK 0
#define UVHTTP_WS_CLOSE_ERR_CAPACITY 1  /* the whole call: out_cap too small */
#define UVHTTP_WS_CLOSE_NO_KEYS 3       /* a client connection to close and d_mask_keys == NULL */
#define UVHTTP_WS_CLOSE_MAX_CLEAR 4

typedef struct {            /* 16 B, one per connection, device-written */
    uint32_t code;          /* 1002, 1007, or 0: no frame */
    uint32_t out_len;       /* bytes of its frame */
    uint8_t status;         /* UVHTTP_WS_CLOSE_* */
    uint8_t reserved[7];
} uvhttp_ws_close_conn_t;

typedef struct {            /* 32 B */
    uint64_t out_bytes;     /* bytes of d_out the call needs */
    uint32_t n_closes;      /* n_1002 + n_1007 */
    uint32_t n_1002;
    uint32_t n_1007;
    int32_t status;         /* UVHTTP_WS_CLOSE_OK or UVHTTP_WS_CLOSE_ERR_CAPACITY */
    uint32_t reserved[2];
} uvhttp_ws_close_summary_t;

int uvhttp_ws_gpu_close_frames_streams(uvhttp_ws_gpu_engine_t* eng, const uvhttp_ws_stream_t* d_streams,
                                       const uvhttp_ws_stream_result_t* d_results, uint32_t n_streams,
                                       const uvhttp_ws_utf8_conn_verdict_t* d_verdict,
                                       const uvhttp_ws_reply_conn_t* d_reply_conn,
                                       const uint8_t* d_enable, const uint32_t* d_mask_keys,
                                       uint32_t flags, uint8_t* d_out, uint64_t out_cap,
                                       uint64_t* d_out_off, uint32_t* d_runs, uint32_t run_stride,
                                       uint32_t* const* d_clear_runs, const uint32_t* clear_stride,
                                       uint32_t n_clear, uvhttp_ws_close_conn_t* d_conn,
                                       uvhttp_ws_close_summary_t* d_summary, void* stream);
/* Host twin (plain C, host copies of the same tables): all connections of the call at once and
 * the same outputs, byte for byte; the statement of the rule.  Returns 0, or -1 for an argument
 * the device call answers with EINVAL. */
int uvhttp_ws_close_frames(const uvhttp_ws_stream_t* streams, const uvhttp_ws_stream_result_t* results,
                           uint32_t n_streams, const uvhttp_ws_utf8_conn_verdict_t* verdict,
                           const uvhttp_ws_reply_conn_t* reply_conn, const uint8_t* enable,
                           const uint32_t* mask_keys, uint32_t flags, uint8_t* out, uint64_t out_cap,
                           uint64_t* out_off, uint32_t* runs, uint32_t run_stride,
                           uint32_t* const* clear_runs, const uint32_t* clear_stride, uint32_t n_clear,
                           uvhttp_ws_close_conn_t* conn, uvhttp_ws_close_summary_t* summary);

/* ---- fail points: stop a connection at its first violation ---------------------------------- */
/* One pass between the judging (decode, validate_utf8_streams) and the sends (echo_messages or
 * relay_messages, control_replies, close_frames).  It finds the frame at which a server that
 * follows RFC 6455 §7.1.7 fails each connection, and rewrites the two outcome tables into what
 * that server would have seen had the decode stopped there.  The send passes then run unchanged
 * on the rewritten tables: a failed connection sends its echoes and replies before the violation
 * and then its close; a bad CLOSE is not echoed (`closed` stays 0, so close_frames sends the
 * 1002); an invalid sender's message never enters its room; no PING after the cut gets a PONG.
 *
 * Considered frames of connection s: desc[first_frame, first_frame + n_delivered), clipped to
 * max_frames as the echo clips them.  c = the first considered CLOSE with status OK, if any.
 *
 * CLOSE violation (only with UVHTTP_WS_FAIL_CHECK_CLOSE, only frame c; RFC 6455 §7.4, the
 * reference checks neither): payload_len == 1 is reason CLOSE_LEN; payload_len >= 2 with an
 * invalid big-endian code in payload[0, 2) is reason CLOSE_CODE.  Valid codes are 1000-1003,
 * 1007-1014 and 3000-4999: RFC 6455 §7.4.1-2 plus the IANA-registered 1012-1014, this project's
 * choice.  Either reason fails the connection with 1002 at frame c.  If frame c has payload_len >=
 * 2 and its payload range is not inside [0, wire_len), the connection gets status
 * UVHTTP_WS_FAIL_BAD_RANGE (a caller error): reason NONE, no cut, both tables copied as they are.
 * Nothing outside the wire is read, and only those 2 bytes of one frame per connection ever are.
 * UTF-8 violation: d_verdict[s].status == UVHTTP_WS_UTF8_INVALID, u = first_invalid is a
 * considered frame and u <= c (or there is no c): 1007 at frame u, reason UTF8.  A violation after
 * the first delivered CLOSE is no failure: the server stopped at the CLOSE (what close_frames
 * expresses through `closed`).
 * Precedence: the earlier frame wins; on the same frame (a CLOSE with a bad code and a reason
 * that is not UTF-8) 1002 wins.
 * Decode failure: no cut and first_status < 0: reason DECODE, code 1002, frame = first_frame +
 * n_delivered.  Nothing is rewritten, the decode already stopped there.
 * Not judged: connections with d_enable[s] == 0 and connections whose result is ERR_CAPACITY,
 * ERR_LAYOUT or ERR_DEVICE are copied unchanged, reason NONE.
 *
 * A cut at frame k.  d_results_out[s] is a copy with n_delivered = k - first_frame, n_frames =
 * n_delivered + 1, status = UVHTTP_ERROR_INVALID_PARAM and first_status = UVHTTP_WS_FRAME_ERR_UTF8
 * or UVHTTP_WS_FRAME_ERR_CLOSE; every other field (consumed_bytes, pending_bytes, ... of the whole
 * decode) is copied.  d_verdict_out[s] is a copy, except that a connection cut by a CLOSE
 * violation at or before its first_invalid, or (cut or not) whose first_invalid lies after c, gets
 * status VALID, first_invalid 0xFFFFFFFF and a zero state, the verdict over the kept frames
 * (n_text_frames is copied).  d_fail[s] names the frame, the code, the reason, and n_dropped = the
 * considered frames at or after the cut.  close_frames over the rewritten tables sends
 * d_fail[s].code: 1007 for first_status ERR_UTF8 (the verdict stays INVALID), 1002 for ERR_CLOSE.
 *
 * One wart.  The echo reports the bytes of the cut message's earlier fragments as "open"; that
 * carry is dropped with the connection, as a session driver drops any leaver's carry.
 * Out of scope: uvhttp_ws_deliver_stream keeps taking the ORIGINAL d_results; host delivery from
 * the rewritten table is not supported (its consumed_bytes / pending_bytes are the whole decode's).
 *
 * d_results_out may be d_results and d_verdict_out may be d_verdict (in place); any other overlap
 * is unspecified.  d_verdict and d_verdict_out are both given or both NULL; d_enable may be NULL.
 * Device pointers: d_desc, d_results, d_results_out and d_summary 8-byte aligned, the others 4
 * (d_wire, d_enable 1).  EINVAL for NULL or misaligned arguments, unknown flags, max_frames > 2^28,
 * n_streams > 2^31.  Asynchronous on `stream` under the engine's stream rule; 4 bytes of engine
 * scratch per descriptor and per connection, grown on demand: graph-capturable once one uncaptured
 * call of the same or a larger shape has been made.  Reads one 32-byte descriptor per frame, one
 * 64 + 16-byte entry per connection and 2 wire bytes per closing connection. */
#define UVHTTP_WS_FRAME_ERR_UTF8 (-12)   /* first_status of a connection cut at invalid UTF-8 */
#define UVHTTP_WS_FRAME_ERR_CLOSE (-13)  /* ... at a CLOSE with a 1-byte payload or a bad code */

#define UVHTTP_WS_FAIL_CHECK_CLOSE 0x1u  /* flags: judge the first CLOSE's payload length and code */

#define UVHTTP_WS_FAIL_OK 0
#define UVHTTP_WS_FAIL_BAD_RANGE 2       /* the first CLOSE's payload range lies outside the wire */

#define UVHTTP_WS_FAIL_NONE 0            /* reasons */
#define UVHTTP_WS_FAIL_DECODE 1
#define UVHTTP_WS_FAIL_UTF8 2
#define UVHTTP_WS_FAIL_CLOSE_LEN 3
#define UVHTTP_WS_FAIL_CLOSE_CODE 4

typedef struct {            /* 16 B, one per connection, device-written */
    uint32_t frame;         /* desc index (absolute) of the fail point, 0xFFFFFFFF if none */
    uint32_t n_dropped;     /* considered frames at or after a cut (0 for DECODE) */
    uint16_t code;          /* 0, 1002 or 1007 */
    uint8_t reason;         /* UVHTTP_WS_FAIL_NONE / DECODE / UTF8 / CLOSE_LEN / CLOSE_CODE */
    uint8_t status;         /* UVHTTP_WS_FAIL_OK or UVHTTP_WS_FAIL_BAD_RANGE */
    uint32_t reserved;
} uvhttp_ws_fail_conn_t;

typedef struct {            /* 32 B */
    uint64_t n_dropped;     /* sum over the connections */
    uint32_t n_decode;      /* connections per reason */
    uint32_t n_utf8;
    uint32_t n_close_len;
    uint32_t n_close_code;
    uint32_t n_bad_range;   /* connections with status BAD_RANGE */
    uint32_t first_failed;  /* lowest connection with a reason, 0xFFFFFFFF if none */
} uvhttp_ws_fail_summary_t;

int uvhttp_ws_gpu_fail_points_streams(uvhttp_ws_gpu_engine_t* eng, const uint8_t* d_wire, uint64_t wire_len,
                                      const uvhttp_ws_frame_desc_t* d_desc, uint32_t max_frames,
                                      const uvhttp_ws_stream_result_t* d_results, uint32_t n_streams,
                                      const uvhttp_ws_utf8_conn_verdict_t* d_verdict, const uint8_t* d_enable,
                                      uint32_t flags, uvhttp_ws_stream_result_t* d_results_out,
                                      uvhttp_ws_utf8_conn_verdict_t* d_verdict_out,
                                      uvhttp_ws_fail_conn_t* d_fail, uvhttp_ws_fail_summary_t* d_summary,
                                      void* stream);
/* Host twin (plain C, host copies of the same tables): all connections of the call at once and
 * the same four outputs, byte for byte; the statement of the rule.  Returns 0, or -1 for an
 * argument the device call answers with EINVAL. */
int uvhttp_ws_fail_points(const uint8_t* wire, uint64_t wire_len, const uvhttp_ws_frame_desc_t* desc,
                          uint32_t max_frames, const uvhttp_ws_stream_result_t* results, uint32_t n_streams,
                          const uvhttp_ws_utf8_conn_verdict_t* verdict, const uint8_t* enable, uint32_t flags,
                          uvhttp_ws_stream_result_t* results_out, uvhttp_ws_utf8_conn_verdict_t* verdict_out,
                          uvhttp_ws_fail_conn_t* fail, uvhttp_ws_fail_summary_t* summary);

/* ---- host-memory pipeline (libuv read buffers in, decoded payloads out) ---------------- */
/* A pipeline owns `depth` slots.  Each slot = a pinned host staging buffer (the caller
 * writes masked frames there, e.g. hands it out from the libuv alloc callback) and a device
 * wire buffer.  Every slot's H2D copy runs on the pipeline's upload stream and its decode and
 * D2H copy on its compute stream (behind an event), so slot k's upload overlaps slot k-1's
 * kernels and download on the two copy queues.  submit() enqueues
 *   H2D(wire[0, wire_len)) -> decode_inplace -> D2H(wire, desc, summary)
 * and returns at once; wait() blocks until the slot's decoded bytes, descriptors and
 * summary are back in pinned host memory (the in-place contract: delivered payloads are
 * unmasked inside the slot buffer).  At most three submissions are in flight: submit() first
 * waits for the submission three back to finish, so depth 4 and up give the caller more slots
 * to fill while three are in flight (with more queued, the copies ran at 22-27 instead of 44
 * GiB/s on MI355X). */
typedef struct uvhttp_ws_gpu_pipeline uvhttp_ws_gpu_pipeline_t;
int uvhttp_ws_gpu_pipeline_create(int device, int depth, uint64_t slot_bytes,
                                  uint32_t slot_frames, uvhttp_ws_gpu_pipeline_t** out);
void uvhttp_ws_gpu_pipeline_free(uvhttp_ws_gpu_pipeline_t* p);
uint8_t* uvhttp_ws_gpu_pipeline_slot_buffer(uvhttp_ws_gpu_pipeline_t* p, int slot);
uint64_t* uvhttp_ws_gpu_pipeline_slot_offsets(uvhttp_ws_gpu_pipeline_t* p, int slot);
/* offsets: when use_offsets != 0 the first n entries of slot_offsets() are used, else
 * frame i starts at i * stride.  Limits as uvhttp_ws_batch_t. */
int uvhttp_ws_gpu_pipeline_submit(uvhttp_ws_gpu_pipeline_t* p, int slot, uint64_t wire_len,
                                  int use_offsets, uint64_t stride, uint32_t n_frames,
                                  int32_t max_frame_size, int32_t max_message_size,
                                  int32_t is_server);
int uvhttp_ws_gpu_pipeline_wait(uvhttp_ws_gpu_pipeline_t* p, int slot,
                                const uvhttp_ws_frame_desc_t** desc,
                                const uvhttp_ws_batch_summary_t** summary);
/* Compact submissions: H2D -> uvhttp_ws_gpu_decode_compact -> D2H of the message arena, the
 * message table and the summary, for uvhttp_ws_deliver_messages (messages reassembled on the
 * device: on_message reads the arena, no fragment copying on the host).  A fixed-stride batch
 * of >= 140-byte frames decodes summary-only (no descriptors) and only its last frame's slot
 * comes back into the slot buffer; any other batch decodes into descriptors, which come back
 * with the decoded wire.  wait_compact returns host pointers valid until the slot's next
 * submission; *desc is NULL for a summary-only batch.  Deliver with
 *   uvhttp_ws_deliver_messages(conn, arena, msgs, summary, slot_buffer(slot), desc, stride).
 * A slot's arena and table are allocated at its first compact submission (slot_bytes + 64 and
 * slot_frames entries). */
int uvhttp_ws_gpu_pipeline_submit_compact(uvhttp_ws_gpu_pipeline_t* p, int slot, uint64_t wire_len,
                                          int use_offsets, uint64_t stride, uint32_t n_frames,
                                          int32_t max_frame_size, int32_t max_message_size,
                                          int32_t is_server);
int uvhttp_ws_gpu_pipeline_wait_compact(uvhttp_ws_gpu_pipeline_t* p, int slot, const uint8_t** arena,
                                        const uvhttp_ws_message_desc_t** msgs,
                                        const uvhttp_ws_frame_desc_t** desc,
                                        const uvhttp_ws_batch_summary_t** summary);

/* Deliver a decoded in-place batch to a connection exactly as uvhttp_ws_process_data would
 * have (src/uvhttp_websocket.c:950-1084): on_message per complete message (fragments
 * reassembled in conn->fragmented_message with the reference growth rules), on_close +
 * state = CLOSED for CLOSE, control-sink echo / pong when conn->user_data != NULL.  `wire`
 * is the host copy of the decoded wire (slot buffer).  Frames [0, summary->n_delivered) are
 * delivered; returns UVHTTP_OK, or UVHTTP_ERROR_INVALID_PARAM if the batch failed (after
 * delivering the frames before the failure, like process_data).  `desc` holds the batch's
 * n_frames entries: when the failing frame, desc[n_delivered], is a first fragment that crossed
 * max_message_size, conn->fragmented_opcode takes its opcode, as the reference sets it before
 * it measures the fragment (src/uvhttp_websocket.c:972-980). */
uvhttp_error_t uvhttp_ws_deliver_batch(struct uvhttp_ws_connection* conn, const uint8_t* wire,
                                       const uvhttp_ws_frame_desc_t* desc,
                                       const uvhttp_ws_batch_summary_t* summary);

/* Deliver a decoded COMPACT batch (uvhttp_ws_gpu_decode_compact, with or without descriptors)
 * to a connection as uvhttp_ws_process_data would have (src/uvhttp_websocket.c:950-1084, the
 * caller's dispatch src/uvhttp_connection.c:1234-1263): on_message(arena + msgs[m].arena_off,
 * msgs[m].len, msgs[m].opcode) per complete message, CLOSE (on_close, echo, state = CLOSED) and
 * PING (pong) through the same hooks as uvhttp_ws_deliver_batch, all in frame order; and a
 * message still open after the last delivered frame (summary->pending_bytes != 0, described by
 * msgs[summary->n_messages], which a compact decode writes then) is left in
 * conn->fragmented_message with the reference's size, capacity and opcode, so the connection's
 * next process_data call continues it.  Like uvhttp_ws_deliver_batch the batch's bytes never
 * passed through recv_buffer, which is not touched; the connection must have no message open
 * (the batch was decoded from a fresh connection's state), else UVHTTP_ERROR_INVALID_PARAM and
 * nothing is delivered.
 *   arena, msgs: host copies of arena[0, summary->arena_bytes) and msgs[0, n_messages + 1).
 *   Control frames keep their (unmasked) payloads in the wire.  With descriptors (desc != NULL,
 *   host copy of the n_delivered + 1 first entries) they are found there and read from `wire`
 *   (host copy of the decoded wire; only control payloads are read).  Summary-only (desc ==
 *   NULL) needs a fixed-stride batch with frame_stride >= 140 — a control frame (<= 131 wire
 *   bytes) then cannot fill a slot, so only the LAST delivered frame can be one; when that
 *   frame belongs to no message, `wire` must hold it at wire + (n_delivered - 1) *
 *   frame_stride (a caller may copy back just those frame_stride bytes into a buffer it
 *   offsets accordingly).  Reserved opcodes 3-7 / 11-15 are delivered without a callback, as
 *   the reference ignores them.  Returns UVHTTP_OK, or UVHTTP_ERROR_INVALID_PARAM if the batch
 *   failed (after delivering the frames before the failure, like process_data; with descriptors
 *   a failing first fragment leaves its opcode in conn->fragmented_opcode as in
 *   uvhttp_ws_deliver_batch) or the arguments cannot describe the batch. */
uvhttp_error_t uvhttp_ws_deliver_messages(struct uvhttp_ws_connection* conn, const uint8_t* arena,
                                          const uvhttp_ws_message_desc_t* msgs,
                                          const uvhttp_ws_batch_summary_t* summary,
                                          const uint8_t* wire, const uvhttp_ws_frame_desc_t* desc,
                                          uint64_t frame_stride);

/* ---- batcher: live libuv reads -> one device decode per flush -------------------------- */
/* The caller side of the reference, on_websocket_read (src/uvhttp_connection.c:1098-1175),
 * calls uvhttp_ws_process_data once per libuv read.  The batcher takes those reads instead
 * (submit_read copies them, as process_data copies into recv_buffer) and decodes everything
 * queued at flush(): per connection, exactly the sequence of process_data calls the reads
 * would have made — same return codes, callbacks, recv-buffer and fragment state (tests/
 * test_c1_echo.py, tests/test_gpu_batcher.py check it against the oracle).  Callbacks fire
 * from flush(), connection by connection in first-read order; within a connection in read
 * order.  A flush whose queued bytes are below min_device_bytes runs the host decoder (one
 * libuv-sized read does not pay for a device round trip); a larger one goes
 * through the device: buffered bytes + reads in a pinned arena -> H2D -> gather ->
 * uvhttp_ws_gpu_decode_reads -> D2H -> uvhttp_ws_deliver_stream per connection.
 *
 * Asynchronous flushes.  The batcher holds two queues.  flush_async() hands the queue being
 * filled to the device and returns at once; submit_read() keeps queueing into the other one
 * (whose arena already streams to HBM while it fills, once it holds min_device_bytes).  The
 * decoded queue is delivered — callbacks fire — by poll() once its results are back in host
 * memory (or by flush()); a queue is staged for the device only after the queue before it
 * was delivered (a connection's later reads see the state its earlier ones left, so every
 * connection still sees exactly the process_data sequence).  With the host decoder (device -1, or a small queue) every
 * flush delivers before it returns.  Integration: flush_async() in the loop's uv_check
 * callback, poll() from a uv_async_t that on_ready signals.
 * Not thread-safe (the loop thread owns it, like the reference); only on_ready runs on
 * another thread. */
typedef struct uvhttp_ws_amd_batcher uvhttp_ws_amd_batcher_t;
/* a connection's queued reads failed: process_data returned rc (the reference then sends
 * close 1002 and closes, :1166-1174); the batcher drops the connection's later reads until
 * uvhttp_ws_amd_batcher_forget */
typedef void (*uvhttp_ws_amd_failure_cb)(void* ctx, struct uvhttp_ws_connection* conn, int rc);
/* an asynchronous flush's results are in host memory (called from a HIP runtime thread:
 * only signal the loop, e.g. uv_async_send; then call poll() on the loop thread) */
typedef void (*uvhttp_ws_amd_ready_cb)(void* ctx);
/* A TLS connection's record stream reached something that is not authenticated application
 * data the device may open: an alert or handshake record (first_status
 * UVHTTP_TLS_REC_CONTROL: close_notify, KeyUpdate, NewSessionTicket ...).  The records before it
 * were decrypted and decoded; `ciphertext` (len bytes, valid during the call) is everything
 * from that record on, including reads queued since, and next_seq is the read sequence number
 * of its first record.  The batcher forgets the connection's TLS state: the caller hands the
 * bytes to mbedtls (mbedtls_ssl_read, as src/uvhttp_connection.c:1128-1144 does) and may
 * register the connection again with uvhttp_ws_amd_batcher_set_tls (e.g. after a KeyUpdate). */
/* first_status of a handback that is not about a record: the device could not open this
 * connection's queued records (a device or launch error, or a queue that did not fit the device
 * layout).  Nothing of them was delivered; `ciphertext` is all of it from next_seq on. */
#define UVHTTP_WS_BATCHER_HANDBACK_DEVICE (-100)
typedef void (*uvhttp_ws_amd_tls_handback_cb)(void* ctx, struct uvhttp_ws_connection* conn,
                                              const uint8_t* ciphertext, size_t len,
                                              uint64_t next_seq, int first_status);
typedef struct {
    int device;                /* HIP device for large flushes; -1 = host decoder only */
    uint64_t min_device_bytes; /* flushes with fewer queued bytes run on the host */
    uint64_t max_bytes;        /* staging capacity (buffered bytes + reads) per flush; with a
                                  device, max_bytes / 6 + max_connections must stay < 2^26 */
    uint32_t max_connections;  /* connections per flush */
    uint32_t max_reads;        /* reads per flush */
    uvhttp_ws_amd_failure_cb on_failure;
    void* ctx;
    uvhttp_ws_amd_ready_cb on_ready; /* optional */
    void* ready_ctx;
    uvhttp_ws_amd_tls_handback_cb on_tls_handback; /* TLS connections (called with ctx) */
} uvhttp_ws_amd_batcher_config_t;
typedef struct {
    uint64_t flushes, device_flushes, host_flushes;
    uint64_t host_reads, device_reads;    /* reads decoded by each path */
    uint64_t device_frames, device_bytes; /* frames / staged bytes decoded on the device */
    uint64_t failures;                    /* connections reported through on_failure */
    uint64_t capacity_flushes;            /* device flushes re-run on the host (frame capacity) */
    double device_ms;                     /* wall time of device flushes (stage -> deliver) */
    uint64_t async_flushes;               /* queues handed to the device */
    uint64_t fallback_flushes;            /* queues that did not fit the device layout: host */
    uint64_t device_errors;               /* device failures; those queues ran on the host */
    uint64_t direct_reads;                /* reads larger than a flush, decoded in submit_read */
    double blocked_ms;                    /* loop-thread time inside batcher calls that flush,
                                             poll or wait: staging, delivering, waiting */
    double max_blocked_ms;                /* the longest single such call */
    double wait_ms;                       /* of blocked_ms: waiting for a device decode */
    double copy_ms;                       /* submit_read: copying reads into the pinned arena */
    double upload_ms;                     /* submit_read: enqueueing early H2D pieces */
    double stage_ms;                      /* staging a queue (prefixes, tables) + enqueueing */
    double deliver_ms;                    /* delivering device results (callbacks included) */
    uint64_t tls_records;                 /* TLS records opened and delivered on the device */
    uint64_t tls_bytes;                   /* their ciphertext bytes */
    uint64_t tls_handbacks;               /* connections handed back (on_tls_handback) */
    uint64_t desc_refetches;              /* flushes whose descriptors outgrew the copy-back
                                             high-water mark (rest fetched on completion) */
    uint64_t blocked_calls;               /* batcher calls counted in blocked_ms */
    double blocked_p50_ms, blocked_p99_ms;  /* their distribution (the last 65 536 calls) */
    double max_blocked_wait_ms;           /* the longest call's split: waiting for the device */
    double max_blocked_stage_ms;          /*   staging + enqueueing */
    double max_blocked_deliver_ms;        /*   delivering (callbacks included) */
    uint64_t zero_copy_reads;             /* reads queued through alloc_read / commit_read */
} uvhttp_ws_amd_batcher_stats_t;
void uvhttp_ws_amd_batcher_config_init(uvhttp_ws_amd_batcher_config_t* cfg);
/* UVHTTP_WS_GPU_ENODEV if cfg->device >= 0 names no usable MI355X (no silent host mode) */
int uvhttp_ws_amd_batcher_create(const uvhttp_ws_amd_batcher_config_t* cfg,
                                 uvhttp_ws_amd_batcher_t** out);
void uvhttp_ws_amd_batcher_free(uvhttp_ws_amd_batcher_t* b);
/* Queue one read of `conn` (the bytes are copied).  When the read would not fit the staging
 * capacity the queue is handed over first (flush_async); a read larger than a whole flush is
 * decoded right here, after the connection's earlier reads were delivered.  Returns
 * UVHTTP_OK, or UVHTTP_ERROR_INVALID_PARAM for a NULL argument, a connection whose earlier
 * reads already failed, or — only from inside a batcher callback, where no flush can start —
 * a read that does not fit the queue. */
uvhttp_error_t uvhttp_ws_amd_batcher_submit_read(uvhttp_ws_amd_batcher_t* b,
                                                 struct uvhttp_ws_connection* conn,
                                                 const uint8_t* data, size_t len);
/* Zero-copy reads: the loop's uv_alloc_cb / uv_read_cb pair (src/uvhttp_connection.c:128-158,
 * 1098-1175).  alloc_read returns space for conn's next read inside the queue's own (pinned)
 * staging arena — *buf, *len bytes, len <= suggested (less when the read would not fit a whole
 * flush); libuv reads the socket straight into it; commit_read then queues the nread bytes
 * exactly as submit_read(conn, buf, nread) would, without copying them.  nread = 0 (EAGAIN, EOF,
 * an error) gives the space back.  One allocation is outstanding at a time: libuv calls the
 * read callback right after the alloc callback for the same stream; any other batcher call in
 * between (a flush may hand the queue over) makes commit_read refuse with
 * UVHTTP_ERROR_INVALID_PARAM, as does a commit for another connection or nread > *len.
 * alloc_read may hand a full queue over first, like submit_read.  TLS connections: the space
 * takes ciphertext (as submit_tls_read). */
uvhttp_error_t uvhttp_ws_amd_batcher_alloc_read(uvhttp_ws_amd_batcher_t* b,
                                                struct uvhttp_ws_connection* conn, size_t suggested,
                                                uint8_t** buf, size_t* len);
uvhttp_error_t uvhttp_ws_amd_batcher_commit_read(uvhttp_ws_amd_batcher_t* b,
                                                 struct uvhttp_ws_connection* conn, size_t nread);
/* Hand everything queued to the decoder and return (see "Asynchronous flushes").  Never waits
 * for the device: when a queue is still in flight the request is remembered and poll() starts
 * this queue right after delivering that one (until then reads keep joining it; a read that
 * no longer fits makes submit_read wait).  0, or the UVHTTP_WS_GPU_* error of a device decode
 * that failed (its queue was decoded by the host decoder instead, so nothing is lost; stats
 * count it).  From inside a batcher callback: does nothing. */
int uvhttp_ws_amd_batcher_flush_async(uvhttp_ws_amd_batcher_t* b);
/* Deliver the queue in flight if its results are back (never waits), then start the queue a
 * flush_async asked for meanwhile: 1 delivered, 0 nothing to deliver yet, or a
 * UVHTTP_WS_GPU_* error as flush_async. */
int uvhttp_ws_amd_batcher_poll(uvhttp_ws_amd_batcher_t* b);
/* 1 while a queue is in flight (the loop must poll or flush before it can idle) */
int uvhttp_ws_amd_batcher_in_flight(const uvhttp_ws_amd_batcher_t* b);
/* Decode everything queued — the queue in flight, then the one being filled — and deliver it
 * before returning (callbacks fire here); returns as flush_async. */
int uvhttp_ws_amd_batcher_flush(uvhttp_ws_amd_batcher_t* b);
/* Drop a connection's queued reads (in both queues), failure mark and TLS state (call before
 * freeing the connection; safe from inside callbacks of a flush). */
void uvhttp_ws_amd_batcher_forget(uvhttp_ws_amd_batcher_t* b, struct uvhttp_ws_connection* conn);

/* TLS connections (the on_websocket_read TLS branch, src/uvhttp_connection.c:1122-1159:
 * mbedtls_ssl_read until WANT_READ, process_data on every decrypted chunk).  set_tls registers
 * the connection's read key (include/uvhttp_tls_amd.h: AES-128/256-GCM or ChaCha20-Poly1305,
 * TLS 1.3 or 1.2, from mbedtls's key export) and the sequence number of its next record;
 * submit_tls_read then queues ciphertext as libuv delivers it.  A flush opens the records of
 * every TLS connection on the device (uvhttp_tls_gpu_open_records), hands each delivered
 * record's content to the WebSocket decoder as one process_data call
 * (uvhttp_tls_gpu_ws_streams -> uvhttp_ws_gpu_decode_reads) and delivers as for plain
 * connections; an incomplete trailing record is kept for the next flush.  A record that is
 * not application data ends the batcher's TLS handling of the connection
 * (on_tls_handback); a record that fails (bad MAC, overflow, bad type or version) reports the
 * connection through on_failure with UVHTTP_ERROR_INVALID_PARAM, as the reference closes it
 * (:1139-1144).  TLS queues always decode on the device (the host decoder has no AEAD):
 * set_tls returns UVHTTP_WS_GPU_ENODEV for a host-only batcher.  A connection is either
 * plain or TLS: submit_read on a TLS connection (and submit_tls_read on a plain one) is
 * UVHTTP_ERROR_INVALID_PARAM.  set_tls flushes the connection's queued plain reads first; from
 * inside a batcher callback, where no flush can run, it returns UVHTTP_WS_GPU_EINVAL while such
 * reads are queued (call it again after the flush). */
int uvhttp_ws_amd_batcher_set_tls(uvhttp_ws_amd_batcher_t* b, struct uvhttp_ws_connection* conn,
                                  const void* tls_key /* uvhttp_tls_key_t */, uint64_t read_seq);
uvhttp_error_t uvhttp_ws_amd_batcher_submit_tls_read(uvhttp_ws_amd_batcher_t* b,
                                                     struct uvhttp_ws_connection* conn,
                                                     const uint8_t* ciphertext, size_t len);
/* Zero the counters (e.g. after a warm-up), so stats() describes what follows. */
void uvhttp_ws_amd_batcher_reset_stats(uvhttp_ws_amd_batcher_t* b);
int uvhttp_ws_amd_batcher_stats(const uvhttp_ws_amd_batcher_t* b,
                                uvhttp_ws_amd_batcher_stats_t* out);
/* NUMA node of the batcher's GPU (its PCI device's sysfs numa_node), or -1 (host-only batcher,
 * or not known).  Run the loop thread that calls submit_read on this node: submit_read copies
 * each read into pinned memory that HIP places next to the GPU, and on the MI355X box that copy
 * ran at 91 GB/s from the GPU's node against 48 GB/s from the other socket — the live shape end
 * to end 38 vs 22 GiB/s (profiles/r03p44_numa_copy_e2e.txt). */
int uvhttp_ws_amd_batcher_numa_node(const uvhttp_ws_amd_batcher_t* b);

/* ---- batcher group: the live path over several GPUs ------------------------------------ */
/* One batcher per device (the same config, cfg->device replaced by devices[k]; a device may be
 * listed twice, -1 = a host-decoder member).  Each connection is pinned to one member on its
 * first call — the member with the fewest live connections — until group_forget, so its reads
 * keep their process_data order (the member guarantees it) while different connections flush
 * over different PCIe links.  flush_async / poll / flush fan out to every member (flush: every
 * member's queue is handed over before any is waited for); poll returns the queues delivered
 * (summed) or the first error.  Callbacks are the members' (cfg's).  Not thread-safe, like the
 * batcher: one loop thread owns the group.  A loop thread copies reads at full rate only into
 * members on its own NUMA node (uvhttp_ws_amd_batcher_numa_node): on a two-socket node run one
 * loop per socket, each with a group of that socket's GPUs. */
typedef struct uvhttp_ws_amd_batcher_group uvhttp_ws_amd_batcher_group_t;
int uvhttp_ws_amd_batcher_group_create(const uvhttp_ws_amd_batcher_config_t* cfg, const int* devices,
                                       int n_devices, uvhttp_ws_amd_batcher_group_t** out);
void uvhttp_ws_amd_batcher_group_free(uvhttp_ws_amd_batcher_group_t* g);
int uvhttp_ws_amd_batcher_group_size(const uvhttp_ws_amd_batcher_group_t* g);
/* member i (its stats, NUMA node), or NULL */
uvhttp_ws_amd_batcher_t* uvhttp_ws_amd_batcher_group_batcher(uvhttp_ws_amd_batcher_group_t* g, int i);
/* the member a connection is pinned to, or -1 if it is not pinned (a query: never pins) */
int uvhttp_ws_amd_batcher_group_member(uvhttp_ws_amd_batcher_group_t* g, struct uvhttp_ws_connection* conn);
uvhttp_error_t uvhttp_ws_amd_batcher_group_submit_read(uvhttp_ws_amd_batcher_group_t* g,
                                                       struct uvhttp_ws_connection* conn,
                                                       const uint8_t* data, size_t len);
/* TLS records open only on device members: a new connection is pinned among them, and one
 * pinned to a host-decoder member moves to a device member when the host member holds nothing
 * of it (reads queued, a failure mark); otherwise, or with no device member, UVHTTP_WS_GPU_ENODEV */
int uvhttp_ws_amd_batcher_group_set_tls(uvhttp_ws_amd_batcher_group_t* g, struct uvhttp_ws_connection* conn,
                                        const void* tls_key, uint64_t read_seq);
/* zero-copy reads through the connection's member (pinned on its first alloc_read) */
uvhttp_error_t uvhttp_ws_amd_batcher_group_alloc_read(uvhttp_ws_amd_batcher_group_t* g,
                                                      struct uvhttp_ws_connection* conn, size_t suggested,
                                                      uint8_t** buf, size_t* len);
uvhttp_error_t uvhttp_ws_amd_batcher_group_commit_read(uvhttp_ws_amd_batcher_group_t* g,
                                                       struct uvhttp_ws_connection* conn, size_t nread);
uvhttp_error_t uvhttp_ws_amd_batcher_group_submit_tls_read(uvhttp_ws_amd_batcher_group_t* g,
                                                           struct uvhttp_ws_connection* conn,
                                                           const uint8_t* ciphertext, size_t len);
int uvhttp_ws_amd_batcher_group_flush_async(uvhttp_ws_amd_batcher_group_t* g);
int uvhttp_ws_amd_batcher_group_poll(uvhttp_ws_amd_batcher_group_t* g);
int uvhttp_ws_amd_batcher_group_flush(uvhttp_ws_amd_batcher_group_t* g);
int uvhttp_ws_amd_batcher_group_in_flight(const uvhttp_ws_amd_batcher_group_t* g);
void uvhttp_ws_amd_batcher_group_forget(uvhttp_ws_amd_batcher_group_t* g, struct uvhttp_ws_connection* conn);
/* counters summed over the members; max_blocked / percentiles: the worst member's */
int uvhttp_ws_amd_batcher_group_stats(const uvhttp_ws_amd_batcher_group_t* g,
                                      uvhttp_ws_amd_batcher_stats_t* out);
void uvhttp_ws_amd_batcher_group_reset_stats(uvhttp_ws_amd_batcher_group_t* g);

/* Library identity, for the loader checks in tests/. */
const char* uvhttp_ws_amd_version(void);

#ifdef __cplusplus
}
#endif

#endif /* UVHTTP_WS_AMD_H */
