/*
 * oracle/ref_driver.c — TEST INFRASTRUCTURE ONLY.
 *
 * Drives the reference's own WebSocket unit (src/uvhttp_websocket.c of the reference tree,
 * compiled as it stands by ref.mk) so that tests can run it: oracle/_ref/libws_ref.so is that
 * object plus this file.  Everything here is ours:
 *   - definitions of the symbols the unit leaves undefined (other units of the reference and
 *     five mbedtls functions): do-nothing stubs, a capturing mbedtls_ssl_write and a
 *     deterministic mbedtls_ctr_drbg_random;
 *   - a zeroed wrapper -> connection -> server -> context chain that can hang on user_data;
 *   - callbacks that write a transcript;
 *   - a flat C API for ctypes (ws_ref_*).
 *
 * Transcript record, the layout oracle/ws_oracle.c uses:  u8 type | i32 a | u64 len | bytes.
 *   1 message  a = opcode, bytes = the message
 *   2 close    a = code, no bytes (the reference hands on_close a pointer into the receive
 *              buffer with no terminator, so the reason cannot be read safely)
 *   3 error    a = error code, no bytes
 *   4 sent     bytes = what one mbedtls_ssl_write call was handed (one whole frame: the fake
 *              accepts everything at once)
 *
 * Masking keys: byte j of the connection's key stream is byte (j & 3), low first, of
 * ws_ref_key_word(seed, j >> 2); mbedtls_ctr_drbg_random hands out the stream in order, so a
 * client's i-th frame is masked with word i.  ws_ref_key_word is exported for the tests.
 */
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "uvhttp_context.h"
#include "uvhttp_protocol_upgrade.h"
#include "uvhttp_server.h"
#include "uvhttp_utils.h"
#include "uvhttp_websocket.h"

enum { REF_EV_MESSAGE = 1, REF_EV_CLOSE = 2, REF_EV_ERROR = 3, REF_EV_SENT = 4 };

typedef struct ws_ref_conn {
    mbedtls_ssl_context ssl;       /* first: mbedtls_ssl_write finds the connection by it */
    mbedtls_ctr_drbg_context drbg; /* found by offset in mbedtls_ctr_drbg_random */
    uvhttp_ws_connection_t* ws;
    uvhttp_ws_wrapper_t wrapper;
    uvhttp_connection_t http;
    uvhttp_server_t server;
    uvhttp_context_t context;
    int echo;
    uint64_t seed, key_bytes; /* key stream: seed and bytes handed out so far */
    uint8_t* ev;
    size_t ev_len, ev_cap;
} ws_ref_conn_t;

/* ---- transcript ---------------------------------------------------------------------------- */

static void ev_push(ws_ref_conn_t* c, uint8_t type, int32_t a, const void* p, uint64_t len) {
    const size_t need = 1 + 4 + 8 + (size_t)len;
    if (c->ev_len + need > c->ev_cap) {
        size_t nc = c->ev_cap ? c->ev_cap : 4096;
        while (nc < c->ev_len + need) nc *= 2;
        uint8_t* nb = (uint8_t*)realloc(c->ev, nc);
        if (!nb) abort();
        c->ev = nb;
        c->ev_cap = nc;
    }
    uint8_t* w = c->ev + c->ev_len;
    w[0] = type;
    memcpy(w + 1, &a, 4);
    memcpy(w + 5, &len, 8);
    if (len) memcpy(w + 13, p, (size_t)len);
    c->ev_len += need;
}

/* ---- key stream ---------------------------------------------------------------------------- */

uint32_t ws_ref_key_word(uint64_t seed, uint64_t i) {
    uint64_t z = seed + (i + 1) * 0x9E3779B97F4A7C15ull; /* splitmix64 */
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return (uint32_t)(z >> 16);
}

/* ---- what the unit leaves undefined ------------------------------------------------------- */

int mbedtls_ssl_write(mbedtls_ssl_context* ssl, const unsigned char* buf, size_t len) {
    ws_ref_conn_t* c = (ws_ref_conn_t*)(void*)ssl;
    ev_push(c, REF_EV_SENT, 0, buf, len);
    return (int)len;
}

int mbedtls_ssl_read(mbedtls_ssl_context* ssl, unsigned char* buf, size_t len) {
    (void)ssl;
    (void)buf;
    (void)len;
    return -1; /* uvhttp_ws_recv_frame is not driven */
}

int mbedtls_ctr_drbg_random(void* p_rng, unsigned char* out, size_t len) {
    ws_ref_conn_t* c = (ws_ref_conn_t*)(void*)((char*)p_rng - offsetof(ws_ref_conn_t, drbg));
    for (size_t k = 0; k < len; ++k, ++c->key_bytes)
        out[k] = (unsigned char)(ws_ref_key_word(c->seed, c->key_bytes >> 2) >>
                                 (8 * (c->key_bytes & 3)));
    return 0;
}

int mbedtls_sha1(const unsigned char* in, size_t len, unsigned char out[20]) {
    (void)in;
    (void)len;
    memset(out, 0, 20); /* the handshake is not driven */
    return 0;
}

int mbedtls_base64_encode(unsigned char* dst, size_t dlen, size_t* olen, const unsigned char* src,
                          size_t slen) {
    (void)src;
    (void)slen;
    if (dlen) dst[0] = 0;
    *olen = 0;
    return 0;
}

void uvhttp_connection_close(uvhttp_connection_t* conn) { (void)conn; }

uvhttp_error_t uvhttp_connection_handle_websocket_handshake(uvhttp_connection_t* conn,
                                                            const char* key) {
    (void)conn;
    (void)key;
    return UVHTTP_ERROR_INVALID_PARAM;
}

const char* uvhttp_request_get_header(uvhttp_request_t* req, const char* name) {
    (void)req;
    (void)name;
    return NULL;
}

uvhttp_error_t uvhttp_response_set_status(uvhttp_response_t* r, int code) {
    (void)r;
    (void)code;
    return UVHTTP_OK;
}

uvhttp_error_t uvhttp_response_set_header(uvhttp_response_t* r, const char* n, const char* v) {
    (void)r;
    (void)n;
    (void)v;
    return UVHTTP_OK;
}

uvhttp_error_t uvhttp_response_set_body(uvhttp_response_t* r, const char* b, size_t n) {
    (void)r;
    (void)b;
    (void)n;
    return UVHTTP_OK;
}

uvhttp_error_t uvhttp_response_send(uvhttp_response_t* r) {
    (void)r;
    return UVHTTP_OK;
}

int uvhttp_safe_strncpy(char* dst, const char* src, size_t cap) {
    if (!dst || !src || cap == 0) return -1;
    size_t n = strlen(src);
    if (n >= cap) n = cap - 1;
    memcpy(dst, src, n);
    dst[n] = 0;
    return 0;
}

uvhttp_error_t uvhttp_server_register_protocol_upgrade(uvhttp_server_t* s, const char* name,
                                                       const char* upgrade,
                                                       uvhttp_protocol_detector_t det,
                                                       uvhttp_protocol_upgrade_handler_t h,
                                                       void* user) {
    (void)s;
    (void)name;
    (void)upgrade;
    (void)det;
    (void)h;
    (void)user;
    return UVHTTP_OK;
}

/* ---- callbacks ----------------------------------------------------------------------------- */

static ws_ref_conn_t* owner_of(uvhttp_ws_connection_t* ws) {
    return (ws_ref_conn_t*)(void*)ws->ssl;
}

static int cb_message(uvhttp_ws_connection_t* ws, const char* data, size_t len, int opcode) {
    ws_ref_conn_t* c = owner_of(ws);
    ev_push(c, REF_EV_MESSAGE, opcode, data, len);
    /* the echo hook: what the reference's echo server does with a message, with the message's
     * own opcode; the application holds its context whether or not user_data leads to one */
    if (c->echo)
        uvhttp_ws_send_frame(&c->context, ws, (const uint8_t*)data, len,
                             (uvhttp_ws_opcode_t)opcode);
    return 0;
}

static int cb_close(uvhttp_ws_connection_t* ws, int code, const char* reason) {
    (void)reason;
    ev_push(owner_of(ws), REF_EV_CLOSE, code, NULL, 0);
    return 0;
}

static int cb_error(uvhttp_ws_connection_t* ws, int code, const char* msg) {
    (void)msg;
    ev_push(owner_of(ws), REF_EV_ERROR, code, NULL, 0);
    return 0;
}

/* ---- flat API ------------------------------------------------------------------------------ */

/* max_frame_size and max_message_size both < 0: a NULL config (the reference's own defaults);
 * otherwise a config with the two values, a negative one replaced by the reference's default.
 * The connection is OPEN as after a handshake. */
ws_ref_conn_t* ws_ref_conn_new(int is_server, int max_frame_size, int max_message_size,
                               int wire_context, int echo, uint64_t key_seed) {
    ws_ref_conn_t* c = (ws_ref_conn_t*)calloc(1, sizeof(*c));
    if (!c) return NULL;
    uvhttp_config_t cfg;
    memset(&cfg, 0, sizeof(cfg));
    cfg.websocket_max_frame_size =
        max_frame_size < 0 ? UVHTTP_WEBSOCKET_DEFAULT_MAX_FRAME_SIZE : max_frame_size;
    cfg.websocket_max_message_size =
        max_message_size < 0 ? UVHTTP_WEBSOCKET_DEFAULT_MAX_MESSAGE_SIZE : max_message_size;
    cfg.websocket_ping_interval = UVHTTP_WEBSOCKET_DEFAULT_PING_INTERVAL;
    cfg.websocket_ping_timeout = UVHTTP_WEBSOCKET_DEFAULT_PING_TIMEOUT;
    const int defaults = max_frame_size < 0 && max_message_size < 0;
    c->ws = uvhttp_ws_connection_create(-1, &c->ssl, is_server, defaults ? NULL : &cfg);
    if (!c->ws) {
        free(c);
        return NULL;
    }
    c->ws->state = UVHTTP_WS_STATE_OPEN;
    c->echo = echo;
    c->seed = key_seed;
    c->context.ws_drbg = &c->drbg;
    c->context.ws_drbg_initialized = 1;
    c->server.context = &c->context;
    c->http.server = &c->server;
    c->wrapper.conn = &c->http;
    if (wire_context) c->ws->user_data = &c->wrapper;
    uvhttp_ws_set_callbacks(c->ws, cb_message, cb_close, cb_error);
    return c;
}

void ws_ref_conn_free(ws_ref_conn_t* c) {
    if (!c) return;
    uvhttp_ws_connection_free(c->ws);
    free(c->ev);
    free(c);
}

int ws_ref_feed(ws_ref_conn_t* c, const uint8_t* data, size_t len) {
    return (int)uvhttp_ws_process_data(c->ws, data, len);
}

size_t ws_ref_events(const ws_ref_conn_t* c, uint8_t* out, size_t cap) {
    if (out && cap >= c->ev_len && c->ev_len) memcpy(out, c->ev, c->ev_len);
    return c->ev_len;
}

/* state, recv_buffer_pos, recv_buffer_size, fragmented_size, fragmented_opcode,
 * fragmented_message == NULL, frames_sent, key bytes handed out */
void ws_ref_end_state(const ws_ref_conn_t* c, uint64_t out[8]) {
    const uvhttp_ws_connection_t* w = c->ws;
    out[0] = (uint64_t)w->state;
    out[1] = w->recv_buffer_pos;
    out[2] = w->recv_buffer_size;
    out[3] = w->fragmented_size;
    out[4] = (uint64_t)w->fragmented_opcode;
    out[5] = w->fragmented_message == NULL;
    out[6] = w->frames_sent;
    out[7] = c->key_bytes;
}

/* fields: fin, rsv1, rsv2, rsv3, opcode, mask, payload_len (the length code), payload_length */
int ws_ref_parse_frame_header(const uint8_t* data, size_t len, uint64_t fields[8],
                              size_t* header_size) {
    uvhttp_ws_frame_header_t h;
    memset(&h, 0, sizeof(h)); /* a call that returns before it writes the header reads as zeros */
    const int rc = (int)uvhttp_ws_parse_frame_header(data, len, &h, header_size);
    fields[0] = h.fin;
    fields[1] = h.rsv1;
    fields[2] = h.rsv2;
    fields[3] = h.rsv3;
    fields[4] = h.opcode;
    fields[5] = h.mask;
    fields[6] = h.payload_len;
    fields[7] = h.payload_length;
    return rc;
}

/* n calls in one: call i parses bufs[i * stride, + lens[i]) into rc[i], fields[8 * i ..] and
 * header_size[i] (both zero before the call) */
void ws_ref_parse_many(const uint8_t* bufs, size_t stride, const uint32_t* lens, size_t n,
                       int32_t* rc, uint64_t* fields, uint64_t* header_size) {
    for (size_t i = 0; i < n; ++i) {
        size_t hs = 0;
        rc[i] = ws_ref_parse_frame_header(bufs + i * stride, lens[i], fields + 8 * i, &hs);
        header_size[i] = hs;
    }
}

void ws_ref_apply_mask(uint8_t* data, size_t len, const uint8_t* key) {
    uvhttp_ws_apply_mask(data, len, key);
}

/* keys come from c's key stream */
long ws_ref_build_frame(ws_ref_conn_t* c, uint8_t* buffer, size_t buffer_size,
                        const uint8_t* payload, size_t payload_len, int opcode, int mask,
                        int fin) {
    return uvhttp_ws_build_frame(&c->context, buffer, buffer_size, payload, payload_len,
                                 (uvhttp_ws_opcode_t)opcode, mask, fin);
}
