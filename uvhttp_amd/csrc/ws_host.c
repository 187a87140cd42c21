/*
 * ws_host.c — drop-in host side of the decode surface (include/uvhttp_ws_amd.h §1b).
 *
 * These are the functions src/uvhttp_connection.c links against
 * (on_websocket_read -> uvhttp_ws_process_data, src/uvhttp_connection.c:1154-1164).  A live
 * libuv read is <= 16 KiB (include/uvhttp_constants.h:207-208), far below what pays for a
 * device round trip, so the per-connection stream path runs here on the host; batches of
 * frames resident in HBM go through the gfx950 kernels in ws_gpu.hip instead.
 *
 * Structure: process_data = append (grow_recv) -> repeat { scan_frame -> unmask ->
 * dispatch_frame -> drain } until the buffered bytes hold no complete frame.  The observable
 * behaviour — return codes, callback order and arguments, recv/fragment buffer sizes, state —
 * matches src/uvhttp_websocket.c:825-1097; tests/test_host_dropin.py replays the reference's
 * own known-answer tests and a randomized stream against the oracle to check it.
 */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "utf8_rules.h"
#include "uvhttp_ws_amd.h"

static uvhttp_ws_amd_context_resolver g_resolver = NULL;
static uvhttp_ws_amd_control_sink g_control_sink = NULL;

void uvhttp_ws_amd_set_control_hooks(uvhttp_ws_amd_context_resolver resolver,
                                     uvhttp_ws_amd_control_sink sink) {
    g_resolver = resolver;
    g_control_sink = sink;
}

/* the server context the reference reaches through conn->user_data, or NULL */
static void* server_context(uvhttp_ws_connection_t* c) {
    return (c->user_data != NULL && g_resolver != NULL) ? g_resolver(c) : NULL;
}

/* ---- connection lifetime (src/uvhttp_websocket.c:71-130, 1100-1111) ------------------- */

struct uvhttp_ws_connection* uvhttp_ws_connection_create(int fd, mbedtls_ssl_context* ssl,
                                                         int is_server,
                                                         const uvhttp_config_t* config) {
    uvhttp_ws_connection_t* c = (uvhttp_ws_connection_t*)calloc(1, sizeof(*c));
    if (c == NULL) return NULL;
    c->fd = fd;
    c->ssl = ssl;
    c->is_server = is_server;
    c->state = UVHTTP_WS_STATE_CONNECTING;
    c->config.max_frame_size =
        config ? config->websocket_max_frame_size : UVHTTP_WS_AMD_DEFAULT_MAX_FRAME_SIZE;
    c->config.max_message_size =
        config ? config->websocket_max_message_size : UVHTTP_WS_AMD_DEFAULT_MAX_MESSAGE_SIZE;
    c->config.ping_interval =
        config ? config->websocket_ping_interval : UVHTTP_WS_AMD_DEFAULT_PING_INTERVAL;
    c->config.ping_timeout =
        config ? config->websocket_ping_timeout : UVHTTP_WS_AMD_DEFAULT_PING_TIMEOUT;
    c->recv_buffer_size = UVHTTP_WS_AMD_DEFAULT_RECV_BUFFER_SIZE;
    c->recv_buffer = (uint8_t*)malloc(c->recv_buffer_size);
    if (c->recv_buffer == NULL) {
        free(c);
        return NULL;
    }
    return c;
}

void uvhttp_ws_connection_free(struct uvhttp_ws_connection* c) {
    if (c == NULL) return;
    free(c->recv_buffer);
    free(c->send_buffer);
    free(c->fragmented_message);
    free(c);
}

void uvhttp_ws_set_callbacks(struct uvhttp_ws_connection* c,
                             uvhttp_ws_on_message_callback on_message,
                             uvhttp_ws_on_close_callback on_close,
                             uvhttp_ws_on_error_callback on_error) {
    if (c == NULL) return;
    c->on_message = on_message;
    c->on_close = on_close;
    c->on_error = on_error;
}

/* ---- header + mask --------------------------------------------------------------------- */

/* Length code -> bytes of header before the mask key (RFC 6455 §5.2). */
static size_t header_span(uint8_t second_byte) {
    uint8_t code = second_byte & 0x7F;
    return code == 126 ? 4 : code == 127 ? 10 : 2;
}

uvhttp_error_t uvhttp_ws_parse_frame_header(const uint8_t* data, size_t len,
                                            uvhttp_ws_frame_header_t* header,
                                            size_t* header_size) {
    if (data == NULL || header == NULL || header_size == NULL || len < 2)
        return UVHTTP_ERROR_INVALID_PARAM;
    memset(header, 0, sizeof(*header));
    const uint8_t b0 = data[0], b1 = data[1];
    header->fin = b0 >> 7;
    header->rsv1 = (b0 >> 6) & 1;
    header->rsv2 = (b0 >> 5) & 1;
    header->rsv3 = (b0 >> 4) & 1;
    header->opcode = b0 & 0x0F;
    header->mask = b1 >> 7;
    header->payload_len = b1 & 0x7F;
    const size_t span = header_span(b1);
    uint64_t length = b1 & 0x7F;
    header->payload_length = length;
    *header_size = 2;
    if (span > 2) {
        if (len < span) return UVHTTP_ERROR_INVALID_PARAM;
        length = 0;
        for (size_t k = 2; k < span; ++k) length = (length << 8) | data[k];
        header->payload_length = length;
        if (span == 10 && (length >> 63)) return UVHTTP_ERROR_INVALID_PARAM;
        *header_size = span;
    }
    header->payload_length = length;
    return UVHTTP_OK;
}

/* Word-at-a-time XOR: the key rotated to the first aligned byte is replicated into a
 * 64-bit word; head and tail bytes use the plain byte rule. */
void uvhttp_ws_apply_mask(uint8_t* data, size_t len, const uint8_t* key) {
    if (data == NULL || key == NULL) return;
    size_t i = 0;
    while (i < len && ((uintptr_t)(data + i) & 7u)) {
        data[i] ^= key[i & 3];
        ++i;
    }
    if (len - i >= 8) {
        uint8_t rot[8];
        for (int b = 0; b < 8; ++b) rot[b] = key[(i + (size_t)b) & 3];
        uint64_t k64;
        memcpy(&k64, rot, 8);
        uint64_t* w = (uint64_t*)(void*)(data + i);
        size_t nw = (len - i) / 8;
        for (size_t j = 0; j < nw; ++j) w[j] ^= k64;
        i += nw * 8;
    }
    for (; i < len; ++i) data[i] ^= key[i & 3];
}

/* ---- stream decode ----------------------------------------------------------------------- */

enum scan_outcome { SCAN_FRAME, SCAN_NEED_MORE, SCAN_REJECT };

typedef struct {
    uvhttp_ws_frame_header_t hdr;
    size_t head;  /* header bytes before the key */
    size_t total; /* header + key + payload */
} frame_view_t;

/* Recv-buffer growth (src/uvhttp_websocket.c:832-866): double until the new bytes fit,
 * never beyond config.max_frame_size. */
static int grow_recv(uvhttp_ws_connection_t* c, size_t extra) {
    const size_t want = c->recv_buffer_pos + extra;
    if (want <= c->recv_buffer_size) return 0;
    size_t cap = c->recv_buffer_size;
    do {
        if (cap > SIZE_MAX / 2) return -1;
        cap *= 2;
    } while (want > cap);
    const size_t ceiling = (size_t)c->config.max_frame_size;
    if (cap > ceiling) {
        cap = ceiling;
        if (want > cap) return -1;
    }
    uint8_t* nb = (uint8_t*)realloc(c->recv_buffer, cap);
    if (nb == NULL) return -1;
    c->recv_buffer = nb;
    c->recv_buffer_size = cap;
    return 0;
}

/* Decide what the head of the receive buffer holds (src/uvhttp_websocket.c:876-932). */
static enum scan_outcome scan_frame(const uvhttp_ws_connection_t* c, frame_view_t* v) {
    const uint8_t* buf = c->recv_buffer;
    const size_t have = c->recv_buffer_pos;
    if (uvhttp_ws_parse_frame_header(buf, have, &v->hdr, &v->head) != UVHTTP_OK)
        return have < header_span(buf[1]) ? SCAN_NEED_MORE : SCAN_REJECT;
    const uvhttp_ws_frame_header_t* h = &v->hdr;
    if (h->rsv1 | h->rsv2 | h->rsv3) return SCAN_REJECT;
    if (h->opcode >= UVHTTP_WS_OPCODE_CLOSE && (h->payload_length > 125 || !h->fin))
        return SCAN_REJECT;
    if (c->is_server && !h->mask) return SCAN_REJECT;
    if (h->payload_length > (uint64_t)c->config.max_frame_size) return SCAN_REJECT;
    v->total = v->head + (h->mask ? 4u : 0u) + (size_t)h->payload_length;
    return have < v->total ? SCAN_NEED_MORE : SCAN_FRAME;
}

/* uvhttp_ws_fragment_append semantics (src/uvhttp_websocket.c:781-822). */
static int append_fragment(uvhttp_ws_connection_t* c, const uint8_t* p, size_t n) {
    const size_t limit = (size_t)c->config.max_message_size;
    if (limit != 0 && (c->fragmented_size > limit || n > limit - c->fragmented_size)) return -1;
    if (n > c->fragmented_capacity - c->fragmented_size) {
        const size_t need = c->fragmented_size + n;
        size_t cap = c->fragmented_capacity;
        if (cap == 0) {
            cap = need;
        } else {
            while (cap < need) {
                if (cap > SIZE_MAX / 2) return -1;
                cap *= 2;
            }
        }
        uint8_t* nb = (uint8_t*)realloc(c->fragmented_message, cap);
        if (nb == NULL) return -1;
        c->fragmented_message = nb;
        c->fragmented_capacity = cap;
    }
    if (n) memcpy(c->fragmented_message + c->fragmented_size, p, n);
    c->fragmented_size += n;
    return 0;
}

static void drop_fragment(uvhttp_ws_connection_t* c) {
    free(c->fragmented_message);
    c->fragmented_message = NULL;
    c->fragmented_size = 0;
    c->fragmented_capacity = 0;
}

/* Data frames: RFC 6455 §5.4 reassembly (src/uvhttp_websocket.c:950-1015). */
static int on_data_frame(uvhttp_ws_connection_t* c, const uvhttp_ws_frame_header_t* h,
                         const uint8_t* payload) {
    const size_t n = (size_t)h->payload_length;
    const int is_cont = h->opcode == UVHTTP_WS_OPCODE_CONTINUATION;
    if (c->fragmented_message != NULL) { /* a message is open */
        if (!is_cont) return -1;
        if (append_fragment(c, payload, n) != 0) return -1;
        if (h->fin) {
            if (c->on_message)
                c->on_message(c, (const char*)c->fragmented_message, c->fragmented_size,
                              c->fragmented_opcode);
            drop_fragment(c);
        }
        return 0;
    }
    if (is_cont) return -1;
    if (h->fin) {
        if (c->on_message) c->on_message(c, (const char*)payload, n, h->opcode);
        return 0;
    }
    c->fragmented_opcode = (uvhttp_ws_opcode_t)h->opcode;
    c->fragmented_size = 0;
    c->fragmented_capacity = 0;
    c->fragmented_message = NULL;
    return append_fragment(c, payload, n);
}

/* CLOSE (src/uvhttp_websocket.c:1016-1069). */
static void on_close_frame(uvhttp_ws_connection_t* c, const uint8_t* payload, size_t n) {
    int code = 1000;
    const char* reason = "";
    if (n >= 2) {
        code = (payload[0] << 8) | payload[1];
        if (n > 2) reason = (const char*)(payload + 2);
    }
    void* ctx = server_context(c); /* captured before on_close frees the wrapper */
    if (c->on_close) c->on_close(c, code, reason);
    if (ctx != NULL && g_control_sink != NULL) {
        uint8_t echo[2 + 125];
        size_t elen = 0;
        if (n >= 2) {
            size_t r = n - 2 > 125 ? 125 : n - 2;
            memcpy(echo, payload, 2 + r);
            elen = 2 + r;
        }
        g_control_sink(ctx, c, UVHTTP_WS_OPCODE_CLOSE, echo, elen);
    }
    c->state = UVHTTP_WS_STATE_CLOSED;
}

static int dispatch_frame(uvhttp_ws_connection_t* c, const uvhttp_ws_frame_header_t* h,
                          const uint8_t* payload) {
    switch (h->opcode) {
        case UVHTTP_WS_OPCODE_CONTINUATION:
        case UVHTTP_WS_OPCODE_TEXT:
        case UVHTTP_WS_OPCODE_BINARY:
            return on_data_frame(c, h, payload);
        case UVHTTP_WS_OPCODE_CLOSE:
            on_close_frame(c, payload, (size_t)h->payload_length);
            return 0;
        case UVHTTP_WS_OPCODE_PING: { /* src/uvhttp_websocket.c:1070-1084 */
            void* ctx = server_context(c);
            if (ctx != NULL && g_control_sink != NULL)
                g_control_sink(ctx, c, UVHTTP_WS_OPCODE_PONG, payload, (size_t)h->payload_length);
            return 0;
        }
        default: /* PONG and reserved opcodes are ignored (:1085) */
            return 0;
    }
}

uvhttp_error_t uvhttp_ws_process_data(struct uvhttp_ws_connection* c, const uint8_t* data,
                                      size_t len) {
    if (c == NULL || data == NULL) return UVHTTP_ERROR_INVALID_PARAM;
    if (grow_recv(c, len) != 0) return UVHTTP_ERROR_INVALID_PARAM;
    if (len) memcpy(c->recv_buffer + c->recv_buffer_pos, data, len);
    c->recv_buffer_pos += len;

    while (c->recv_buffer_pos >= 2) {
        frame_view_t v;
        const enum scan_outcome s = scan_frame(c, &v);
        if (s == SCAN_NEED_MORE) break;
        if (s == SCAN_REJECT) return UVHTTP_ERROR_INVALID_PARAM;

        uint8_t* payload = NULL;
        if (v.hdr.payload_length > 0) {
            payload = c->recv_buffer + v.head;
            if (v.hdr.mask) {
                uint8_t key[4];
                memcpy(key, payload, 4);
                payload += 4;
                uvhttp_ws_apply_mask(payload, (size_t)v.hdr.payload_length, key);
            }
        }
        if (dispatch_frame(c, &v.hdr, payload) != 0) return UVHTTP_ERROR_INVALID_PARAM;

        const size_t rest = c->recv_buffer_pos - v.total;
        if (rest) memmove(c->recv_buffer, c->recv_buffer + v.total, rest);
        c->recv_buffer_pos = rest;
    }
    return UVHTTP_OK;
}

/* ---- delivery of a device-decoded batch (include/uvhttp_ws_amd.h) ----------------------- */

/* What the frame that failed a batch left behind in the reference: a first fragment (TEXT /
 * BINARY, FIN clear, no message open) records its opcode and zeroes the fragment sizes BEFORE
 * uvhttp_ws_fragment_append measures it against max_message_size (src/uvhttp_websocket.c:972-980),
 * so a start that fails that check still changes fragmented_opcode.  Every other failure returns
 * before it writes anything. */
static void failed_start_keeps_its_opcode(uvhttp_ws_connection_t* c,
                                          const uvhttp_ws_batch_summary_t* summary,
                                          const uvhttp_ws_frame_desc_t* failing) {
    if (summary->first_status != UVHTTP_WS_FRAME_ERR_MESSAGE || failing == NULL ||
        c->fragmented_message != NULL)
        return;
    const int opcode = failing->opcode & 0x0F;
    if ((opcode != UVHTTP_WS_OPCODE_TEXT && opcode != UVHTTP_WS_OPCODE_BINARY) ||
        (failing->flags & UVHTTP_WS_FLAG_FIN))
        return;
    c->fragmented_opcode = (uvhttp_ws_opcode_t)opcode;
    c->fragmented_size = 0;
    c->fragmented_capacity = 0;
}

uvhttp_error_t uvhttp_ws_deliver_batch(struct uvhttp_ws_connection* c, const uint8_t* wire,
                                       const uvhttp_ws_frame_desc_t* desc,
                                       const uvhttp_ws_batch_summary_t* summary) {
    if (c == NULL || summary == NULL || (summary->n_delivered && (wire == NULL || desc == NULL)))
        return UVHTTP_ERROR_INVALID_PARAM;
    for (uint32_t i = 0; i < summary->n_delivered; ++i) {
        const uvhttp_ws_frame_desc_t* d = &desc[i];
        uvhttp_ws_frame_header_t h;
        memset(&h, 0, sizeof(h));
        h.fin = (d->flags & UVHTTP_WS_FLAG_FIN) ? 1 : 0;
        h.mask = (d->flags & UVHTTP_WS_FLAG_MASK) ? 1 : 0;
        h.opcode = d->opcode & 0x0F;
        h.payload_length = d->payload_len;
        const uint8_t* payload = d->payload_len ? wire + d->payload_off : NULL;
        if (dispatch_frame(c, &h, payload) != 0) return UVHTTP_ERROR_INVALID_PARAM;
    }
    if (summary->status != 0 && desc != NULL && summary->n_delivered < summary->n_frames)
        failed_start_keeps_its_opcode(c, summary, &desc[summary->n_delivered]);
    return summary->status == 0 ? UVHTTP_OK : UVHTTP_ERROR_INVALID_PARAM;
}

/* A control frame of a compact decode (payload unmasked in place in the wire) through the
 * same dispatch as process_data; data frames of reserved opcodes fall through to its default. */
static void dispatch_control(uvhttp_ws_connection_t* c, int opcode, const uint8_t* payload,
                             uint64_t len) {
    uvhttp_ws_frame_header_t h;
    memset(&h, 0, sizeof(h));
    h.fin = 1;
    h.opcode = (uint8_t)(opcode & 0x0F);
    h.payload_length = len;
    (void)dispatch_frame(c, &h, len ? payload : NULL);
}

/* The delivered frames of a compact decode are its messages (each fires at its last frame) and
 * its non-data frames, merged in frame order (include/uvhttp_ws_amd.h). */
uvhttp_error_t uvhttp_ws_deliver_messages(struct uvhttp_ws_connection* c, const uint8_t* arena,
                                          const uvhttp_ws_message_desc_t* msgs,
                                          const uvhttp_ws_batch_summary_t* summary,
                                          const uint8_t* wire, const uvhttp_ws_frame_desc_t* desc,
                                          uint64_t frame_stride) {
    if (c == NULL || summary == NULL || c->fragmented_message != NULL)
        return UVHTTP_ERROR_INVALID_PARAM;
    const uint32_t nd = summary->n_delivered, nm = summary->n_messages;
    const int open = summary->pending_bytes != 0;
    if (nd > summary->n_frames || nm > nd || ((nm || open) && (msgs == NULL || arena == NULL)))
        return UVHTTP_ERROR_INVALID_PARAM;
    /* every message inside the arena, in frame order, ending at a delivered frame */
    for (uint32_t m = 0; m < nm + (uint32_t)open; ++m) {
        const uvhttp_ws_message_desc_t* d = &msgs[m];
        if (d->arena_off > summary->arena_bytes || d->len > summary->arena_bytes - d->arena_off ||
            d->first_frame > d->last_frame || d->last_frame >= nd ||
            (m && d->first_frame <= msgs[m - 1].last_frame))
            return UVHTTP_ERROR_INVALID_PARAM;
    }
    if (open && (msgs[nm].len != summary->pending_bytes || msgs[nm].reserved == 0))
        return UVHTTP_ERROR_INVALID_PARAM;
    /* summary-only: only the last delivered frame can be a non-data frame (frames of a
     * >= 140-byte stride are too long to be control frames); find out whether it is one */
    const uint8_t* last_ctl = NULL;
    int last_start = 0; /* the last frame is an empty first fragment: its opcode */
    uvhttp_ws_frame_header_t lh;
    size_t lhead = 0;
    if (desc == NULL && nd > 0) {
        if (frame_stride < 140) return UVHTTP_ERROR_INVALID_PARAM;
        const uint32_t last = nd - 1;
        const int covered = (nm && msgs[nm - 1].last_frame == last) || (open && msgs[nm].last_frame == last);
        if (!covered) {
            if (wire == NULL) return UVHTTP_ERROR_INVALID_PARAM;
            last_ctl = wire + (size_t)last * frame_stride;
            if (uvhttp_ws_parse_frame_header(last_ctl, (size_t)frame_stride, &lh, &lhead) != UVHTTP_OK)
                return UVHTTP_ERROR_INVALID_PARAM;
            if (lh.opcode < UVHTTP_WS_OPCODE_CLOSE) { /* a data frame that completes nothing: a
                                                         zero-length start (or empty middle fragment) */
                last_ctl = NULL;
                if ((lh.opcode == UVHTTP_WS_OPCODE_TEXT || lh.opcode == UVHTTP_WS_OPCODE_BINARY) && !lh.fin)
                    last_start = lh.opcode;
            }
        }
    }
    if (desc != NULL && nd > 0 && wire == NULL) {
        for (uint32_t i = 0; i < nd; ++i)
            if (desc[i].opcode >= UVHTTP_WS_OPCODE_CLOSE && desc[i].payload_len)
                return UVHTTP_ERROR_INVALID_PARAM;
    }

    uint32_t m = 0;
    if (desc != NULL) {
        for (uint32_t i = 0; i < nd; ++i) {
            const uvhttp_ws_frame_desc_t* d = &desc[i];
            if (d->opcode < UVHTTP_WS_OPCODE_CLOSE) continue; /* data frames: their messages */
            for (; m < nm && msgs[m].last_frame < i; ++m)
                if (c->on_message)
                    c->on_message(c, (const char*)arena + msgs[m].arena_off, (size_t)msgs[m].len,
                                  msgs[m].opcode);
            dispatch_control(c, d->opcode, wire ? wire + d->payload_off : NULL, d->payload_len);
        }
    }
    for (; m < nm; ++m)
        if (c->on_message)
            c->on_message(c, (const char*)arena + msgs[m].arena_off, (size_t)msgs[m].len,
                          msgs[m].opcode);
    if (last_ctl != NULL)
        dispatch_control(c, lh.opcode, last_ctl + lhead + (lh.mask ? 4u : 0u), lh.payload_length);
    /* fragmented_opcode is what the last first fragment wrote there: the reference sets it when a
     * TEXT / BINARY frame with FIN clear arrives and no message is open (:972) and never clears
     * it, so it outlives the message; a zero-length first fragment writes it too */
    if (desc != NULL) {
        for (uint32_t i = 0; i < nd; ++i)
            if ((desc[i].opcode == UVHTTP_WS_OPCODE_TEXT || desc[i].opcode == UVHTTP_WS_OPCODE_BINARY) &&
                !(desc[i].flags & UVHTTP_WS_FLAG_FIN))
                c->fragmented_opcode = (uvhttp_ws_opcode_t)desc[i].opcode;
    } else { /* summary-only: a message of several frames began with such a fragment, and only the
                last frame can be an empty one (every other fills its >= 140-byte slot) */
        for (uint32_t k = 0; k < nm; ++k)
            if (msgs[k].first_frame != msgs[k].last_frame)
                c->fragmented_opcode = (uvhttp_ws_opcode_t)msgs[k].opcode;
        if (last_start) c->fragmented_opcode = (uvhttp_ws_opcode_t)last_start;
    }
    if (open) { /* the open message as append_fragment left it: capacity = first fragment
                   doubled until it holds everything appended (src/uvhttp_websocket.c:794-816) */
        const uvhttp_ws_message_desc_t* d = &msgs[nm];
        size_t cap = (size_t)d->reserved;
        while (cap < (size_t)d->len) {
            if (cap > SIZE_MAX / 2) return UVHTTP_ERROR_INVALID_PARAM;
            cap *= 2;
        }
        uint8_t* buf = (uint8_t*)malloc(cap);
        if (buf == NULL) return UVHTTP_ERROR_INVALID_PARAM;
        memcpy(buf, arena + d->arena_off, (size_t)d->len);
        c->fragmented_message = buf;
        c->fragmented_size = (size_t)d->len;
        c->fragmented_capacity = cap;
        c->fragmented_opcode = (uvhttp_ws_opcode_t)d->opcode;
    }
    if (summary->status != 0 && desc != NULL && nd < summary->n_frames)
        failed_start_keeps_its_opcode(c, summary, &desc[nd]);
    return summary->status == 0 ? UVHTTP_OK : UVHTTP_ERROR_INVALID_PARAM;
}

/* ---- stream decode, host side (include/uvhttp_ws_amd.h) ---------------------------------- */

void uvhttp_ws_stream_init(const struct uvhttp_ws_connection* c, uint64_t begin, uint64_t len,
                           uvhttp_ws_stream_t* out) {
    if (c == NULL || out == NULL) return;
    memset(out, 0, sizeof(*out));
    out->begin = begin;
    out->len = len;
    out->recv_buffer_size = c->recv_buffer_size;
    out->pending_bytes = c->fragmented_message != NULL ? c->fragmented_size : 0;
    out->pending_opcode = (int32_t)c->fragmented_opcode;
    out->max_frame_size = c->config.max_frame_size;
    out->max_message_size = c->config.max_message_size;
    out->is_server = c->is_server;
}

uvhttp_error_t uvhttp_ws_deliver_stream(struct uvhttp_ws_connection* c, const uint8_t* wire,
                                        const uvhttp_ws_frame_desc_t* desc,
                                        const uvhttp_ws_stream_t* s,
                                        const uvhttp_ws_stream_result_t* r) {
    if (c == NULL || s == NULL || r == NULL || (s->len && wire == NULL))
        return UVHTTP_ERROR_INVALID_PARAM;
    /* nothing ran on the connection: a malformed descriptor, too many frames for the batch,
     * a device fault, or the first call failed its growth check and returned before touching
     * the buffer (src/uvhttp_websocket.c:836-857) */
    if (r->first_status == UVHTTP_WS_FRAME_ERR_CAPACITY ||
        r->first_status == UVHTTP_WS_FRAME_ERR_LAYOUT ||
        r->first_status == UVHTTP_WS_FRAME_ERR_DEVICE ||
        (r->first_status == UVHTTP_WS_FRAME_ERR_BUFFER && r->calls <= 1))
        return UVHTTP_ERROR_INVALID_PARAM;
    if (r->consumed_bytes > r->buffered_end || r->buffered_end > s->len ||
        (r->n_delivered && desc == NULL))
        return UVHTTP_ERROR_INVALID_PARAM;
    if (r->recv_buffer_size != c->recv_buffer_size) {
        uint8_t* nb = (uint8_t*)realloc(c->recv_buffer, (size_t)r->recv_buffer_size);
        if (nb == NULL) return UVHTTP_ERROR_INVALID_PARAM;
        c->recv_buffer = nb;
        c->recv_buffer_size = (size_t)r->recv_buffer_size;
    }
    const uint8_t* base = wire + s->begin;
    for (uint32_t k = 0; k < r->n_delivered; ++k) {
        const uvhttp_ws_frame_desc_t* d = &desc[r->first_frame + k];
        uvhttp_ws_frame_header_t h;
        memset(&h, 0, sizeof(h));
        h.fin = (d->flags & UVHTTP_WS_FLAG_FIN) ? 1 : 0;
        h.mask = (d->flags & UVHTTP_WS_FLAG_MASK) ? 1 : 0;
        h.opcode = d->opcode & 0x0F;
        h.payload_length = d->payload_len;
        const uint8_t* payload = d->payload_len ? wire + d->payload_off : NULL;
        if (dispatch_frame(c, &h, payload) != 0) break; /* cannot happen after a clean decode */
    }
    /* what the calls leave buffered: the stream bytes after the delivered frames, up to the
     * end of the last call that ran */
    const size_t rest = (size_t)(r->buffered_end - r->consumed_bytes);
    if (rest) memmove(c->recv_buffer, base + r->consumed_bytes, rest);
    c->recv_buffer_pos = rest;
    /* a complete data frame rejected by the fragment state machine: the reference unmasked it
     * in recv_buffer (:944) before its fragment checks failed (:964-1000), and those checks
     * may already have changed the fragment state (a start records its opcode before the
     * size check) — replay that frame's unmask and dispatch, which fails the same way */
    if ((r->first_status == UVHTTP_WS_FRAME_ERR_FRAGMENT ||
         r->first_status == UVHTTP_WS_FRAME_ERR_MESSAGE) && desc != NULL) {
        const uvhttp_ws_frame_desc_t* d = &desc[r->first_frame + r->n_delivered];
        const size_t at = (size_t)(d->payload_off - s->begin - r->consumed_bytes);
        if (d->payload_len && at + d->payload_len <= rest) {
            uint8_t* payload = c->recv_buffer + at;
            if (d->flags & UVHTTP_WS_FLAG_MASK) {
                uint8_t key[4];
                memcpy(key, &d->masking_key, 4); /* k0 = low byte */
                uvhttp_ws_apply_mask(payload, (size_t)d->payload_len, key);
            }
            uvhttp_ws_frame_header_t h;
            memset(&h, 0, sizeof(h));
            h.fin = (d->flags & UVHTTP_WS_FLAG_FIN) ? 1 : 0;
            h.mask = (d->flags & UVHTTP_WS_FLAG_MASK) ? 1 : 0;
            h.opcode = d->opcode & 0x0F;
            h.payload_length = d->payload_len;
            (void)dispatch_frame(c, &h, payload);
        } else if (!d->payload_len) {
            uvhttp_ws_frame_header_t h;
            memset(&h, 0, sizeof(h));
            h.fin = (d->flags & UVHTTP_WS_FLAG_FIN) ? 1 : 0;
            h.opcode = d->opcode & 0x0F;
            (void)dispatch_frame(c, &h, NULL);
        }
    }
    return r->status == 0 ? UVHTTP_OK : UVHTTP_ERROR_INVALID_PARAM;
}

/* Copy of a read into the batcher's pinned arena (ws_batcher.hip; internal).  The arena is
 * only read again by the DMA engine, so whole vectors go out with non-temporal stores: no
 * read-for-ownership of the destination lines, no cache pollution (glibc memcpy switches to
 * streaming stores only far above libuv's 16 KiB reads).  32-byte AVX2 streaming stores where
 * the CPU has them: 91 GB/s into pinned memory on the MI355X box's EPYC 9575F against 54-59 GB/s
 * for 16-byte SSE2 ones and 45 GB/s for memcpy (tools/copy_probe.cpp,
 * profiles/r03p42_copy_probe.jsonl).  Other targets (the host decoder builds anywhere) copy
 * with memcpy and fence with a full barrier. */
#if defined(__x86_64__) || defined(__i386__)
#include <immintrin.h>

__attribute__((target("avx2"))) static void copy_stream_avx2(uint8_t* d, const uint8_t* s, size_t len) {
    const size_t head = (32u - ((uintptr_t)d & 31u)) & 31u;
    memcpy(d, s, head);
    d += head;
    s += head;
    len -= head;
    size_t i = 0;
    for (; i + 128 <= len; i += 128) {
        const __m256i a = _mm256_loadu_si256((const __m256i*)(s + i));
        const __m256i b = _mm256_loadu_si256((const __m256i*)(s + i + 32));
        const __m256i c = _mm256_loadu_si256((const __m256i*)(s + i + 64));
        const __m256i e = _mm256_loadu_si256((const __m256i*)(s + i + 96));
        _mm256_stream_si256((__m256i*)(d + i), a);
        _mm256_stream_si256((__m256i*)(d + i + 32), b);
        _mm256_stream_si256((__m256i*)(d + i + 64), c);
        _mm256_stream_si256((__m256i*)(d + i + 96), e);
    }
    for (; i + 32 <= len; i += 32)
        _mm256_stream_si256((__m256i*)(d + i), _mm256_loadu_si256((const __m256i*)(s + i)));
    memcpy(d + i, s + i, len - i);
}

static void copy_stream_sse2(uint8_t* d, const uint8_t* s, size_t len) {
    const size_t head = (16u - ((uintptr_t)d & 15u)) & 15u;
    memcpy(d, s, head);
    d += head;
    s += head;
    len -= head;
    size_t i = 0;
    for (; i + 64 <= len; i += 64) {
        const __m128i a = _mm_loadu_si128((const __m128i*)(s + i));
        const __m128i b = _mm_loadu_si128((const __m128i*)(s + i + 16));
        const __m128i c = _mm_loadu_si128((const __m128i*)(s + i + 32));
        const __m128i e = _mm_loadu_si128((const __m128i*)(s + i + 48));
        _mm_stream_si128((__m128i*)(d + i), a);
        _mm_stream_si128((__m128i*)(d + i + 16), b);
        _mm_stream_si128((__m128i*)(d + i + 32), c);
        _mm_stream_si128((__m128i*)(d + i + 48), e);
    }
    for (; i + 16 <= len; i += 16)
        _mm_stream_si128((__m128i*)(d + i), _mm_loadu_si128((const __m128i*)(s + i)));
    memcpy(d + i, s + i, len - i);
}

/* The streaming stores of copy_stream are weakly ordered: make them visible before a DMA engine
 * reads the arena (the batcher calls this before each H2D of it).  One fence per upload, not one
 * per 16 KiB read: a fence per call cost a third of the copy rate (58.8 vs 91 GB/s,
 * profiles/r03p44_numa_copy_e2e.txt). */
__attribute__((visibility("hidden"))) void uvhttp_ws_amd_copy_fence(void) { _mm_sfence(); }
#else
__attribute__((visibility("hidden"))) void uvhttp_ws_amd_copy_fence(void) {
    __atomic_thread_fence(__ATOMIC_SEQ_CST);
}
#endif

__attribute__((visibility("hidden"))) void uvhttp_ws_amd_copy_stream(void* dst, const void* src,
                                                                     size_t len) {
#if defined(__x86_64__) || defined(__i386__)
    static int have_avx2 = -1;
    if (len < 1024) {
        memcpy(dst, src, len);
        return;
    }
    if (have_avx2 < 0) {
#ifdef UVWS_EXPERIMENTS  /* UVHTTP_WS_COPY_SSE2=1: the SSE2 path, for tests on AVX2 machines */
        const char* f = getenv("UVHTTP_WS_COPY_SSE2");
        have_avx2 = (__builtin_cpu_supports("avx2") && !(f && f[0] == '1')) ? 1 : 0;
#else
        have_avx2 = __builtin_cpu_supports("avx2") ? 1 : 0;
#endif
    }
    if (have_avx2)
        copy_stream_avx2((uint8_t*)dst, (const uint8_t*)src, len);
    else
        copy_stream_sse2((uint8_t*)dst, (const uint8_t*)src, len);
#else
    memcpy(dst, src, len);
#endif
}

/* ---- UTF-8 check of TEXT payloads (RFC 6455 §5.6; the reference has none) --------------- */
/* The state is the open sequence itself: pend[0, n) are its bytes so far, in order.  So the
 * state after a device PREFIX verdict (uvhttp_ws_gpu_validate_utf8) is n = tail and pend = the
 * last `tail` bytes of the message's arena range.  The rules are utf8_rules.h's, shared with
 * the device kernels; runs of ASCII are skipped eight bytes at a time. */
int uvhttp_ws_utf8_feed(uvhttp_ws_utf8_state_t* st, const uint8_t* data, size_t len) {
    if (st == NULL || st->n > 3 || (data == NULL && len != 0)) return -1;
    uint32_t p1 = 0, p2 = 0, p3 = 0;
    if (st->n == 1) {
        p1 = st->pend[0];
    } else if (st->n == 2) {
        p2 = st->pend[0], p1 = st->pend[1];
    } else if (st->n == 3) {
        p3 = st->pend[0], p2 = st->pend[1], p1 = st->pend[2];
    }
    size_t i = 0;
    while (i < len) {
        if (p1 < 0x80u) { /* no sequence open: p2, p3 cannot matter after an ASCII byte */
            while (i + 8 <= len) {
                uint64_t w;
                memcpy(&w, data + i, 8);
                if (w & 0x8080808080808080ull) break;
                i += 8;
                p1 = p2 = p3 = 0;
            }
            if (i == len) break;
        }
        const uint32_t b = data[i++];
        if (uvws_utf8_bad(b, p1, p2, p3)) return -1;
        p3 = p2, p2 = p1, p1 = b;
    }
    const uint32_t n = uvws_utf8_open(p1, p2, p3);
    st->n = (uint8_t)n;
    st->pend[0] = (uint8_t)(n == 1 ? p1 : n == 2 ? p2 : n == 3 ? p3 : 0);
    st->pend[1] = (uint8_t)(n == 2 ? p1 : n == 3 ? p2 : 0);
    st->pend[2] = (uint8_t)(n == 3 ? p1 : 0);
    return 0;
}

int uvhttp_ws_utf8_finish(const uvhttp_ws_utf8_state_t* st) {
    return (st != NULL && st->n == 0) ? 0 : -1;
}

/* One connection's delivered frames, walked in order (the host twin of
 * uvhttp_ws_gpu_validate_utf8_streams / _inplace): the decoder's message membership, feed per
 * TEXT frame, finish at FIN.  After the first INVALID / BAD_RANGE frame only the membership is
 * still followed (n_text_frames counts every TEXT frame). */
static int utf8_range_ok(uint64_t wire_len, uint64_t off, uint64_t len) {
    return len <= wire_len && off <= wire_len - len;
}

int uvhttp_ws_utf8_judge_frames(const uint8_t* wire, uint64_t wire_len,
                                const uvhttp_ws_frame_desc_t* desc, uint32_t first_frame,
                                uint32_t n_delivered, int open_opcode,
                                const uvhttp_ws_utf8_state_t* state_in, uint32_t flags,
                                uvhttp_ws_utf8_conn_verdict_t* out) {
    if (out == NULL || (desc == NULL && n_delivered != 0) || (wire == NULL && wire_len != 0)) return -1;
    memset(out, 0, sizeof(*out));
    out->first_invalid = 0xFFFFFFFFu;
    int op = (open_opcode == 1 || open_opcode == 2) ? open_opcode : 0;
    uvhttp_ws_utf8_state_t st;
    memset(&st, 0, sizeof(st));
    if (op == 1 && state_in != NULL) {
        st = *state_in;
        if (st.n > 3) st.n = 3;
    }
    uint8_t status = UVHTTP_WS_UTF8_VALID;
    for (uint32_t i = 0; i < n_delivered; ++i) {
        const uvhttp_ws_frame_desc_t* d = &desc[(uint64_t)first_frame + i];
        if (d->status != UVHTTP_WS_FRAME_OK) break; /* not delivered: the caller's count was wrong */
        const int fop = d->opcode;
        const int fin = (d->flags & UVHTTP_WS_FLAG_FIN) != 0;
        const int judging = status == UVHTTP_WS_UTF8_VALID;
        if (fop >= 8) {
            if (fop == 8 && (flags & UVHTTP_WS_UTF8_CHECK_CLOSE) && d->payload_len > 2 && judging) {
                if (!utf8_range_ok(wire_len, d->payload_off, d->payload_len)) {
                    status = UVHTTP_WS_UTF8_BAD_RANGE;
                } else {
                    uvhttp_ws_utf8_state_t cs;
                    memset(&cs, 0, sizeof(cs));
                    if (uvhttp_ws_utf8_feed(&cs, wire + d->payload_off + 2, (size_t)(d->payload_len - 2)) != 0 ||
                        uvhttp_ws_utf8_finish(&cs) != 0)
                        status = UVHTTP_WS_UTF8_INVALID;
                }
                if (status != UVHTTP_WS_UTF8_VALID) out->first_invalid = first_frame + i;
            }
            continue;
        }
        if (fop == 1 || fop == 2) {
            op = fop;
            memset(&st, 0, sizeof(st));
        } else if (fop != 0) {
            continue; /* reserved opcodes are never delivered */
        }
        if (op == 1) {
            out->n_text_frames++;
            if (judging) {
                if (!utf8_range_ok(wire_len, d->payload_off, d->payload_len))
                    status = UVHTTP_WS_UTF8_BAD_RANGE;
                else if (uvhttp_ws_utf8_feed(&st, d->payload_len ? wire + d->payload_off : NULL,
                                             (size_t)d->payload_len) != 0 ||
                         (fin && uvhttp_ws_utf8_finish(&st) != 0))
                    status = UVHTTP_WS_UTF8_INVALID;
                if (status != UVHTTP_WS_UTF8_VALID) out->first_invalid = first_frame + i;
            }
        }
        if (fin) {
            op = 0;
            memset(&st, 0, sizeof(st));
        }
    }
    if (status == UVHTTP_WS_UTF8_VALID && op == 1) {
        status = UVHTTP_WS_UTF8_PREFIX;
        out->state = st;
    }
    out->status = status;
    return 0;
}

/* ---- control replies: PONG / CLOSE echo frames of one connection's delivered frames -------- */
/* The host twin of uvhttp_ws_gpu_control_replies_streams / _inplace, and what dispatch_frame
 * hands the control sink (on_close_frame's echo, the PING branch), written as the frames
 * uvhttp_ws_build_frame(..., opcode, mask = !is_server, fin = 1) makes of them. */
int uvhttp_ws_control_replies(const uint8_t* wire, uint64_t wire_len,
                              const uvhttp_ws_frame_desc_t* desc, uint32_t first_frame,
                              uint32_t n_delivered, int is_server, int enable,
                              const uint32_t* mask_keys, uint32_t flags, uint8_t* out,
                              uint64_t out_cap, uint64_t* out_off, uint32_t max_replies,
                              uvhttp_ws_reply_conn_t* r) {
    if (r == NULL || out_off == NULL || (desc == NULL && n_delivered != 0) ||
        (wire == NULL && wire_len != 0) || (out == NULL && out_cap != 0))
        return -1;
    memset(r, 0, sizeof(*r));
    for (uint64_t j = 0; j <= max_replies; ++j) out_off[j] = 0;
    const int masked = !is_server;
    const uint64_t hdr = masked ? 6u : 2u;
    if (enable && masked && mask_keys == NULL) r->status = UVHTTP_WS_REPLY_NO_KEYS;
    /* two passes over the same walk: size (and the statuses), then emit */
    for (int pass = 0; pass < 2; ++pass) {
        uint64_t n = 0, bytes = 0;
        int closed = 0;
        for (uint32_t i = 0; i < n_delivered; ++i) {
            const uvhttp_ws_frame_desc_t* d = &desc[(uint64_t)first_frame + i];
            if (d->status != UVHTTP_WS_FRAME_OK) continue; /* not delivered: no reply */
            const int op = d->opcode;
            if (op != UVHTTP_WS_OPCODE_PING && op != UVHTTP_WS_OPCODE_CLOSE) continue;
            const int after = closed;
            if (op == UVHTTP_WS_OPCODE_CLOSE) closed = 1;
            if (pass == 0 && op == UVHTTP_WS_OPCODE_CLOSE) r->closed = 1;
            if (!enable) continue;
            uint64_t len = d->payload_len;
            if (op == UVHTTP_WS_OPCODE_CLOSE) len = len < 2 ? 0 : len > 127 ? 127 : len;
            if (len > 125) len = 125; /* a delivered control frame has at most 125 bytes */
            if (pass == 0 && len != 0 && !utf8_range_ok(wire_len, d->payload_off, len) &&
                r->status == UVHTTP_WS_REPLY_OK)
                r->status = UVHTTP_WS_REPLY_BAD_RANGE;
            if (after && !(flags & UVHTTP_WS_REPLY_AFTER_CLOSE)) continue;
            if (pass == 1) {
                uint8_t* o = out + bytes;
                const uint32_t key = masked ? mask_keys[n] : 0u;
                o[0] = (uint8_t)(0x80u | (op == UVHTTP_WS_OPCODE_PING ? UVHTTP_WS_OPCODE_PONG
                                                                      : UVHTTP_WS_OPCODE_CLOSE));
                o[1] = (uint8_t)((masked ? 0x80u : 0u) | len);
                if (masked)
                    for (int k = 0; k < 4; ++k) o[2 + k] = (uint8_t)(key >> (8 * k));
                for (uint64_t b = 0; b < len; ++b)
                    o[hdr + b] = (uint8_t)(wire[d->payload_off + b] ^ (uint8_t)(key >> (8 * (b & 3))));
                out_off[n] = bytes;
            }
            n++;
            bytes += hdr + len;
        }
        if (pass == 0) {
            if (r->status != UVHTTP_WS_REPLY_OK) return 0; /* NO_KEYS / BAD_RANGE: no replies */
            r->n_replies = (uint32_t)n;
            r->out_len = bytes > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)bytes;
            if (n > max_replies || bytes > out_cap) {
                r->status = UVHTTP_WS_REPLY_ERR_CAPACITY;
                return 0;
            }
            if (n == 0) return 0;
        } else {
            for (uint64_t j = n; j <= max_replies; ++j) out_off[j] = bytes;
        }
    }
    return 0;
}

/* ---- echo of data messages: the echo server's frames of one connection's delivered frames -- */
/* The host twin of uvhttp_ws_gpu_echo_messages_streams / _inplace and the statement of their
 * rules (include/uvhttp_ws_amd.h): what on_message -> uvhttp_ws_send_text / _send_binary puts on
 * the wire for every message whose FIN frame is delivered while state == OPEN, written as the
 * frames uvhttp_ws_build_frame(..., opcode, mask = !is_server, fin = 1) makes of them, and the
 * bytes of the message still open afterwards. */
static int echo_is_data(const uvhttp_ws_frame_desc_t* d) {
    return d->status == UVHTTP_WS_FRAME_OK && d->opcode <= UVHTTP_WS_OPCODE_BINARY;
}

/* the message's bytes in order — the carry when it was carried in (first == -1), then the data
 * payloads of desc[lo, hi] — to dst, XOR-ed with the key from message offset 0 on */
static void echo_gather(uint8_t* dst, const uint8_t* wire, const uvhttp_ws_frame_desc_t* desc,
                        uint64_t lo, uint64_t hi, const uint8_t* carry, uint64_t carry_len,
                        uint32_t key) {
    uint64_t m = 0;
    for (uint64_t b = 0; b < carry_len; ++b, ++m) dst[m] = (uint8_t)(carry[b] ^ (uint8_t)(key >> (8 * (m & 3))));
    for (uint64_t i = lo; i <= hi; ++i) {
        if (!echo_is_data(&desc[i])) continue;
        const uint8_t* p = wire + desc[i].payload_off;
        for (uint64_t b = 0; b < desc[i].payload_len; ++b, ++m)
            dst[m] = (uint8_t)(p[b] ^ (uint8_t)(key >> (8 * (m & 3))));
    }
}

int uvhttp_ws_echo_messages(const uint8_t* wire, uint64_t wire_len,
                            const uvhttp_ws_frame_desc_t* desc, uint32_t first_frame,
                            uint32_t n_delivered, int is_server, int enable,
                            const uint32_t* mask_keys, uint32_t flags, int pending_opcode,
                            uint64_t pending_bytes, const uint8_t* carry, uint64_t carry_len,
                            uint8_t* out, uint64_t out_cap, uint64_t* out_off,
                            uint32_t max_echoes, uint8_t* open, uint64_t open_cap,
                            uvhttp_ws_echo_conn_t* r) {
    if (r == NULL || out_off == NULL || (desc == NULL && n_delivered != 0) ||
        (wire == NULL && wire_len != 0) || (out == NULL && out_cap != 0) ||
        (carry == NULL && carry_len != 0))
        return -1;
    memset(r, 0, sizeof(*r));
    for (uint64_t j = 0; j <= max_echoes; ++j) out_off[j] = 0;
    if (!enable) return 0; /* skipped as a whole */
    const int masked = !is_server;
    if (masked && mask_keys == NULL) {
        r->status = UVHTTP_WS_ECHO_NO_KEYS;
        return 0;
    }
    if (pending_bytes != 0 && carry_len != pending_bytes) {
        r->status = UVHTTP_WS_ECHO_NO_CARRY;
        return 0;
    }
    /* two passes over the same walk: size (and BAD_RANGE), then emit */
    for (int pass = 0; pass < 2; ++pass) {
        uint64_t n = 0, bytes = 0;
        int closed = 0;
        /* the open message: is there one, its opcode, its length, whether it was carried in and
         * the first descriptor that can hold a fragment of it */
        int cur = pending_bytes != 0, cur_op = pending_opcode & 0x0F, carried = cur;
        uint64_t cur_len = pending_bytes, lo = first_frame;
        for (uint32_t i = 0; i < n_delivered; ++i) {
            const uint64_t f = (uint64_t)first_frame + i;
            const uvhttp_ws_frame_desc_t* d = &desc[f];
            if (d->status != UVHTTP_WS_FRAME_OK) continue; /* not delivered */
            if (d->opcode == UVHTTP_WS_OPCODE_CLOSE) closed = 1;
            if (!echo_is_data(d)) continue;
            if (pass == 0 && d->payload_len != 0 && !utf8_range_ok(wire_len, d->payload_off, d->payload_len)) {
                r->status = UVHTTP_WS_ECHO_BAD_RANGE;
                return 0;
            }
            if (d->opcode != UVHTTP_WS_OPCODE_CONTINUATION) {
                cur = 1;
                cur_op = d->opcode;
                carried = 0;
                cur_len = 0;
                lo = f;
            } else if (!cur) {
                continue; /* a CONTINUATION of nothing */
            }
            cur_len += d->payload_len;
            if (!(d->flags & UVHTTP_WS_FLAG_FIN)) continue;
            cur = 0;
            if (closed || ((flags & UVHTTP_WS_ECHO_SERVER_SEND) && cur_len == 0)) continue;
            const uint64_t hdr = (cur_len <= 125 ? 2u : cur_len <= 65535 ? 4u : 10u) + (masked ? 4u : 0u);
            if (pass == 1) {
                uint8_t* o = out + bytes;
                const uint32_t key = masked ? mask_keys[n] : 0u;
                const int op = (flags & UVHTTP_WS_ECHO_SERVER_SEND) ? UVHTTP_WS_OPCODE_TEXT : cur_op;
                uint64_t h = 2;
                o[0] = (uint8_t)(0x80u | (unsigned)op);
                if (cur_len <= 125) {
                    o[1] = (uint8_t)cur_len;
                } else if (cur_len <= 65535) {
                    o[1] = 126;
                    o[2] = (uint8_t)(cur_len >> 8);
                    o[3] = (uint8_t)cur_len;
                    h = 4;
                } else {
                    o[1] = 127;
                    for (int k = 0; k < 8; ++k) o[2 + k] = (uint8_t)(cur_len >> (8 * (7 - k)));
                    h = 10;
                }
                if (masked) {
                    o[1] |= 0x80u;
                    for (int k = 0; k < 4; ++k) o[h + k] = (uint8_t)(key >> (8 * k));
                }
                echo_gather(o + hdr, wire, desc, lo, f, carry, carried ? carry_len : 0, key);
                out_off[n] = bytes;
            }
            n++;
            bytes += hdr + cur_len;
        }
        if (!cur || cur_len == 0) {
            cur = 0;
            cur_len = 0;
        }
        if (pass == 0) {
            r->n_echoes = (uint32_t)n;
            r->out_len = bytes;
            r->open_len = cur_len;
            if (n > max_echoes || bytes > out_cap || (open != NULL && cur_len > open_cap)) {
                r->status = UVHTTP_WS_ECHO_ERR_CAPACITY;
                return 0;
            }
            r->open_opcode = (uint8_t)(cur ? cur_op : 0);
        } else {
            for (uint64_t j = n; j <= max_echoes; ++j) out_off[j] = bytes;
            if (cur && open != NULL && n_delivered != 0)
                echo_gather(open, wire, desc, lo, (uint64_t)first_frame + n_delivered - 1, carry,
                            carried ? carry_len : 0, 0u);
            else if (cur && open != NULL)
                memcpy(open, carry, (size_t)carry_len);
        }
    }
    return 0;
}

/* ---- answers: one connection's echoes and control replies in frame order -------------------- */
/* The host twin of uvhttp_ws_gpu_answer_messages_streams / _inplace and the statement of their
 * rule (include/uvhttp_ws_amd.h): what uvhttp_ws_process_data hands uvhttp_ws_send_frame as it
 * goes — the PONG where the PING stood, the echo where the message's FIN frame stood, the CLOSE
 * echo where the CLOSE stood — as one run of frames. */
static uint64_t answer_ctl_len(const uvhttp_ws_frame_desc_t* d) {
    uint64_t len = d->payload_len;
    if (d->opcode == UVHTTP_WS_OPCODE_CLOSE && len < 2) len = 0;
    return len > 125 ? 125 : len; /* a delivered control frame has at most 125 bytes */
}

int uvhttp_ws_answer_messages(const uint8_t* wire, uint64_t wire_len,
                              const uvhttp_ws_frame_desc_t* desc, uint32_t first_frame,
                              uint32_t n_delivered, int is_server, int enable,
                              const uint32_t* mask_keys, uint32_t flags, int pending_opcode,
                              uint64_t pending_bytes, const uint8_t* carry, uint64_t carry_len,
                              uint8_t* out, uint64_t out_cap, uint64_t* out_off,
                              uint32_t max_answers, uint8_t* open, uint64_t open_cap,
                              uvhttp_ws_answer_conn_t* r, uvhttp_ws_reply_conn_t* q) {
    if (r == NULL || out_off == NULL || (desc == NULL && n_delivered != 0) ||
        (wire == NULL && wire_len != 0) || (out == NULL && out_cap != 0) ||
        (carry == NULL && carry_len != 0) ||
        (flags & ~(UVHTTP_WS_ANSWER_SERVER_SEND | UVHTTP_WS_ANSWER_REPLY_AFTER_CLOSE)) != 0)
        return -1;
    memset(r, 0, sizeof(*r));
    if (q != NULL) memset(q, 0, sizeof(*q));
    for (uint64_t j = 0; j <= max_answers; ++j) out_off[j] = 0;
    /* closed: a CLOSE was delivered, whatever else holds */
    for (uint32_t i = 0; i < n_delivered; ++i) {
        const uvhttp_ws_frame_desc_t* d = &desc[(uint64_t)first_frame + i];
        if (d->status == UVHTTP_WS_FRAME_OK && d->opcode == UVHTTP_WS_OPCODE_CLOSE) r->closed = 1;
    }
    if (q != NULL) q->closed = r->closed;
    if (!enable) return 0; /* skipped as a whole */
    const int masked = !is_server;
    if (masked && mask_keys == NULL) {
        r->status = UVHTTP_WS_ECHO_NO_KEYS;
        if (q != NULL) q->status = UVHTTP_WS_REPLY_NO_KEYS;
        return 0;
    }
    if (pending_bytes != 0 && carry_len != pending_bytes) {
        r->status = UVHTTP_WS_ECHO_NO_CARRY;
        return 0;
    }
    /* BAD_RANGE: every delivered data frame and every delivered PING / CLOSE, answered or not */
    for (uint32_t i = 0; i < n_delivered; ++i) {
        const uvhttp_ws_frame_desc_t* d = &desc[(uint64_t)first_frame + i];
        if (d->status != UVHTTP_WS_FRAME_OK) continue;
        uint64_t len;
        if (echo_is_data(d)) len = d->payload_len;
        else if (d->opcode == UVHTTP_WS_OPCODE_PING || d->opcode == UVHTTP_WS_OPCODE_CLOSE) len = answer_ctl_len(d);
        else continue;
        if (len != 0 && !utf8_range_ok(wire_len, d->payload_off, len)) {
            r->status = UVHTTP_WS_ECHO_BAD_RANGE;
            if (q != NULL) q->status = UVHTTP_WS_REPLY_BAD_RANGE;
            return 0;
        }
    }
    /* two passes over the same walk: size, then emit */
    for (int pass = 0; pass < 2; ++pass) {
        uint64_t n = 0, bytes = 0, n_rep = 0, rep_bytes = 0;
        int closed = 0;
        int cur = pending_bytes != 0, cur_op = pending_opcode & 0x0F, carried = cur;
        uint64_t cur_len = pending_bytes, lo = first_frame;
        for (uint32_t i = 0; i < n_delivered; ++i) {
            const uint64_t f = (uint64_t)first_frame + i;
            const uvhttp_ws_frame_desc_t* d = &desc[f];
            if (d->status != UVHTTP_WS_FRAME_OK) continue; /* not delivered */
            if (d->opcode == UVHTTP_WS_OPCODE_PING || d->opcode == UVHTTP_WS_OPCODE_CLOSE) {
                const int after = closed;
                if (d->opcode == UVHTTP_WS_OPCODE_CLOSE) closed = 1;
                if (after && !(flags & UVHTTP_WS_ANSWER_REPLY_AFTER_CLOSE)) continue;
                const uint64_t len = answer_ctl_len(d), hdr = masked ? 6u : 2u;
                if (pass == 1) {
                    uint8_t* o = out + bytes;
                    const uint32_t key = masked ? mask_keys[n] : 0u;
                    o[0] = (uint8_t)(0x80u | (d->opcode == UVHTTP_WS_OPCODE_PING ? UVHTTP_WS_OPCODE_PONG
                                                                                 : UVHTTP_WS_OPCODE_CLOSE));
                    o[1] = (uint8_t)((masked ? 0x80u : 0u) | len);
                    if (masked)
                        for (int k = 0; k < 4; ++k) o[2 + k] = (uint8_t)(key >> (8 * k));
                    for (uint64_t b = 0; b < len; ++b)
                        o[hdr + b] = (uint8_t)(wire[d->payload_off + b] ^ (uint8_t)(key >> (8 * (b & 3))));
                    out_off[n] = bytes;
                }
                n++;
                n_rep++;
                bytes += hdr + len;
                rep_bytes += hdr + len;
                continue;
            }
            if (!echo_is_data(d)) continue;
            if (d->opcode != UVHTTP_WS_OPCODE_CONTINUATION) {
                cur = 1;
                cur_op = d->opcode;
                carried = 0;
                cur_len = 0;
                lo = f;
            } else if (!cur) {
                continue; /* a CONTINUATION of nothing */
            }
            cur_len += d->payload_len;
            if (!(d->flags & UVHTTP_WS_FLAG_FIN)) continue;
            cur = 0;
            if (closed || ((flags & UVHTTP_WS_ANSWER_SERVER_SEND) && cur_len == 0)) continue;
            const uint64_t hdr = (cur_len <= 125 ? 2u : cur_len <= 65535 ? 4u : 10u) + (masked ? 4u : 0u);
            if (pass == 1) {
                uint8_t* o = out + bytes;
                const uint32_t key = masked ? mask_keys[n] : 0u;
                const int op = (flags & UVHTTP_WS_ANSWER_SERVER_SEND) ? UVHTTP_WS_OPCODE_TEXT : cur_op;
                uint64_t h = 2;
                o[0] = (uint8_t)(0x80u | (unsigned)op);
                if (cur_len <= 125) {
                    o[1] = (uint8_t)cur_len;
                } else if (cur_len <= 65535) {
                    o[1] = 126;
                    o[2] = (uint8_t)(cur_len >> 8);
                    o[3] = (uint8_t)cur_len;
                    h = 4;
                } else {
                    o[1] = 127;
                    for (int k = 0; k < 8; ++k) o[2 + k] = (uint8_t)(cur_len >> (8 * (7 - k)));
                    h = 10;
                }
                if (masked) {
                    o[1] |= 0x80u;
                    for (int k = 0; k < 4; ++k) o[h + k] = (uint8_t)(key >> (8 * k));
                }
                echo_gather(o + hdr, wire, desc, lo, f, carry, carried ? carry_len : 0, key);
                out_off[n] = bytes;
            }
            n++;
            bytes += hdr + cur_len;
        }
        if (!cur || cur_len == 0) {
            cur = 0;
            cur_len = 0;
        }
        if (pass == 0) {
            r->n_answers = (uint32_t)n;
            r->n_replies = (uint32_t)n_rep;
            r->out_len = bytes;
            r->open_len = cur_len;
            if (n > max_answers || bytes > out_cap || (open != NULL && cur_len > open_cap)) {
                r->status = UVHTTP_WS_ECHO_ERR_CAPACITY;
                if (q != NULL) q->status = UVHTTP_WS_REPLY_ERR_CAPACITY; /* closed stays, the rest 0 */
                return 0;
            }
            if (q != NULL) {
                q->n_replies = (uint32_t)n_rep;
                q->out_len = rep_bytes > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)rep_bytes;
            }
            r->open_opcode = (uint8_t)(cur ? cur_op : 0);
        } else {
            for (uint64_t j = n; j <= max_answers; ++j) out_off[j] = bytes;
            if (cur && open != NULL && n_delivered != 0)
                echo_gather(open, wire, desc, lo, (uint64_t)first_frame + n_delivered - 1, carry,
                            carried ? carry_len : 0, 0u);
            else if (cur && open != NULL)
                memcpy(open, carry, (size_t)carry_len);
        }
    }
    return 0;
}

/* ---- relay of data messages: the room server's frames of a whole decoded batch -------------- */
/* The host twin of uvhttp_ws_gpu_relay_messages_streams and the statement of its rules
 * (include/uvhttp_ws_amd.h): every connection's frames are what uvhttp_ws_echo_messages makes of
 * it as a server without keys; they are laid out by (room, connection index), every room gets
 * its run and every receiver its room's. */
typedef struct {
    uint32_t key, s;
} relay_place_t;

static int relay_place_cmp(const void* pa, const void* pb) {
    const relay_place_t* a = (const relay_place_t*)pa;
    const relay_place_t* b = (const relay_place_t*)pb;
    if (a->key != b->key) return a->key < b->key ? -1 : 1;
    return a->s < b->s ? -1 : a->s > b->s;
}

/* connection s as the echo twin takes it: its considered frames and its usable carry */
typedef struct {
    uint32_t ff, nd;
    int pending_opcode;
    uint64_t pending_bytes, carry_len;
    const uint8_t* carry;
} relay_conn_t;

static relay_conn_t relay_conn(const uvhttp_ws_stream_t* st, const uvhttp_ws_stream_result_t* q,
                               uint32_t max_frames, const uint8_t* carry,
                               uint64_t carry_len, const uint64_t* carry_off, uint32_t s) {
    relay_conn_t c;
    c.ff = q->first_frame;
    c.nd = q->n_delivered;
    if (q->first_status == UVHTTP_WS_FRAME_ERR_CAPACITY || q->first_status == UVHTTP_WS_FRAME_ERR_LAYOUT ||
        q->first_status == UVHTTP_WS_FRAME_ERR_DEVICE)
        c.nd = 0;
    if (c.ff >= max_frames) c.nd = 0;
    else if (c.nd > max_frames - c.ff) c.nd = max_frames - c.ff;
    if (c.nd == 0) c.ff = 0;
    c.pending_opcode = st->pending_opcode;
    c.pending_bytes = st->pending_bytes;
    c.carry = NULL;
    c.carry_len = 0; /* unusable: the echo twin says NO_CARRY when pending_bytes != 0 */
    if (c.pending_bytes != 0 && carry != NULL && carry_off != NULL) {
        const uint64_t lo = carry_off[s], hi = carry_off[s + 1];
        if (hi >= lo && hi <= carry_len && hi - lo == c.pending_bytes) {
            c.carry = carry + lo;
            c.carry_len = c.pending_bytes;
        }
    }
    return c;
}

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
                             uvhttp_ws_echo_conn_t* conn, uvhttp_ws_relay_summary_t* summary) {
    if (streams == NULL || results == NULL || room == NULL || out_off == NULL || open_off == NULL ||
        conn == NULL || summary == NULL || (desc == NULL && max_frames != 0) ||
        (wire == NULL && wire_len != 0) || (out == NULL && out_cap != 0) || (rooms == NULL && n_rooms != 0) ||
        ((recv_room == NULL || sends == NULL) && n_receivers != 0) ||
        (sends != NULL && (send_stride < 8 || (send_stride & 3u))))
        return -1;
    memset(summary, 0, sizeof(*summary));
    relay_place_t* order = (relay_place_t*)malloc(((size_t)n_streams + 1) * sizeof(*order));
    if (order == NULL) return -1;
    /* sizes: every connection through the echo twin with no room for anything */
    uint64_t n_total = 0, bytes_total = 0, open_total = 0, dummy_off[1];
    for (uint32_t s = 0; s < n_streams; ++s) {
        const int en = enable == NULL || enable[s] != 0;
        const relay_conn_t c = relay_conn(&streams[s], &results[s], max_frames, carry, carry_len, carry_off, s);
        uvhttp_ws_echo_conn_t* r = &conn[s];
        memset(r, 0, sizeof(*r));
        order[s].key = room[s] < n_rooms ? room[s] : n_rooms;
        order[s].s = s;
        if (!en) continue;
        if (c.pending_bytes != 0 && c.carry_len != c.pending_bytes) {
            r->status = UVHTTP_WS_ECHO_NO_CARRY;
        } else if (room[s] >= n_rooms) {
            r->status = UVHTTP_WS_RELAY_BAD_ROOM;
            summary->n_bad_rooms++;
        } else {
            (void)uvhttp_ws_echo_messages(wire, wire_len, desc, c.ff, c.nd, 1, 1, NULL, flags, c.pending_opcode,
                                          c.pending_bytes, c.carry, c.carry_len, NULL, 0, dummy_off, 0, NULL, 0, r);
            if (r->status == UVHTTP_WS_ECHO_ERR_CAPACITY) r->status = UVHTTP_WS_ECHO_OK; /* sized only */
        }
        n_total += r->n_echoes;
        bytes_total += r->out_len;
        open_total += r->open_len;
    }
    for (uint32_t k = 0; k < n_receivers; ++k)
        if (recv_room[k] >= n_rooms) summary->n_bad_receivers++;
    summary->out_bytes = bytes_total;
    summary->open_bytes = open_total;
    summary->n_frames = (uint32_t)n_total;
    const int fits = n_total <= max_frames_out && bytes_total <= out_cap && (open == NULL || open_total <= open_cap);
    summary->status = fits ? UVHTTP_WS_ECHO_OK : UVHTTP_WS_ECHO_ERR_CAPACITY;
    for (uint64_t j = 0; j <= max_frames_out; ++j) out_off[j] = fits ? bytes_total : 0;
    for (uint32_t r = 0; r < n_rooms; ++r) memset(&rooms[r], 0, sizeof(rooms[r]));
    if (!fits) {
        for (uint32_t s = 0; s <= n_streams; ++s) open_off[s] = 0;
        for (uint32_t s = 0; s < n_streams; ++s) {
            memset(&conn[s], 0, sizeof(conn[s]));
            conn[s].status = UVHTTP_WS_ECHO_ERR_CAPACITY;
        }
    } else {
        /* the open messages' places: connection index order */
        uint64_t at_open = 0;
        for (uint32_t s = 0; s < n_streams; ++s) {
            open_off[s] = at_open;
            at_open += conn[s].open_len;
        }
        open_off[n_streams] = at_open;
        /* the frames: (room, connection index) order */
        qsort(order, n_streams, sizeof(*order), relay_place_cmp);
        order[n_streams].key = 0xFFFFFFFFu;
        uint64_t j = 0, at = 0;
        uint32_t p = 0;
        for (uint32_t r = 0; r <= n_rooms; ++r) { /* r == n_rooms: the connections after every room */
            if (r < n_rooms) {
                rooms[r].first_frame = (uint32_t)j;
                rooms[r].out_off = at;
            }
            for (; p < n_streams && order[p].key == r; ++p) {
                const uint32_t s = order[p].s;
                uvhttp_ws_echo_conn_t* q = &conn[s];
                const uint32_t n = q->n_echoes;
                q->first_echo = (uint32_t)j;
                if (q->status != UVHTTP_WS_ECHO_OK || (enable != NULL && enable[s] == 0)) continue;
                const relay_conn_t c = relay_conn(&streams[s], &results[s], max_frames, carry, carry_len, carry_off, s);
                uint64_t* off = (uint64_t*)malloc(((size_t)n + 1) * sizeof(*off));
                if (off == NULL) {
                    free(order);
                    return -1;
                }
                uvhttp_ws_echo_conn_t again;
                (void)uvhttp_ws_echo_messages(wire, wire_len, desc, c.ff, c.nd, 1, 1, NULL, flags, c.pending_opcode,
                                              c.pending_bytes, c.carry, c.carry_len, out != NULL ? out + at : NULL,
                                              q->out_len, off, n, open != NULL ? open + open_off[s] : NULL,
                                              q->open_len, &again);
                q->open_opcode = again.open_opcode;
                for (uint32_t k = 0; k < n; ++k) out_off[j + k] = at + off[k];
                free(off);
                j += n;
                at += q->out_len;
            }
            if (r < n_rooms) {
                rooms[r].n_frames = (uint32_t)j - rooms[r].first_frame;
                rooms[r].out_len = at - rooms[r].out_off;
            }
        }
    }
    for (uint32_t k = 0; k < n_receivers; ++k) {
        uint32_t* run = (uint32_t*)((char*)sends + (size_t)k * send_stride);
        const int ok = recv_room[k] < n_rooms;
        run[0] = ok ? rooms[recv_room[k]].first_frame : 0;
        run[1] = ok ? rooms[recv_room[k]].n_frames : 0;
    }
    free(order);
    return 0;
}

/* ---- the server's own CLOSE frames (1002 / 1007) for a decoded batch ------------------------ */
/* The host twin of uvhttp_ws_gpu_close_frames_streams and the statement of its rule
 * (include/uvhttp_ws_amd.h): what uvhttp_ws_close(NULL, conn, 1002, "protocol error")
 * (src/uvhttp_websocket.c:627-666) hands to uvhttp_ws_build_frame for every connection whose
 * decode failed, and a 1007 close with no reason for every connection whose text is not UTF-8. */
static const char close_reason_1002[] = "protocol error";

/* the code connection s is closed with (0 = no frame); *no_keys when only the key is missing */
static uint32_t close_code(const uvhttp_ws_stream_t* st, const uvhttp_ws_stream_result_t* res,
                           const uvhttp_ws_utf8_conn_verdict_t* verdict,
                           const uvhttp_ws_reply_conn_t* reply, int enabled, int have_keys,
                           int* no_keys) {
    *no_keys = 0;
    if (!enabled) return 0;
    const int32_t fs = res->first_status;
    if (fs == UVHTTP_WS_FRAME_ERR_CAPACITY || fs == UVHTTP_WS_FRAME_ERR_LAYOUT ||
        fs == UVHTTP_WS_FRAME_ERR_DEVICE)
        return 0;
    if (reply != NULL && reply->closed) return 0;
    uint32_t code = 0;
    if (verdict != NULL && verdict->status == UVHTTP_WS_UTF8_INVALID) code = 1007;
    else if (fs < 0) code = 1002;
    if (code != 0 && !st->is_server && !have_keys) {
        *no_keys = 1;
        return 0;
    }
    return code;
}

static uint32_t close_frame_len(uint32_t code, int masked) {
    if (code == 0) return 0;
    return 2u + (masked ? 4u : 0u) + 2u + (code == 1002 ? (uint32_t)(sizeof(close_reason_1002) - 1) : 0u);
}

int uvhttp_ws_close_frames(const uvhttp_ws_stream_t* streams, const uvhttp_ws_stream_result_t* results,
                           uint32_t n_streams, const uvhttp_ws_utf8_conn_verdict_t* verdict,
                           const uvhttp_ws_reply_conn_t* reply_conn, const uint8_t* enable,
                           const uint32_t* mask_keys, uint32_t flags, uint8_t* out, uint64_t out_cap,
                           uint64_t* out_off, uint32_t* runs, uint32_t run_stride,
                           uint32_t* const* clear_runs, const uint32_t* clear_stride, uint32_t n_clear,
                           uvhttp_ws_close_conn_t* conn, uvhttp_ws_close_summary_t* summary) {
    if (out_off == NULL || summary == NULL || (out == NULL && out_cap != 0) || flags != 0 ||
        (n_streams != 0 && (streams == NULL || results == NULL || conn == NULL)) ||
        n_streams > (1u << 31) || (runs != NULL && (run_stride < 8 || (run_stride & 3u))) ||
        n_clear > UVHTTP_WS_CLOSE_MAX_CLEAR || (n_clear != 0 && (clear_runs == NULL || clear_stride == NULL)))
        return -1;
    for (uint32_t k = 0; k < n_clear; ++k)
        if (clear_runs[k] == NULL || clear_stride[k] < 8 || (clear_stride[k] & 3u)) return -1;
    memset(summary, 0, sizeof(*summary));
    /* size, then emit */
    uint64_t bytes = 0;
    for (uint32_t s = 0; s < n_streams; ++s) {
        int nk;
        const uint32_t code = close_code(&streams[s], &results[s], verdict ? &verdict[s] : NULL,
                                         reply_conn ? &reply_conn[s] : NULL,
                                         enable == NULL || enable[s] != 0, mask_keys != NULL, &nk);
        bytes += close_frame_len(code, !streams[s].is_server);
        summary->n_1002 += code == 1002;
        summary->n_1007 += code == 1007;
    }
    summary->n_closes = summary->n_1002 + summary->n_1007;
    summary->out_bytes = bytes;
    const int fits = bytes <= out_cap;
    summary->status = fits ? UVHTTP_WS_CLOSE_OK : UVHTTP_WS_CLOSE_ERR_CAPACITY;
    uint64_t at = 0;
    uint32_t j = 0;
    for (uint32_t s = 0; s < n_streams; ++s) {
        uvhttp_ws_close_conn_t* r = &conn[s];
        memset(r, 0, sizeof(*r));
        uint32_t* run = runs ? (uint32_t*)((char*)runs + (size_t)s * run_stride) : NULL;
        if (!fits) {
            r->status = UVHTTP_WS_CLOSE_ERR_CAPACITY;
            out_off[s] = 0;
            if (run) run[0] = run[1] = 0;
            continue;
        }
        int nk;
        const int masked = !streams[s].is_server;
        const uint32_t code = close_code(&streams[s], &results[s], verdict ? &verdict[s] : NULL,
                                         reply_conn ? &reply_conn[s] : NULL,
                                         enable == NULL || enable[s] != 0, mask_keys != NULL, &nk);
        const uint32_t len = close_frame_len(code, masked);
        if (nk) r->status = UVHTTP_WS_CLOSE_NO_KEYS;
        if (run) {
            run[0] = j;
            run[1] = code ? 1u : 0u;
        }
        if (code) {
            const uint32_t key = masked ? mask_keys[s] : 0u;
            const uint32_t plen = len - (masked ? 6u : 2u);
            uint8_t* o = out + at;
            uint8_t* p = o + (masked ? 6 : 2);
            o[0] = (uint8_t)(0x80u | UVHTTP_WS_OPCODE_CLOSE);
            o[1] = (uint8_t)((masked ? 0x80u : 0u) | plen);
            if (masked)
                for (int k = 0; k < 4; ++k) o[2 + k] = (uint8_t)(key >> (8 * k));
            p[0] = (uint8_t)(code >> 8);
            p[1] = (uint8_t)code;
            for (uint32_t b = 2; b < plen; ++b) p[b] = (uint8_t)close_reason_1002[b - 2];
            for (uint32_t b = 0; b < plen; ++b) p[b] ^= (uint8_t)(key >> (8 * (b & 3)));
            r->code = code;
            r->out_len = len;
            out_off[j++] = at;
            at += len;
            if (code == 1007)
                for (uint32_t k = 0; k < n_clear; ++k)
                    ((uint32_t*)((char*)clear_runs[k] + (size_t)s * clear_stride[k]))[1] = 0;
        }
    }
    for (uint64_t k = fits ? j : n_streams; k <= n_streams; ++k) out_off[k] = fits ? at : 0;
    return 0;
}

/* ---- fail points: stop a connection at its first violation ---------------------------------- */
/* The host twin of uvhttp_ws_gpu_fail_points_streams and the statement of its rule
 * (include/uvhttp_ws_amd.h). */
static int fail_code_valid(uint32_t code) {
    return (code >= 1000 && code <= 1003) || (code >= 1007 && code <= 1014) || (code >= 3000 && code <= 4999);
}

int uvhttp_ws_fail_points(const uint8_t* wire, uint64_t wire_len, const uvhttp_ws_frame_desc_t* desc,
                          uint32_t max_frames, const uvhttp_ws_stream_result_t* results, uint32_t n_streams,
                          const uvhttp_ws_utf8_conn_verdict_t* verdict, const uint8_t* enable, uint32_t flags,
                          uvhttp_ws_stream_result_t* results_out, uvhttp_ws_utf8_conn_verdict_t* verdict_out,
                          uvhttp_ws_fail_conn_t* fail, uvhttp_ws_fail_summary_t* summary) {
    const uint32_t none = 0xFFFFFFFFu;
    if (desc == NULL || results == NULL || results_out == NULL || fail == NULL || summary == NULL ||
        (wire == NULL && wire_len != 0) || (verdict == NULL) != (verdict_out == NULL))
        return -1;
    if (((uintptr_t)desc & 7u) || ((uintptr_t)results & 7u) || ((uintptr_t)results_out & 7u) ||
        ((uintptr_t)summary & 7u) || ((uintptr_t)verdict & 3u) || ((uintptr_t)verdict_out & 3u) ||
        ((uintptr_t)fail & 3u))
        return -1;
    if ((flags & ~UVHTTP_WS_FAIL_CHECK_CLOSE) != 0 || max_frames > (1u << 28) || n_streams > (1u << 31)) return -1;
    uvhttp_ws_fail_summary_t sum;
    memset(&sum, 0, sizeof(sum));
    sum.first_failed = none;
    for (uint32_t s = 0; s < n_streams; ++s) {
        uvhttp_ws_stream_result_t r = results[s];  /* copies first: the outputs may be the inputs */
        uvhttp_ws_utf8_conn_verdict_t v;
        memset(&v, 0, sizeof(v));
        if (verdict != NULL) v = verdict[s];
        uvhttp_ws_fail_conn_t f;
        memset(&f, 0, sizeof(f));
        f.frame = none;
        const int32_t fs = r.first_status;
        const int judged = (enable == NULL || enable[s] != 0) && fs != UVHTTP_WS_FRAME_ERR_CAPACITY &&
                           fs != UVHTTP_WS_FRAME_ERR_LAYOUT && fs != UVHTTP_WS_FRAME_ERR_DEVICE;
        if (judged) {
            const uint32_t ff = r.first_frame;
            uint32_t nd = r.n_delivered;
            if (ff >= max_frames) nd = 0;
            else if (nd > max_frames - ff) nd = max_frames - ff;
            uint32_t c = none;
            for (uint32_t i = 0; i < nd && c == none; ++i)
                if (desc[ff + i].opcode == UVHTTP_WS_OPCODE_CLOSE && desc[ff + i].status == UVHTTP_WS_FRAME_OK)
                    c = ff + i;
            uint32_t k = none, reason = UVHTTP_WS_FAIL_NONE;
            int bad = 0;
            if ((flags & UVHTTP_WS_FAIL_CHECK_CLOSE) && c != none) {
                const uint64_t len = desc[c].payload_len, off = desc[c].payload_off;
                if (len == 1) {
                    reason = UVHTTP_WS_FAIL_CLOSE_LEN;
                } else if (len >= 2) {
                    if (len > wire_len || off > wire_len - len) bad = 1;
                    else if (!fail_code_valid((uint32_t)wire[off] << 8 | wire[off + 1]))
                        reason = UVHTTP_WS_FAIL_CLOSE_CODE;
                }
                if (reason != UVHTTP_WS_FAIL_NONE) k = c;
            }
            if (bad) {
                f.status = UVHTTP_WS_FAIL_BAD_RANGE;
                ++sum.n_bad_range;
            } else {
                const uint32_t u = v.first_invalid;
                const int close_cut = k != none;
                if (verdict != NULL && v.status == UVHTTP_WS_UTF8_INVALID && u >= ff && u - ff < nd &&
                    (c == none || u <= c) && (k == none || u < k)) {
                    k = u;
                    reason = UVHTTP_WS_FAIL_UTF8;
                }
                if (k != none) {
                    f.frame = k;
                    f.n_dropped = nd - (k - ff);
                    f.code = reason == UVHTTP_WS_FAIL_UTF8 ? 1007 : 1002;
                    r.n_delivered = k - ff;
                    r.n_frames = r.n_delivered + 1;
                    r.status = UVHTTP_ERROR_INVALID_PARAM;
                    r.first_status = reason == UVHTTP_WS_FAIL_UTF8 ? UVHTTP_WS_FRAME_ERR_UTF8 : UVHTTP_WS_FRAME_ERR_CLOSE;
                } else if (fs < 0) {
                    reason = UVHTTP_WS_FAIL_DECODE;
                    f.frame = r.first_frame + r.n_delivered;
                    f.code = 1002;
                }
                f.reason = (uint8_t)reason;
                /* the verdict over the kept frames */
                if (verdict != NULL && u != none && c != none && (u > c || (close_cut && u == c))) {
                    v.status = UVHTTP_WS_UTF8_VALID;
                    v.first_invalid = none;
                    memset(&v.state, 0, sizeof(v.state));
                }
                sum.n_dropped += f.n_dropped;
                sum.n_decode += reason == UVHTTP_WS_FAIL_DECODE;
                sum.n_utf8 += reason == UVHTTP_WS_FAIL_UTF8;
                sum.n_close_len += reason == UVHTTP_WS_FAIL_CLOSE_LEN;
                sum.n_close_code += reason == UVHTTP_WS_FAIL_CLOSE_CODE;
                if (reason != UVHTTP_WS_FAIL_NONE && sum.first_failed == none) sum.first_failed = s;
            }
        }
        results_out[s] = r;
        if (verdict_out != NULL) verdict_out[s] = v;
        fail[s] = f;
    }
    *summary = sum;
    return 0;
}
