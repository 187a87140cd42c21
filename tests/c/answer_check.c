/* uvhttp_ws_answer_messages (ws_host.c) under ASan/UBSan: seeded descriptor tables of data and
 * control frames over a wire of random bytes, servers and clients, both flags, a carried-in
 * message; every output in a heap block of exactly its size (so a byte past any of them is
 * reported).  The call is made with no room first, to learn the sizes, then with exactly those,
 * and the frames are parsed back: they tile [0, out_len), their order is the descriptors' (a PONG
 * where the PING stood, the echo where the FIN frame stood, the CLOSE echo where the CLOSE
 * stood), every payload unmasks to its source bytes, and the open message is the carry and the
 * fragments so far.
 * Usage: answer_check [rounds] [seed]; prints "answer_check: ok <rounds> <answers>" and exits 0. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "uvhttp_ws_amd.h"

static uint64_t rng_state;
static uint32_t rnd(void) {
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(rng_state >> 33);
}

#define CHECK(c)                                                               \
    do {                                                                       \
        if (!(c)) {                                                            \
            fprintf(stderr, "answer_check: %s failed (line %d)\n", #c, __LINE__); \
            exit(1);                                                           \
        }                                                                      \
    } while (0)

static const uint32_t kLens[] = {0, 0, 1, 2, 5, 124, 125, 126, 300, 65535, 65536};

/* one expected answer: its opcode and its payload, gathered by the checker's own walk */
typedef struct {
    uint8_t op;
    uint64_t len;
    uint8_t* bytes;
} want_t;

int main(int argc, char** argv) {
    const int rounds = argc > 1 ? atoi(argv[1]) : 150;
    rng_state = argc > 2 ? strtoull(argv[2], NULL, 0) : 1;
    uint64_t answers = 0;
    for (int round = 0; round < rounds; ++round) {
        const uint32_t n = rnd() % 24;
        const uint32_t flags = rnd() % 4;
        const int is_server = rnd() % 3 != 0;
        const uint64_t carry_len = rnd() % 3 == 0 ? 1 + rnd() % 200 : 0;
        const int pend_op = carry_len ? 1 + (int)(rnd() % 2) : 0;
        uvhttp_ws_frame_desc_t* desc = calloc(n ? n : 1, sizeof(*desc));
        uint8_t* carry = malloc(carry_len ? carry_len : 1);
        CHECK(desc && carry);
        for (uint64_t b = 0; b < carry_len; ++b) carry[b] = (uint8_t)rnd();
        /* frames back to back in the wire, payloads unmasked as a decode leaves them */
        uint64_t wire_len = 0;
        int open_msg = carry_len != 0;
        for (uint32_t i = 0; i < n; ++i) {
            uvhttp_ws_frame_desc_t* d = &desc[i];
            const uint32_t r = rnd() % 10;
            if (r < 3) { /* PING, PONG or CLOSE */
                d->opcode = r == 0 ? UVHTTP_WS_OPCODE_CLOSE : r == 1 ? UVHTTP_WS_OPCODE_PONG : UVHTTP_WS_OPCODE_PING;
                d->payload_len = kLens[rnd() % 7];
                d->flags = UVHTTP_WS_FLAG_FIN;
            } else {
                const int fin = rnd() % 2;
                d->opcode = open_msg ? UVHTTP_WS_OPCODE_CONTINUATION : (uint8_t)(1 + rnd() % 2);
                d->payload_len = kLens[rnd() % (sizeof(kLens) / sizeof(kLens[0]))];
                if (!open_msg && !fin && d->payload_len == 0) d->payload_len = 1;
                d->flags = fin ? UVHTTP_WS_FLAG_FIN : 0;
                open_msg = !fin;
            }
            d->status = rnd() % 40 == 0 ? UVHTTP_WS_FRAME_SKIPPED : UVHTTP_WS_FRAME_OK;
            d->header_size = 6;
            d->payload_off = wire_len + d->header_size;
            wire_len = d->payload_off + d->payload_len;
        }
        uint8_t* wire = malloc(wire_len ? wire_len : 1);
        CHECK(wire);
        for (uint64_t b = 0; b < wire_len; ++b) wire[b] = (uint8_t)rnd();

        /* the checker's own walk: what is answered, in descriptor order */
        want_t* want = calloc(n ? n : 1, sizeof(*want));
        uint8_t* acc = malloc(carry_len + wire_len + 1);
        CHECK(want && acc);
        uint32_t nw = 0, nrep = 0;
        int closed = 0, cur = carry_len != 0, cur_op = pend_op;
        uint64_t acc_len = carry_len;
        memcpy(acc, carry, carry_len);
        for (uint32_t i = 0; i < n; ++i) {
            const uvhttp_ws_frame_desc_t* d = &desc[i];
            if (d->status != UVHTTP_WS_FRAME_OK) continue;
            if (d->opcode == UVHTTP_WS_OPCODE_PING || d->opcode == UVHTTP_WS_OPCODE_CLOSE) {
                const int after = closed;
                if (d->opcode == UVHTTP_WS_OPCODE_CLOSE) closed = 1;
                if (after && !(flags & UVHTTP_WS_ANSWER_REPLY_AFTER_CLOSE)) continue;
                want_t* w = &want[nw++];
                w->op = d->opcode == UVHTTP_WS_OPCODE_PING ? UVHTTP_WS_OPCODE_PONG : UVHTTP_WS_OPCODE_CLOSE;
                w->len = d->opcode == UVHTTP_WS_OPCODE_CLOSE && d->payload_len < 2 ? 0 : d->payload_len;
                w->bytes = malloc(w->len ? w->len : 1);
                CHECK(w->bytes);
                memcpy(w->bytes, wire + d->payload_off, w->len);
                ++nrep;
            } else if (d->opcode <= UVHTTP_WS_OPCODE_BINARY) {
                if (d->opcode != UVHTTP_WS_OPCODE_CONTINUATION) {
                    cur = 1;
                    cur_op = d->opcode;
                    acc_len = 0;
                } else if (!cur) {
                    continue;
                }
                memcpy(acc + acc_len, wire + d->payload_off, d->payload_len);
                acc_len += d->payload_len;
                if (!(d->flags & UVHTTP_WS_FLAG_FIN)) continue;
                cur = 0;
                if (closed || ((flags & UVHTTP_WS_ANSWER_SERVER_SEND) && acc_len == 0)) continue;
                want_t* w = &want[nw++];
                w->op = (flags & UVHTTP_WS_ANSWER_SERVER_SEND) ? UVHTTP_WS_OPCODE_TEXT : (uint8_t)cur_op;
                w->len = acc_len;
                w->bytes = malloc(acc_len ? acc_len : 1);
                CHECK(w->bytes);
                memcpy(w->bytes, acc, acc_len);
            }
        }
        const uint64_t open_want = cur ? acc_len : 0;

        uint32_t* keys = malloc(((size_t)nw + 1) * 4);
        CHECK(keys);
        for (uint32_t j = 0; j <= nw; ++j) keys[j] = rnd() ^ (rnd() << 16);
        uvhttp_ws_answer_conn_t need, res;
        uvhttp_ws_reply_conn_t rep;
        uint64_t* off0 = malloc(8);
        CHECK(off0);
        /* no room at all: the sizes */
        CHECK(uvhttp_ws_answer_messages(wire, wire_len, desc, 0, n, is_server, 1, keys, flags, pend_op, carry_len,
                                        carry, carry_len, NULL, 0, off0, 0, acc, 0, &need, &rep) == 0);
        CHECK(need.n_answers == nw && need.n_replies == nrep && need.open_len == open_want);
        CHECK(need.closed == closed && rep.closed == closed);
        const int fits0 = nw == 0 && open_want == 0;
        CHECK(need.status == (fits0 ? UVHTTP_WS_ECHO_OK : UVHTTP_WS_ECHO_ERR_CAPACITY) && off0[0] == 0);
        free(off0);
        /* exactly the sizes reported */
        uint8_t* out = malloc(need.out_len ? need.out_len : 1);
        uint8_t* opn = malloc(need.open_len ? need.open_len : 1);
        uint64_t* off = malloc(((size_t)nw + 1) * 8);
        CHECK(out && opn && off);
        CHECK(uvhttp_ws_answer_messages(wire, wire_len, desc, 0, n, is_server, 1, keys, flags, pend_op, carry_len,
                                        carry, carry_len, out, need.out_len, off, nw, opn, need.open_len, &res,
                                        rnd() % 4 ? &rep : NULL) == 0);
        CHECK(res.status == UVHTTP_WS_ECHO_OK && res.n_answers == nw && res.out_len == need.out_len);
        CHECK(res.n_replies == nrep && res.open_len == open_want && res.first_answer == 0);
        CHECK(res.open_opcode == (open_want ? cur_op : 0));
        CHECK(open_want == 0 || memcmp(opn, acc, open_want) == 0);
        uint64_t at = 0;
        const int masked = !is_server;
        for (uint32_t j = 0; j < nw; ++j) {
            const want_t* w = &want[j];
            CHECK(off[j] == at);
            const uint8_t* f = out + at;
            uint64_t h = 2, len = f[1] & 0x7F;
            CHECK(f[0] == (0x80 | w->op) && (f[1] >> 7) == masked);
            if (len == 126) {
                len = (uint64_t)f[2] << 8 | f[3];
                h = 4;
            } else if (len == 127) {
                len = 0;
                for (int b = 0; b < 8; ++b) len = len << 8 | f[2 + b];
                h = 10;
            }
            CHECK(len == w->len && h == (len <= 125 ? 2u : len <= 65535 ? 4u : 10u));
            uint8_t key[4] = {0, 0, 0, 0};
            if (masked)
                for (int b = 0; b < 4; ++b) CHECK((key[b] = f[h + b]) == (uint8_t)(keys[j] >> (8 * b)));
            h += masked ? 4 : 0;
            for (uint64_t b = 0; b < len; ++b) CHECK((uint8_t)(f[h + b] ^ key[b & 3]) == w->bytes[b]);
            at += h + len;
        }
        CHECK(off[nw] == at && at == res.out_len);
        answers += nw;
        for (uint32_t j = 0; j < nw; ++j) free(want[j].bytes);
        free(off), free(opn), free(out), free(keys), free(acc), free(want), free(wire), free(carry), free(desc);
    }
    printf("answer_check: ok %d %llu\n", rounds, (unsigned long long)answers);
    return 0;
}
