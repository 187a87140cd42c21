/* uvhttp_ws_close_frames (ws_host.c) under ASan/UBSan: seeded mixes of every input, every output
 * in a heap block of exactly its size (so a byte past any of them is reported), checked against
 * the layout rules: the frames tile [0, out_bytes), every frame is a CLOSE of its connection's
 * code, runs count the closes before, a 1007 close empties the named runs and nothing else.
 * Usage: close_check [rounds] [seed]; prints "ok <rounds> <closes>" and exits 0. */
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

#define CHECK(c)                                                              \
    do {                                                                      \
        if (!(c)) {                                                           \
            fprintf(stderr, "close_check: %s failed (line %d)\n", #c, __LINE__); \
            exit(1);                                                          \
        }                                                                     \
    } while (0)

static const int32_t kStatus[] = {0, 0, 0, 1, 2, -1, -2, -3, -4, -5, -6, -7, -8, -9, -10, -11};

int main(int argc, char** argv) {
    const int rounds = argc > 1 ? atoi(argv[1]) : 200;
    rng_state = argc > 2 ? strtoull(argv[2], NULL, 0) : 1;
    uint64_t closes = 0;
    for (int round = 0; round < rounds; ++round) {
        const uint32_t n = rnd() % 70;
        const size_t m = n ? n : 1;
        uvhttp_ws_stream_t* st = calloc(m, sizeof(*st));
        uvhttp_ws_stream_result_t* res = calloc(m, sizeof(*res));
        uvhttp_ws_utf8_conn_verdict_t* ver = calloc(m, sizeof(*ver));
        uvhttp_ws_reply_conn_t* rep = calloc(m, sizeof(*rep));
        uint8_t* en = calloc(m, 1);
        uint32_t* keys = calloc(m, 4);
        CHECK(st && res && ver && rep && en && keys);
        for (uint32_t s = 0; s < n; ++s) {
            st[s].is_server = rnd() % 3 != 0;
            res[s].first_status = kStatus[rnd() % (sizeof(kStatus) / sizeof(kStatus[0]))];
            ver[s].status = (uint8_t)(rnd() % 5);
            rep[s].closed = rnd() % 7 == 0;
            en[s] = rnd() % 8 != 0;
            keys[s] = rnd() ^ (rnd() << 16);
        }
        const int with_ver = rnd() % 4 != 0, with_rep = rnd() % 4 != 0, with_en = rnd() % 4 != 0;
        const int with_keys = rnd() % 4 != 0, with_runs = rnd() % 4 != 0;
        const uint32_t stride = 8 + 4 * (rnd() % 7), n_clear = rnd() % 5;
        uint32_t cstride[4];
        uint32_t* ctab[4];
        for (uint32_t k = 0; k < n_clear; ++k) {
            cstride[k] = 8 + 4 * (rnd() % 7);
            ctab[k] = malloc(m * cstride[k]);
            CHECK(ctab[k]);
            memset(ctab[k], 0x5A, m * cstride[k]);
        }
        uint32_t* runs = malloc(m * stride);
        uint64_t* off = malloc(((size_t)n + 1) * 8);
        uvhttp_ws_close_conn_t* conn = malloc(m * sizeof(*conn));
        CHECK(runs && off && conn);
        memset(runs, 0x5A, m * stride);
        /* first with no room at all, to learn the size; then with exactly that */
        uvhttp_ws_close_summary_t need, sum;
        CHECK(uvhttp_ws_close_frames(st, res, n, with_ver ? ver : NULL, with_rep ? rep : NULL,
                                     with_en ? en : NULL, with_keys ? keys : NULL, 0, NULL, 0, off,
                                     with_runs ? runs : NULL, stride, ctab, cstride, n_clear, conn, &need) == 0);
        CHECK(need.status == (need.out_bytes ? UVHTTP_WS_CLOSE_ERR_CAPACITY : UVHTTP_WS_CLOSE_OK));
        if (need.out_bytes) {
            for (uint32_t k = 0; k < n_clear; ++k)  /* nothing is cleared on capacity */
                for (size_t b = 0; b < m * cstride[k]; ++b) CHECK(((uint8_t*)ctab[k])[b] == 0x5A);
            for (uint32_t s = 0; s < n; ++s) CHECK(conn[s].status == UVHTTP_WS_CLOSE_ERR_CAPACITY && off[s] == 0);
        }
        uint8_t* out = malloc(need.out_bytes ? need.out_bytes : 1);
        CHECK(out);
        CHECK(uvhttp_ws_close_frames(st, res, n, with_ver ? ver : NULL, with_rep ? rep : NULL,
                                     with_en ? en : NULL, with_keys ? keys : NULL, 0, out, need.out_bytes, off,
                                     with_runs ? runs : NULL, stride, ctab, cstride, n_clear, conn, &sum) == 0);
        CHECK(sum.status == UVHTTP_WS_CLOSE_OK && sum.out_bytes == need.out_bytes);
        CHECK(sum.n_closes == need.n_closes && sum.n_closes == sum.n_1002 + sum.n_1007);
        uint64_t at = 0;
        uint32_t j = 0, n1002 = 0, n1007 = 0;
        for (uint32_t s = 0; s < n; ++s) {
            const uvhttp_ws_close_conn_t* c = &conn[s];
            const uint32_t* run = (const uint32_t*)((const char*)runs + (size_t)s * stride);
            if (with_runs) CHECK(run[0] == j && run[1] == (c->code ? 1u : 0u));
            for (uint32_t k = 0; k < n_clear; ++k) {
                const uint32_t* cr = (const uint32_t*)((const char*)ctab[k] + (size_t)s * cstride[k]);
                CHECK(cr[0] == 0x5A5A5A5Au && cr[1] == (c->code == 1007 ? 0u : 0x5A5A5A5Au));
            }
            if (!c->code) {
                CHECK(c->out_len == 0);
                continue;
            }
            CHECK(c->code == 1002 || c->code == 1007);
            CHECK(c->status == UVHTTP_WS_CLOSE_OK && off[j] == at);
            const int masked = !st[s].is_server;
            const uint32_t plen = c->code == 1002 ? 16 : 2, hdr = masked ? 6 : 2;
            CHECK(c->out_len == hdr + plen);
            const uint8_t* f = out + at;
            CHECK(f[0] == 0x88 && f[1] == ((masked ? 0x80 : 0) | plen));
            uint8_t key[4] = {0, 0, 0, 0};
            if (masked)
                for (int b = 0; b < 4; ++b) CHECK((key[b] = f[2 + b]) == (uint8_t)(keys[s] >> (8 * b)));
            uint8_t plain[16];
            for (uint32_t b = 0; b < plen; ++b) plain[b] = f[hdr + b] ^ key[b & 3];
            CHECK(((uint32_t)plain[0] << 8 | plain[1]) == c->code);
            if (plen > 2) CHECK(memcmp(plain + 2, "protocol error", 14) == 0);
            n1002 += c->code == 1002;
            n1007 += c->code == 1007;
            at += c->out_len;
            ++j;
        }
        for (uint32_t k = j; k <= n; ++k) CHECK(off[k] == at);
        CHECK(at == sum.out_bytes && n1002 == sum.n_1002 && n1007 == sum.n_1007);
        closes += j;
        for (uint32_t k = 0; k < n_clear; ++k) free(ctab[k]);
        free(out), free(conn), free(off), free(runs);
        free(keys), free(en), free(rep), free(ver), free(res), free(st);
    }
    printf("ok %d %llu\n", rounds, (unsigned long long)closes);
    return 0;
}
