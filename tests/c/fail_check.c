/* uvhttp_ws_fail_points (ws_host.c) under ASan/UBSan: seeded mixes of every input, the wire and
 * every table in a heap block of exactly its size (so a byte read or written past any of them is
 * reported), checked against the rule's invariants: a cut lies inside the considered range and
 * names a frame that can fail (a CLOSE for the CLOSE reasons, the verdict's first_invalid for
 * UTF8), the rewritten result stops there, connections that are not judged and BAD_RANGE ones are
 * copied byte for byte, the summary is the sum of the entries, and a second call in place gives
 * the same bytes.
 * Usage: fail_check [rounds] [seed]; prints "ok <rounds> <failed connections>" and exits 0. */
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

#define CHECK(c)                                                             \
    do {                                                                     \
        if (!(c)) {                                                          \
            fprintf(stderr, "fail_check: %s failed (line %d)\n", #c, __LINE__); \
            exit(1);                                                         \
        }                                                                    \
    } while (0)

#define NONE 0xFFFFFFFFu

static const int32_t kStatus[] = {0, 0, 0, 0, 0, 1, -1, -2, -7, -9, -10, -11};
static const uint8_t kOpcode[] = {0, 1, 1, 2, 8, 8, 9, 10};
static const uint16_t kCode[] = {999, 1000, 1003, 1004, 1006, 1007, 1014, 1015, 1016, 2999, 3000, 4999, 5000, 65535};
static const uint64_t kCloseLen[] = {0, 1, 2, 2, 2, 5, 125};

int main(int argc, char** argv) {
    const int rounds = argc > 1 ? atoi(argv[1]) : 200;
    rng_state = argc > 2 ? strtoull(argv[2], NULL, 0) : 1;
    uint64_t failed = 0;
    for (int round = 0; round < rounds; ++round) {
        const uint32_t n = rnd() % 40;
        const size_t m = n ? n : 1;
        uvhttp_ws_stream_result_t* res = calloc(m, sizeof(*res));
        uvhttp_ws_utf8_conn_verdict_t* ver = calloc(m, sizeof(*ver));
        uint8_t* en = calloc(m, 1);
        CHECK(res && ver && en);
        uint32_t total = 0;
        for (uint32_t s = 0; s < n; ++s) {
            res[s].first_frame = total;
            res[s].n_delivered = rnd() % 7;
            res[s].n_frames = res[s].n_delivered;
            res[s].first_status = kStatus[rnd() % (sizeof(kStatus) / sizeof(kStatus[0]))];
            res[s].status = res[s].first_status < 0 ? -1 : 0;
            res[s].consumed_bytes = rnd();
            res[s].pending_bytes = rnd() % 3;
            total += res[s].n_delivered + (rnd() % 4 == 0);  /* (descriptors nobody considers in between) */
            en[s] = rnd() % 8 != 0;
        }
        /* sometimes fewer descriptors than the results name: the clip */
        const uint32_t max_frames = rnd() % 5 == 0 && total ? total - 1 - rnd() % (total < 3 ? total : 3) : total;
        const uint64_t wire_len = 2 * (uint64_t)total + rnd() % 3;
        uint8_t* wire = malloc(wire_len ? wire_len : 1);
        uvhttp_ws_frame_desc_t* desc = calloc(max_frames ? max_frames : 1, sizeof(*desc));
        CHECK(wire && desc);
        for (uint32_t f = 0; f < max_frames; ++f) {
            desc[f].opcode = kOpcode[rnd() % sizeof(kOpcode)];
            desc[f].status = rnd() % 16 == 0 ? 2 : 0;
            desc[f].payload_len = desc[f].opcode == 8 ? kCloseLen[rnd() % 7] : rnd() % 100;
            /* every frame owns wire[2f, 2f + 2): enough for a CLOSE's code; a longer CLOSE near the
             * end, and one time in twelve any CLOSE, lies outside the wire */
            desc[f].payload_off = rnd() % 12 == 0 ? wire_len - (rnd() % 2) : 2 * (uint64_t)f;
            const uint16_t code = rnd() % 3 ? kCode[rnd() % 14] : (uint16_t)(1000 + rnd() % 16);
            wire[2 * f] = (uint8_t)(code >> 8);
            wire[2 * f + 1] = (uint8_t)code;
        }
        for (uint32_t s = 0; s < n; ++s) {
            ver[s].status = (uint8_t)(rnd() % 5);
            ver[s].n_text_frames = rnd() % 9;
            ver[s].first_invalid = NONE;
            if (ver[s].status == UVHTTP_WS_UTF8_INVALID || ver[s].status == UVHTTP_WS_UTF8_BAD_RANGE)
                ver[s].first_invalid = res[s].first_frame + rnd() % (res[s].n_delivered + 1 + (rnd() % 5 == 0));
            if (ver[s].status == UVHTTP_WS_UTF8_PREFIX) ver[s].state.n = 1, ver[s].state.pend[0] = 0xC3;
        }
        const int with_ver = rnd() % 4 != 0, with_en = rnd() % 3 != 0;
        const uint32_t flags = rnd() % 4 != 0 ? UVHTTP_WS_FAIL_CHECK_CLOSE : 0;
        uvhttp_ws_stream_result_t* ro = malloc(m * sizeof(*ro));
        uvhttp_ws_utf8_conn_verdict_t* vo = malloc(m * sizeof(*vo));
        uvhttp_ws_fail_conn_t* fl = malloc(m * sizeof(*fl));
        uvhttp_ws_fail_summary_t* sum = malloc(sizeof(*sum));
        CHECK(ro && vo && fl && sum);
        CHECK(uvhttp_ws_fail_points(wire_len ? wire : NULL, wire_len, desc, max_frames, res, n, with_ver ? ver : NULL,
                                    with_en ? en : NULL, flags, ro, with_ver ? vo : NULL, fl, sum) == 0);
        uvhttp_ws_fail_summary_t want;
        memset(&want, 0, sizeof(want));
        want.first_failed = NONE;
        for (uint32_t s = 0; s < n; ++s) {
            const uvhttp_ws_fail_conn_t* f = &fl[s];
            const uint32_t ff = res[s].first_frame;
            uint32_t nd = res[s].n_delivered;
            if (ff >= max_frames) nd = 0;
            else if (nd > max_frames - ff) nd = max_frames - ff;
            const int32_t fs = res[s].first_status;
            const int judged = (!with_en || en[s]) && fs != -9 && fs != -10 && fs != -11;
            CHECK(f->reserved == 0 && f->reason <= UVHTTP_WS_FAIL_CLOSE_CODE);
            CHECK(f->status == UVHTTP_WS_FAIL_OK || f->status == UVHTTP_WS_FAIL_BAD_RANGE);
            const int cut = f->reason >= UVHTTP_WS_FAIL_UTF8;
            if (!judged || f->status == UVHTTP_WS_FAIL_BAD_RANGE) CHECK(f->reason == UVHTTP_WS_FAIL_NONE);
            if (f->status == UVHTTP_WS_FAIL_BAD_RANGE) CHECK(judged && (flags & UVHTTP_WS_FAIL_CHECK_CLOSE));
            if (f->reason == UVHTTP_WS_FAIL_NONE) {
                CHECK(f->frame == NONE && f->code == 0 && f->n_dropped == 0);
                CHECK(f->status == UVHTTP_WS_FAIL_BAD_RANGE || !judged || fs >= 0);
            }
            if (!cut) CHECK(memcmp(&ro[s], &res[s], sizeof(res[s])) == 0);
            if ((!judged || f->status == UVHTTP_WS_FAIL_BAD_RANGE) && with_ver)
                CHECK(memcmp(&vo[s], &ver[s], sizeof(ver[s])) == 0);
            if (f->reason == UVHTTP_WS_FAIL_DECODE)
                CHECK(fs < 0 && f->code == 1002 && f->frame == ff + res[s].n_delivered && f->n_dropped == 0);
            if (cut) {
                CHECK(f->frame >= ff && f->frame - ff < nd && f->n_dropped == nd - (f->frame - ff));
                for (uint32_t i = ff; i < f->frame; ++i)  /* no CLOSE before the cut */
                    CHECK(!(desc[i].opcode == 8 && desc[i].status == 0));
                uvhttp_ws_stream_result_t w = res[s];
                w.n_delivered = f->frame - ff;
                w.n_frames = w.n_delivered + 1;
                w.status = UVHTTP_ERROR_INVALID_PARAM;
                w.first_status = f->reason == UVHTTP_WS_FAIL_UTF8 ? UVHTTP_WS_FRAME_ERR_UTF8 : UVHTTP_WS_FRAME_ERR_CLOSE;
                CHECK(memcmp(&ro[s], &w, sizeof(w)) == 0);
                if (f->reason == UVHTTP_WS_FAIL_UTF8) {
                    CHECK(with_ver && f->code == 1007 && ver[s].status == UVHTTP_WS_UTF8_INVALID);
                    CHECK(ver[s].first_invalid == f->frame && memcmp(&vo[s], &ver[s], sizeof(ver[s])) == 0);
                } else {
                    const uvhttp_ws_frame_desc_t* d = &desc[f->frame];
                    CHECK((flags & UVHTTP_WS_FAIL_CHECK_CLOSE) && f->code == 1002 && d->opcode == 8 && d->status == 0);
                    CHECK(f->reason == UVHTTP_WS_FAIL_CLOSE_LEN ? d->payload_len == 1 : d->payload_len >= 2);
                    if (with_ver) CHECK(vo[s].status != UVHTTP_WS_UTF8_INVALID || vo[s].first_invalid < f->frame);
                }
            }
            if (with_ver && memcmp(&vo[s], &ver[s], sizeof(ver[s])) != 0) {  /* the only rewrite there is */
                CHECK(vo[s].status == UVHTTP_WS_UTF8_VALID && vo[s].first_invalid == NONE && vo[s].state.n == 0);
                CHECK(vo[s].n_text_frames == ver[s].n_text_frames && ver[s].first_invalid != NONE);
            }
            want.n_dropped += f->n_dropped;
            want.n_decode += f->reason == UVHTTP_WS_FAIL_DECODE;
            want.n_utf8 += f->reason == UVHTTP_WS_FAIL_UTF8;
            want.n_close_len += f->reason == UVHTTP_WS_FAIL_CLOSE_LEN;
            want.n_close_code += f->reason == UVHTTP_WS_FAIL_CLOSE_CODE;
            want.n_bad_range += f->status == UVHTTP_WS_FAIL_BAD_RANGE;
            if (f->reason != UVHTTP_WS_FAIL_NONE && want.first_failed == NONE) want.first_failed = s;
            failed += f->reason != UVHTTP_WS_FAIL_NONE;
        }
        CHECK(memcmp(sum, &want, sizeof(want)) == 0);
        /* in place: the same bytes */
        uvhttp_ws_stream_result_t* r2 = malloc(m * sizeof(*r2));
        uvhttp_ws_utf8_conn_verdict_t* v2 = malloc(m * sizeof(*v2));
        uvhttp_ws_fail_conn_t* f2 = malloc(m * sizeof(*f2));
        CHECK(r2 && v2 && f2);
        memcpy(r2, res, m * sizeof(*r2));
        memcpy(v2, ver, m * sizeof(*v2));
        CHECK(uvhttp_ws_fail_points(wire_len ? wire : NULL, wire_len, desc, max_frames, r2, n, with_ver ? v2 : NULL,
                                    with_en ? en : NULL, flags, r2, with_ver ? v2 : NULL, f2, sum) == 0);
        CHECK(memcmp(sum, &want, sizeof(want)) == 0);
        if (n) {
            CHECK(memcmp(r2, ro, n * sizeof(*r2)) == 0 && memcmp(f2, fl, n * sizeof(*f2)) == 0);
            if (with_ver) CHECK(memcmp(v2, vo, n * sizeof(*v2)) == 0);
        }
        free(f2), free(v2), free(r2), free(sum), free(fl), free(vo), free(ro);
        free(desc), free(wire), free(en), free(ver), free(res);
    }
    printf("ok %d %llu\n", rounds, (unsigned long long)failed);
    return 0;
}
