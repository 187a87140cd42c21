/* The UTF-8 rules (RFC 3629) as the host check (ws_host.c) and the device kernels
 * (utf8_gpu.hip) both apply them: a byte is judged from itself and the three bytes before it
 * in the same message (0 where the message has not that many), so the check is local and
 * fail-fast — a byte is bad as soon as no continuation could make the sequence valid.
 *
 *   1. b is a continuation byte (80..BF) exactly when one is due:
 *      p1 >= C0 (any lead), p2 >= E0 (3- or 4-byte lead), p3 >= F0 (4-byte lead);
 *   2. b is none of C0, C1 (overlong 2-byte), F5..FF (above U+10FFFF);
 *   3. the second byte's range: after E0 >= A0 (overlong), after ED <= 9F (surrogates),
 *      after F0 >= 90 (overlong), after F4 <= 8F (above U+10FFFF).
 *
 * A complete message must also not end inside a sequence: with e1, e2, e3 its last three bytes
 * (e1 the last), e1 < C0, e2 < E0 and e3 < F0.  Plain C, no tables. */
#ifndef UVHTTP_WS_UTF8_RULES_H
#define UVHTTP_WS_UTF8_RULES_H

#include <stdint.h>

#if defined(__HIPCC__)
#define UVWS_HD __host__ __device__ static inline
#else
#define UVWS_HD static inline
#endif

/* one byte: non-zero if b breaks a rule given the three bytes before it */
UVWS_HD uint32_t uvws_utf8_bad(uint32_t b, uint32_t p1, uint32_t p2, uint32_t p3) {
    const uint32_t need = (p1 >= 0xC0u) | (p2 >= 0xE0u) | (p3 >= 0xF0u);
    const uint32_t cont = (b & 0xC0u) == 0x80u;
    uint32_t bad = need ^ cont;
    bad |= ((b & 0xFEu) == 0xC0u) | (b >= 0xF5u);
    bad |= ((p1 == 0xE0u) & (b < 0xA0u)) | ((p1 == 0xEDu) & (b > 0x9Fu)) |
           ((p1 == 0xF0u) & (b < 0x90u)) | ((p1 == 0xF4u) & (b > 0x8Fu));
    return bad;
}

/* bytes (0..3) of the sequence still open after ..., p3, p2, p1 */
UVWS_HD uint32_t uvws_utf8_open(uint32_t p1, uint32_t p2, uint32_t p3) {
    return p1 >= 0xC0u ? 1u : p2 >= 0xE0u ? 2u : p3 >= 0xF0u ? 3u : 0u;
}

/* (hi:lo) >> 8n, the low word: bytes n..n+3 of the eight (v_alignbyte_b32 on the device) */
UVWS_HD uint32_t uvws_alignbyte(uint32_t hi, uint32_t lo, uint32_t n) {
    return (uint32_t)((((uint64_t)hi << 32) | lo) >> (8u * n));
}

/* Four bytes at once.  Per-byte flags of a little-endian word, each in bit 7 of its byte (the
 * other bits are don't-care until the final mask): a left shift by k <= 7 brings bit 7-k of
 * the same byte there, so byte tests become ANDs / ORs of shifted copies. */
typedef struct {
    uint32_t c0, e0, f0; /* byte >= C0, >= E0, >= F0 */
    uint32_t a5s;        /* E0: the next byte needs bit 5 set (>= A0) */
    uint32_t a54;        /* F0: the next byte needs bit 5 or 4 set (>= 90) */
    uint32_t a5c;        /* ED, F4: the next byte needs bit 5 clear (<= 9F) */
    uint32_t a4c;        /* F4: ... and bit 4 clear (<= 8F) */
} uvws_utf8_flags_t;

UVWS_HD uvws_utf8_flags_t uvws_utf8_flags(uint32_t w) {
    uvws_utf8_flags_t f;
    f.c0 = w & (w << 1);
    f.e0 = f.c0 & (w << 2);
    f.f0 = f.e0 & (w << 3);
    const uint32_t nib0 = ~((w << 4) | (w << 5) | (w << 6) | (w << 7)); /* low nibble == 0 */
    const uint32_t e_only = f.e0 & ~f.f0;                              /* E0..EF */
    f.a5s = e_only & nib0;
    f.a54 = f.f0 & nib0;
    f.a4c = f.f0 & (w << 5) & ~((w << 4) | (w << 6) | (w << 7));          /* x4 = 0100 */
    f.a5c = (e_only & (w << 4) & (w << 5) & ~(w << 6) & (w << 7)) | f.a4c; /* xD = 1101 */
    return f;
}

/* Non-zero if any of the four bytes of w breaks a rule; `p` are the flags of the word before
 * (the four bytes preceding w in the same message), `f` = uvws_utf8_flags(w). */
UVWS_HD uint32_t uvws_utf8_bad4(uint32_t w, uvws_utf8_flags_t f, uvws_utf8_flags_t p) {
    const uint32_t need = uvws_alignbyte(f.c0, p.c0, 3) | uvws_alignbyte(f.e0, p.e0, 2) |
                          uvws_alignbyte(f.f0, p.f0, 1);
    const uint32_t cont = w ^ f.c0; /* bit 7 set, bit 6 clear */
    uint32_t bad = need ^ cont;
    bad |= f.c0 & ~((w << 2) | (w << 3) | (w << 4) | (w << 5) | (w << 6));  /* C0, C1 */
    bad |= f.f0 & ((w << 4) | ((w << 5) & ((w << 6) | (w << 7))));          /* F5..FF */
    bad |= uvws_alignbyte(f.a5s, p.a5s, 3) & ~(w << 2);
    bad |= uvws_alignbyte(f.a54, p.a54, 3) & ~((w << 2) | (w << 3));
    bad |= uvws_alignbyte(f.a5c, p.a5c, 3) & (w << 2);
    bad |= uvws_alignbyte(f.a4c, p.a4c, 3) & (w << 3);
    return bad & 0x80808080u;
}

#endif
