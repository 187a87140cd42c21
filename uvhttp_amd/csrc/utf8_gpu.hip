// utf8_gpu.hip — UTF-8 validation of TEXT messages on the device (RFC 6455 §5.6, §8.1;
// include/uvhttp_ws_amd.h: uvhttp_ws_gpu_validate_utf8).
//
// Input: the message arena a compact decode left in HBM (every message one contiguous range)
// and its message table, or a caller's own table of ascending, non-overlapping ranges.  Three
// launches, no scratch, no waiting between workgroups:
//
//   k_utf8_init    one lane per table entry: NOT_TEXT / BAD_RANGE / VALID, and the summary zeroed
//   k_utf8_tiles   position-indexed over the arena: every lane reads 16-byte vectors once
//                  (non-temporal), takes the 4 bytes before each from the lane below, and applies
//                  the rules of utf8_rules.h — each byte is judged from itself and the 3 bytes
//                  before it.  A wave whose 4 KiB are all ASCII leaves right after its loads
//                  (nothing in it can break a rule, wherever the message boundaries fall).
//                  Otherwise the wave finds its place in the table (a 64-ary search on the
//                  arena_off column, one probe per lane and round), and each lane with a
//                  non-ASCII byte in its 19-byte window checks it, four bytes per step on
//                  packed words.  Where a message boundary falls in the window, the first three
//                  bytes of the message are judged again one by one with nothing before them,
//                  and a complete message's last three for an open sequence (a boundary acts as
//                  an ASCII byte: a message may not start with a continuation byte nor end
//                  inside a sequence); the packed-word verdicts serve for the rest.  A lane that
//                  finds an error stores INVALID to the message's verdict — every writer stores
//                  the same word, so a plain store is enough.
//   k_utf8_finish  eight entries per lane: the open message's PREFIX / tail, and the 16-byte summary
//                  (counts reduced per wave and workgroup, one atomic per workgroup and field).
//
// The entry count of a compact decode (n_messages, pending_bytes) is read from the decode's
// summary in device memory by every kernel, so no host sync sits between decode and validation.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "utf8_rules.h"
#include "uvhttp_ws_amd.h"
#include "ws_engine_int.h"

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr int kBlock = 256;                                   // 4 waves
constexpr int kWaves = kBlock / 64;
constexpr int kVpt = 4;                                       // 16-byte vectors per lane
constexpr uint64_t kWaveBytes = 64ull * 16 * kVpt;            // a wave's contiguous share: 4 KiB
constexpr uint64_t kTileBytes = kWaveBytes * kWaves;          // a workgroup's: 16 KiB
constexpr int kFinishPer = 8;                                 // k_utf8_finish: entries per lane
constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr uint32_t kHigh = 0x80808080u;

struct U8Args {
    const uint8_t* data;
    uint64_t data_len;
    const uvhttp_ws_message_desc_t* msgs;
    uint32_t max_msgs;
    const uvhttp_ws_batch_summary_t* bsum;  // compact decode's summary, or null (generic form)
    uint32_t n_msgs;                        // generic form: entries
    uint32_t* verdict;                      // uvhttp_ws_utf8_verdict_t as a word: status | tail << 8
    uvhttp_ws_utf8_summary_t* out;
};

// what a call judges (wave-uniform): entries [0, n), of which entry `open` (or none) is the
// message still open after the batch, judged as a prefix
struct U8Count {
    uint32_t n, open;
};

__device__ __forceinline__ U8Count u8_count(const U8Args& a) {
    U8Count c;
    c.open = kNone;
    if (!a.bsum) {
        c.n = a.n_msgs;
        return c;
    }
    const uint32_t nm = a.bsum->n_messages;
    const bool pending = a.bsum->pending_bytes != 0;
    const uint64_t n = (uint64_t)nm + (pending ? 1 : 0);
    c.n = n < a.max_msgs ? (uint32_t)n : a.max_msgs;
    if (pending && nm < a.max_msgs) c.open = nm;
    return c;
}

struct U8Msg {
    uint64_t off, end;
    bool text;  // TEXT with its range inside the data: its bytes are examined
};

__device__ __forceinline__ bool u8_range_ok(const U8Args& a, uint64_t off, uint64_t len) {
    return len <= a.data_len && off <= a.data_len - len;
}

__device__ __forceinline__ U8Msg u8_msg(const U8Args& a, uint32_t m) {
    const uvhttp_ws_message_desc_t& d = a.msgs[m];
    U8Msg r;
    r.off = d.arena_off;
    const uint64_t len = d.len;
    r.text = d.opcode == 1 && u8_range_ok(a, r.off, len);
    r.end = r.text ? r.off + len : r.off;
    return r;
}

__global__ __launch_bounds__(kBlock) void k_utf8_init(U8Args a) {
    const U8Count c = u8_count(a);
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i == 0) {
        a.out->n_text = 0;
        a.out->n_invalid = 0;
        a.out->first_invalid = kNone;
        a.out->open_verdict = 0;
    }
    if (i >= c.n) return;
    const uvhttp_ws_message_desc_t& d = a.msgs[i];
    uint32_t st = UVHTTP_WS_UTF8_VALID;
    if (d.opcode != 1) st = UVHTTP_WS_UTF8_NOT_TEXT;
    else if (!u8_range_ok(a, d.arena_off, d.len)) st = UVHTTP_WS_UTF8_BAD_RANGE;
    a.verdict[i] = st;
}

// entries of [0, n) with arena_off <= key, for the whole wave at once: every round probes 64
// evenly spaced entries (one per lane) and keeps the gap the key falls in.  All 64 lanes call it.
// Whatever the column holds, the result stays in [0, n] and only entries below n are read.
__device__ __forceinline__ uint32_t u8_wave_upper_bound(const uvhttp_ws_message_desc_t* msgs, uint32_t n,
                                                        uint64_t key, int lane) {
    uint64_t lo = 0, hi = n;  // the answer lies in [lo, hi]
    while (hi > lo) {
        const uint64_t step = (hi - lo + 63) / 64;
        const uint64_t idx = lo + (uint64_t)(lane + 1) * step - 1;
        const bool le = idx < hi && msgs[idx].arena_off <= key;
        const uint64_t c = (uint64_t)__popcll(__ballot(le));
        const uint64_t nhi = lo + (c + 1) * step - 1;
        lo += c * step;
        if (nhi < hi) hi = nhi;
    }
    return (uint32_t)lo;
}

// the same count for one lane's key, among entries [lo, hi) (a wave whose 4 KiB hold more than
// 64 message starts)
__device__ __forceinline__ uint32_t u8_lane_upper_bound(const uvhttp_ws_message_desc_t* msgs, uint32_t lo,
                                                        uint32_t hi, uint64_t key) {
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (msgs[mid].arena_off <= key) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// 16 bytes at p; bytes at or past data_len read as 0
__device__ __forceinline__ u32x4 u8_load(const U8Args& a, uint64_t p) {
    if (p + 16 <= a.data_len) return __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(a.data + p));
    u32x4 r = {0u, 0u, 0u, 0u};
    for (int j = 0; j < 16; ++j) {
        if (p + j < a.data_len) r[j >> 2] |= (uint32_t)a.data[p + j] << (8 * (j & 3));
    }
    return r;
}

__device__ __forceinline__ void u8_invalid(const U8Args& a, uint32_t m) {
    a.verdict[m] = UVHTTP_WS_UTF8_INVALID;
}

// byte x of a vector, x in [-4, 16): negative = the bytes before it (pw)
__device__ __forceinline__ uint32_t u8_byte(const u32x4& w, uint32_t pw, int x) {
    const int k = x + 4;
    const uint32_t word = k < 4 ? pw : k < 8 ? w[0] : k < 12 ? w[1] : k < 16 ? w[2] : w[3];
    return (word >> (8 * (k & 3))) & 0xFFu;
}

// bytes [a, z) of eight as a mask, 0 <= a, z <= 8
__device__ __forceinline__ uint64_t u8_bytes64(int a, int z) {
    const uint64_t up = z >= 8 ? ~0ull : (1ull << (8 * z)) - 1;
    const uint64_t dn = a >= 8 ? ~0ull : (1ull << (8 * a)) - 1;
    return up & ~dn;
}

__device__ __forceinline__ int u8_clamp8(int x) { return x < 0 ? 0 : x > 8 ? 8 : x; }

// A vector whose 19-byte window is not inside one TEXT message.  `flags` are the packed-word
// verdicts of its 16 bytes taken with the real bytes before each (bit 7 of every byte): right
// for every byte that has three bytes of its own message before it.  So per message in the
// vector only the first three bytes are judged again, with nothing before the message's
// start, and the end of a complete message is checked; the flags serve for the rest.
// `cur` = the last entry starting at or before p (0 if none does), m = that entry.
__device__ __forceinline__ void u8_edges(const U8Args& a, const U8Count& c, uint32_t cur, U8Msg m, uint64_t p,
                                         const u32x4& w, uint32_t pw, const u32x4& flags) {
    const uint64_t flo = flags[0] | ((uint64_t)flags[1] << 32), fhi = flags[2] | ((uint64_t)flags[3] << 32);
    for (uint32_t k = cur;;) {
        if (m.off >= p + 16) break;  // starts past the vector: so do all later ones
        if (m.text && m.end > m.off && m.end > p) {
            // the message in vector coordinates: starts at s (-4 = at least four bytes before
            // the vector), ends at e (17 = past the vector's last byte)
            const int s = m.off >= p ? (int)(m.off - p) : m.off + 4 <= p ? -4 : -(int)(p - m.off);
            const int e = m.end > p + 16 ? 17 : (int)(m.end - p);
            const int z = e < 16 ? e : 16;
            uint32_t bad = 0;
            if (s > -3) {  // some of its first three bytes are in the vector
                uint32_t p1 = 0, p2 = 0, p3 = 0;
                for (int t = 0; t < 3; ++t) {
                    const int x = s + t;
                    if (x < z) {
                        const uint32_t b = u8_byte(w, pw, x);
                        if (x >= 0) bad |= uvws_utf8_bad(b, p1, p2, p3);
                        p3 = p2, p2 = p1, p1 = b;
                    }
                }
            }
            const int f0 = s + 3 > 0 ? s + 3 : 0;  // bytes [f0, z): the flags hold
            if (f0 < z) {
                bad |= (flo & u8_bytes64(u8_clamp8(f0), u8_clamp8(z))) != 0;
                bad |= (fhi & u8_bytes64(u8_clamp8(f0 - 8), u8_clamp8(z - 8))) != 0;
            }
            // a complete message may not end inside a sequence (the open one may: k_utf8_finish)
            if (e <= 16 && k != c.open) {
                const uint32_t e1 = u8_byte(w, pw, e - 1);
                const uint32_t e2 = e - 2 >= s ? u8_byte(w, pw, e - 2) : 0u;
                const uint32_t e3 = e - 3 >= s ? u8_byte(w, pw, e - 3) : 0u;
                bad |= uvws_utf8_open(e1, e2, e3);
            }
            if (bad) u8_invalid(a, k);
        }
        if (++k >= c.n) break;
        m = u8_msg(a, k);
    }
}

__global__ __launch_bounds__(kBlock) void k_utf8_tiles(U8Args a, uint64_t tile_base) {
    const int lane = threadIdx.x & 63;
    const uint64_t wbase = ((tile_base + blockIdx.x) * kWaves + (threadIdx.x >> 6)) * kWaveBytes;
    if (wbase >= a.data_len) return;
    if (a.bsum && wbase >= a.bsum->arena_bytes) return;  // arena past the decoded bytes: scratch

    u32x4 d[kVpt];
#pragma unroll
    for (int v = 0; v < kVpt; ++v) d[v] = u8_load(a, wbase + ((uint64_t)v * 64 + lane) * 16);
    // the four bytes before the wave's share (wbase is a multiple of 4 KiB)
    const uint32_t pw0 = wbase ? *reinterpret_cast<const uint32_t*>(a.data + wbase - 4) : 0u;

    uint32_t any = lane == 0 ? pw0 : 0u;
#pragma unroll
    for (int v = 0; v < kVpt; ++v) any |= d[v][0] | d[v][1] | d[v][2] | d[v][3];
    if (!__any((any & kHigh) != 0)) return;  // all ASCII, nothing carried in: no rule can break

    const U8Count c = u8_count(a);
    if (c.n == 0) return;
    // the wave's place in the table: `ub` entries start at or before wbase; the starts inside
    // the wave's share sit one per lane in `nxt` (`cnt` of them; 64 = there may be more)
    const uint32_t ub = u8_wave_upper_bound(a.msgs, c.n, wbase, lane);
    const uint64_t nxt = (uint64_t)ub + lane < c.n ? a.msgs[ub + lane].arena_off : ~0ull;
    const uint32_t cnt = (uint32_t)__popcll(__ballot(nxt < wbase + kWaveBytes));

    uint32_t ubp[kVpt], pw[kVpt];
#pragma unroll
    for (int v = 0; v < kVpt; ++v) {
        ubp[v] = ub;
        const uint32_t up = __shfl_up(d[v][3], 1);
        const uint32_t last = v ? __shfl(d[v ? v - 1 : 0][3], 63) : pw0;
        pw[v] = lane ? up : last;
    }
    if (cnt < 64) {
        for (uint32_t k = 0; k < cnt; ++k) {
            const uint64_t s = __shfl(nxt, (int)k);
#pragma unroll
            for (int v = 0; v < kVpt; ++v) ubp[v] += s <= wbase + ((uint64_t)v * 64 + lane) * 16 ? 1u : 0u;
        }
    } else {
#pragma unroll
        for (int v = 0; v < kVpt; ++v)
            ubp[v] = u8_lane_upper_bound(a.msgs, ub, c.n, wbase + ((uint64_t)v * 64 + lane) * 16);
    }

#pragma unroll
    for (int v = 0; v < kVpt; ++v) {
        const u32x4 w = d[v];
        if ((((w[0] | w[1]) | (w[2] | w[3])) | pw[v]) & kHigh) {
            const uint64_t p = wbase + ((uint64_t)v * 64 + lane) * 16;
            const uint32_t cur = ubp[v] ? ubp[v] - 1 : 0u;
            const U8Msg m = u8_msg(a, cur);
            uvws_utf8_flags_t pf = uvws_utf8_flags(pw[v]);
            u32x4 flags;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const uvws_utf8_flags_t f = uvws_utf8_flags(w[i]);
                flags[i] = uvws_utf8_bad4(w[i], f, pf);
                pf = f;
            }
            if (m.text && p >= m.off + 3 && p + 16 < m.end) {
                // the window lies inside one TEXT message, whose end another lane checks
                if ((flags[0] | flags[1]) | (flags[2] | flags[3])) u8_invalid(a, cur);
            } else {
                u8_edges(a, c, cur, m, p, w, pw[v], flags);
            }
        }
    }
}

__global__ __launch_bounds__(kBlock) void k_utf8_finish(U8Args a) {
    __shared__ uint32_t s_text, s_inv, s_first;
    const U8Count c = u8_count(a);
    if (threadIdx.x == 0) s_text = 0, s_inv = 0, s_first = kNone;
    __syncthreads();
    uint32_t n_text = 0, n_inv = 0, first = kNone;  // the wave's (uniform)
    for (int j = 0; j < kFinishPer; ++j) {
        const uint64_t i = ((uint64_t)blockIdx.x * kFinishPer + j) * kBlock + threadIdx.x;
        bool text = false, inv = false;
        if (i < c.n) {
            uint32_t v = a.verdict[i];
            if (i == c.open) {
                if (v == UVHTTP_WS_UTF8_VALID) {
                    // valid so far (k_utf8_tiles checked every byte): the sequence still open
                    const uint64_t off = a.msgs[i].arena_off, len = a.msgs[i].len;
                    const uint8_t* e = a.data + off + len;
                    const uint32_t p1 = len >= 1 ? e[-1] : 0u, p2 = len >= 2 ? e[-2] : 0u, p3 = len >= 3 ? e[-3] : 0u;
                    v = UVHTTP_WS_UTF8_PREFIX | (uvws_utf8_open(p1, p2, p3) << 8);
                    a.verdict[i] = v;
                }
                a.out->open_verdict = v;
            }
            const uint32_t st = v & 0xFFu;
            text = st != UVHTTP_WS_UTF8_NOT_TEXT;
            inv = st == UVHTTP_WS_UTF8_INVALID || st == UVHTTP_WS_UTF8_BAD_RANGE;
        }
        const uint64_t mt = __ballot(text), mi = __ballot(inv);
        n_text += (uint32_t)__popcll(mt);
        n_inv += (uint32_t)__popcll(mi);
        if (mi && first == kNone)  // indices ascend with j and with the lane
            first = (uint32_t)(i - (threadIdx.x & 63)) + (uint32_t)(__ffsll((unsigned long long)mi) - 1);
    }
    // one LDS atomic per wave, then one device atomic per workgroup and field
    if ((threadIdx.x & 63) == 0) {
        if (n_text) atomicAdd(&s_text, n_text);
        if (n_inv) atomicAdd(&s_inv, n_inv), atomicMin(&s_first, first);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (s_text) atomicAdd(&a.out->n_text, s_text);
        if (s_inv) atomicAdd(&a.out->n_invalid, s_inv), atomicMin(&a.out->first_invalid, s_first);
    }
}

}  // namespace

extern "C" int uvhttp_ws_gpu_validate_utf8(uvhttp_ws_gpu_engine_t* e, const uint8_t* d_data, uint64_t data_len,
                                           const uvhttp_ws_message_desc_t* d_msgs, uint32_t max_msgs,
                                           const uvhttp_ws_batch_summary_t* d_batch_summary, uint32_t n_msgs,
                                           uvhttp_ws_utf8_verdict_t* d_verdict,
                                           uvhttp_ws_utf8_summary_t* d_utf8_summary, void* stream) {
    if (!e) return UVHTTP_WS_GPU_EINVAL;
    if (!d_msgs || !d_verdict || !d_utf8_summary || (!d_data && data_len))
        return uvws_set_err(e, UVHTTP_WS_GPU_EINVAL, "validate_utf8: NULL argument");
    if (((uintptr_t)d_data & 15u) || ((uintptr_t)d_msgs & 7u) || ((uintptr_t)d_batch_summary & 7u) ||
        ((uintptr_t)d_verdict & 3u) || ((uintptr_t)d_utf8_summary & 3u))
        return uvws_set_err(e, UVHTTP_WS_GPU_EINVAL, "validate_utf8: misaligned argument");
    if (!d_batch_summary && n_msgs > max_msgs)
        return uvws_set_err(e, UVHTTP_WS_GPU_EINVAL, "validate_utf8: n_msgs > max_msgs");
    static_assert(sizeof(uvhttp_ws_utf8_verdict_t) == 4 && sizeof(uvhttp_ws_utf8_summary_t) == 16, "ABI");

    U8Args a;
    a.data = d_data;
    a.data_len = data_len;
    a.msgs = d_msgs;
    a.max_msgs = max_msgs;
    a.bsum = d_batch_summary;
    a.n_msgs = d_batch_summary ? 0 : n_msgs;
    a.verdict = reinterpret_cast<uint32_t*>(d_verdict);
    a.out = d_utf8_summary;

    hipStream_t s = (hipStream_t)stream;
    const int prev = uvws_call_enter(e, s);
    // entries: the generic form's count, or (read on the device) at most max_msgs
    const uint64_t n_cap = d_batch_summary ? max_msgs : n_msgs;
    const uint32_t grid_n = (uint32_t)(n_cap ? (n_cap + kBlock - 1) / kBlock : 1);
    hipLaunchKernelGGL(k_utf8_init, dim3(grid_n), dim3(kBlock), 0, s, a);
    const uint64_t tiles = (data_len + kTileBytes - 1) / kTileBytes;
    engine_grid_chunks(e, n_cap ? tiles : 0, [&](uint32_t grid, uint64_t tb) {
        hipLaunchKernelGGL(k_utf8_tiles, dim3(grid), dim3(kBlock), 0, s, a, tb);
    });
    const uint64_t per_f = (uint64_t)kBlock * kFinishPer;
    const uint32_t grid_f = (uint32_t)(n_cap ? (n_cap + per_f - 1) / per_f : 1);
    hipLaunchKernelGGL(k_utf8_finish, dim3(grid_f), dim3(kBlock), 0, s, a);
    return uvws_call_leave(e, prev, "validate_utf8 launch");
}
