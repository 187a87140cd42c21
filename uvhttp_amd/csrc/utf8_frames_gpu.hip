// utf8_frames_gpu.hip — UTF-8 validation of TEXT frames where an in-place or stream decode left
// them (include/uvhttp_ws_amd.h: uvhttp_ws_gpu_validate_utf8_streams / _inplace): a message's
// bytes are split over frames, with headers, control frames and other connections' bytes in
// between, and a message may be open across calls.  Nine short launches, per-frame scratch in
// the engine, no waiting between workgroups:
//
//   k_fu_init     marks[f] = 0 per descriptor; the summary zeroed
//   k_fu_conns    one lane per connection: its per-connection words (first_invalid, first bad
//                 range, text-frame counts, the state after its last frame = the carried-in
//                 state) and a head mark at its first delivered descriptor
//   k_fu_reduce   one lane per descriptor: the frame's effect on the connection's message state
//                 as a 64-bit element (below), and the workgroup's aggregate
//   k_scan_top    one workgroup: the aggregates' inclusive prefixes (ws_scan.h)
//   k_fu_apply    one lane per descriptor: the state carried into the frame (is it text, and the
//                 up to three bytes before its first byte) and its connection from the scan.
//                 Everything a carry can decide is judged here: the frame's first three bytes
//                 against the carried ones, the open sequence at a FIN frame (an empty FIN
//                 CONTINUATION included), frames of up to three bytes whole, bad ranges and
//                 CLOSE reasons.  A TEXT frame longer than three bytes is flagged as a segment
//                 [payload_off + 3, payload end) for the payload pass
//   k_scan_top    (sums: segments | text frames << 32) and k_fu_segs: the flagged segments
//                 compacted into an ascending table (start, end, frame | connection << 32), and
//                 every connection's text frames as the running count at its last frame minus
//                 the count before its first (no atomics: in place all frames share a connection)
//   k_fu_tiles    position-indexed over the wire, as k_utf8_tiles: 16-byte non-temporal loads,
//                 the all-ASCII exit per wave, the packed four-bytes-at-a-time rules with the
//                 real bytes before each byte.  Inside a segment every byte has three bytes of
//                 its own frame before it, so the flags hold as they are.  A wave with no flagged
//                 byte leaves (valid text flags nothing: only waves that hold a header, a BINARY
//                 payload or an error go on); the others find their place in the table by the
//                 64-ary search, take the segments that meet their 4 KiB one per lane, and test
//                 them one per round with the bounds the same in all lanes.  A flagged byte
//                 inside a segment does atomicMin(first_invalid[connection], frame); flagged
//                 bytes outside the segments (headers, BINARY payloads, undelivered frames)
//                 raise nothing
//   k_fu_finish   one lane per connection: status, state and the 16-byte summary (reduced per
//                 wave and workgroup, one device atomic per workgroup and field)
//
// The scan element (one per descriptor, 64 bits): bits 0-23 the last three bytes of the open
// message (most recent in the low byte, zero where the message has fewer: a zero byte before a
// byte acts as no byte at all under utf8_rules.h), 24-25 how many bytes the frame appends
// (saturating at 3), 26-27 the open message's opcode (0 none), 28 "constant": the element fixes
// the state whatever came before (a start frame, a FIN frame, a connection's first frame), 29
// "head": it holds a connection's first frame, 32-63 that connection.  a then b: b constant ->
// b's state, else a's state with b's bytes appended; the head and connection of the later head.
// That is composition of functions on the state, so it is associative and an inclusive scan
// gives every frame the state after it; the state before it is its left neighbour's, or the
// carried-in state at a head.  Descriptors after a connection's delivered frames may hold
// anything: they sit behind every judged frame of their connection and before the next head, so
// whatever they add to the scan is never used, and their payload is read only inside the wire.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "utf8_rules.h"
#include "uvhttp_ws_amd.h"
#include "ws_engine_int.h"
#include "ws_scan.h"

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr int kVpt = 4;                              // k_fu_tiles: 16-byte vectors per lane
constexpr uint64_t kWaveBytes = 64ull * 16 * kVpt;   // a wave's contiguous share: 4 KiB
constexpr uint64_t kTileBytes = kWaveBytes * kWaves; // a workgroup's: 16 KiB
constexpr uint32_t kHigh = 0x80808080u;

constexpr uint64_t kStBytes = 0xFFFFFFull;
constexpr int kStKShift = 24, kStOpShift = 26;
constexpr uint64_t kStConst = 1ull << 28, kStHead = 1ull << 29;
constexpr uint64_t kStLow = 0xFFFFFFFFull;
// k_fu_apply's word per descriptor: a segment for the payload pass, a TEXT frame, a judged frame
constexpr uint64_t kInfoSeg = 1, kInfoText = 2, kInfoJudged = 4;

struct FuArgs {
    const uint8_t* wire;
    uint64_t wire_len;
    const uvhttp_ws_frame_desc_t* desc;
    uint32_t max_frames;
    uint32_t n_streams;
    const uvhttp_ws_stream_t* streams;           // null: the in-place form (one connection)
    const uvhttp_ws_stream_result_t* results;
    const uvhttp_ws_utf8_state_t* state_in;      // or null
    const uvhttp_ws_batch_summary_t* bsum;       // the in-place form's n_delivered
    uint32_t flags;
    uvhttp_ws_utf8_conn_verdict_t* verdict;
    uvhttp_ws_utf8_frames_summary_t* out;
    // engine scratch
    uint32_t* marks;      // [max_frames] connection + 1 at its first delivered descriptor
    uint64_t* elem;       // [max_frames] scan elements; after k_fu_apply: kInfo* | connection << 32
    uint64_t* agg1;       // [blocks] state aggregates, then their inclusive prefixes
    uint64_t* agg2;       // [blocks] segments | text frames << 32, then their inclusive prefixes
    uint64_t* seg_start;  // [max_frames] the segment table (agg2[blocks - 1] entries)
    uint64_t* seg_end;
    uint64_t* seg_fc;     // frame | connection << 32
    uint32_t* first_inv;  // [n_streams]
    uint32_t* first_bad;
    uint32_t* tbeg;       // text frames before the connection's first frame, and up to its last
    uint32_t* tend;
    uint32_t* open;       // low word of the state after the connection's last delivered frame
};

struct StateOp {
    __device__ __forceinline__ uint64_t operator()(uint64_t a, uint64_t b) const {
        const uint64_t hc = (b & kStHead) ? (b & ~kStLow) | kStHead : (a & ~kStLow) | (a & kStHead);
        if (b & kStConst) return (b & kStLow & ~kStHead) | hc;
        const uint32_t bk = (uint32_t)(b >> kStKShift) & 3u, ak = (uint32_t)(a >> kStKShift) & 3u;
        const uint64_t bytes = (((a & kStBytes) << (8 * bk)) | (b & kStBytes)) & kStBytes;
        const uint32_t k = ak + bk > 3 ? 3u : ak + bk;
        const uint64_t low = bytes | ((uint64_t)k << kStKShift) | (a & (3ull << kStOpShift)) | (a & kStConst);
        return low | hc;
    }
};

// connection s's judged descriptors, inside [0, max_frames).  Not call_failed: after ERR_DEVICE
// the delivered frames are still judged (include/uvhttp_ws_amd.h, validate_utf8_streams)
__device__ __forceinline__ Range conn_range(const FuArgs& a, uint32_t s) {
    Range r;
    if (!a.results) {
        r.ff = 0;
        r.nd = a.bsum->n_delivered;
    } else {
        const uvhttp_ws_stream_result_t& q = a.results[s];
        r.ff = q.first_frame;
        r.nd = q.n_delivered;
        if (q.first_status == UVHTTP_WS_FRAME_ERR_CAPACITY || q.first_status == UVHTTP_WS_FRAME_ERR_LAYOUT) r.nd = 0;
    }
    return clamp_range(r, a.max_frames);
}

// the state carried into connection s: a constant head element
__device__ __forceinline__ uint64_t conn_seed(const FuArgs& a, uint32_t s) {
    uint64_t op = 0, bytes = 0;
    if (a.streams) {
        const uvhttp_ws_stream_t& st = a.streams[s];
        if (st.pending_bytes != 0 && (st.pending_opcode == 1 || st.pending_opcode == 2)) op = (uint64_t)st.pending_opcode;
        if (op == 1 && a.state_in) {
            const uvhttp_ws_utf8_state_t in = a.state_in[s];
            const uint32_t n = in.n > 3 ? 3u : in.n;
            for (uint32_t k = 0; k < n; ++k) bytes = (bytes << 8) | in.pend[k];
        }
    }
    return bytes | (op << kStOpShift) | kStConst | kStHead | ((uint64_t)s << 32);
}

// the last min(3, len) payload bytes, most recent in the low byte (range checked by the caller)
__device__ __forceinline__ uint32_t tail_bytes(const FuArgs& a, uint64_t off, uint64_t len, uint32_t k) {
    uint32_t n = 0;
    for (uint32_t t = 0; t < k; ++t) n = (n << 8) | a.wire[off + len - k + t];
    return n;
}

__device__ __forceinline__ uint64_t frame_elem(const FuArgs& a, uint32_t f) {
    const uvhttp_ws_frame_desc_t& d = a.desc[f];
    uint64_t e = 0;  // identity: control frames, frames that were not delivered
    const uint32_t op = d.opcode;
    if (d.status == UVHTTP_WS_FRAME_OK && op <= 2) {
        const bool fin = (d.flags & UVHTTP_WS_FLAG_FIN) != 0;
        if (fin) {
            e = kStConst;
        } else {
            const uint64_t len = d.payload_len;
            uint32_t k = 0, n = 0;
            if (range_ok(a.wire_len, d.payload_off, len)) {
                k = len < 3 ? (uint32_t)len : 3u;
                n = tail_bytes(a, d.payload_off, len, k);
            }
            e = op == 0 ? (uint64_t)n | ((uint64_t)k << kStKShift)
                        : (uint64_t)n | ((uint64_t)op << kStOpShift) | kStConst;
        }
    }
    const uint32_t mk = a.marks[f];
    if (mk) e = StateOp()(conn_seed(a, mk - 1), e);
    return e;
}

__global__ __launch_bounds__(kBlock) void k_fu_init(FuArgs a) {
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i == 0) {
        a.out->n_text_frames = 0;
        a.out->n_invalid_conns = 0;
        a.out->first_invalid_conn = kNone;
        a.out->n_open_conns = 0;
    }
    if (i < a.max_frames) a.marks[i] = 0;
}

__global__ __launch_bounds__(kBlock) void k_fu_conns(FuArgs a) {
    const uint64_t s = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (s >= a.n_streams) return;
    a.first_inv[s] = kNone;
    a.first_bad[s] = kNone;
    a.tbeg[s] = 0;
    a.tend[s] = 0;
    a.open[s] = (uint32_t)conn_seed(a, (uint32_t)s);
    const Range r = conn_range(a, (uint32_t)s);
    if (r.nd) a.marks[r.ff] = (uint32_t)s + 1;
}

__global__ __launch_bounds__(kBlock) void k_fu_reduce(FuArgs a) {
    __shared__ uint64_t s_wave[kWaves];
    const uint64_t f = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    uint64_t e = 0;
    if (f < a.max_frames) {
        e = frame_elem(a, (uint32_t)f);
        a.elem[f] = e;
    }
    uint64_t tot;
    (void)block_scan(e, StateOp(), 0, s_wave, &tot);
    if (threadIdx.x == 0) a.agg1[blockIdx.x] = tot;
}

__device__ __forceinline__ void blame(uint32_t* first, uint32_t conn, uint32_t f) { atomicMin(&first[conn], f); }

__global__ __launch_bounds__(kBlock) void k_fu_apply(FuArgs a) {
    __shared__ uint64_t s_wave[kWaves];
    __shared__ uint64_t s_inc[kBlock];
    __shared__ uint64_t s_cnt[kWaves];
    const int lane = threadIdx.x & 63;
    const uint64_t f = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    const bool live = f < a.max_frames;
    const uint64_t e = live ? a.elem[f] : 0;
    const uint64_t pre = blockIdx.x ? a.agg1[blockIdx.x - 1] : 0;
    uint64_t tot;
    const uint64_t inc = StateOp()(pre, block_scan(e, StateOp(), 0, s_wave, &tot));
    s_inc[threadIdx.x] = inc;
    __syncthreads();
    uint64_t carry = threadIdx.x ? s_inc[threadIdx.x - 1] : pre;

    bool text = false, seg = false, judged = false;
    uint32_t conn = 0;
    if (live && (inc & kStHead)) {
        conn = (uint32_t)(inc >> 32);
        if (conn < a.n_streams) {
            const Range r = conn_range(a, conn);
            const uvhttp_ws_frame_desc_t& d = a.desc[f];
            if (f >= r.ff && f - r.ff < r.nd && d.status == UVHTTP_WS_FRAME_OK) {
                judged = true;
                if (f == r.ff) carry = conn_seed(a, conn);
                if (f - r.ff == r.nd - 1) a.open[conn] = (uint32_t)inc;
                const uint32_t op = d.opcode;
                const uint64_t off = d.payload_off, len = d.payload_len;
                const bool fin = (d.flags & UVHTTP_WS_FLAG_FIN) != 0;
                const uint32_t mop = op == 0 ? (uint32_t)(carry >> kStOpShift) & 3u : op;
                if (op <= 2 && mop == 1) {
                    text = true;
                    if (!range_ok(a.wire_len, off, len)) {
                        blame(a.first_bad, conn, (uint32_t)f);
                    } else {
                        const uint32_t cb = op == 0 ? (uint32_t)(carry & kStBytes) : 0u;
                        uint32_t p1 = cb & 0xFFu, p2 = (cb >> 8) & 0xFFu, p3 = cb >> 16;
                        uint32_t bad = 0;
                        const uint32_t k = len < 3 ? (uint32_t)len : 3u;
                        for (uint32_t t = 0; t < k; ++t) {
                            const uint32_t b = a.wire[off + t];
                            bad |= uvws_utf8_bad(b, p1, p2, p3);
                            p3 = p2, p2 = p1, p1 = b;
                        }
                        if (fin) {  // the message's last three bytes, carried ones included
                            const uint32_t t3 = ((cb << (8 * k)) | tail_bytes(a, off, len, k)) & 0xFFFFFFu;
                            bad |= uvws_utf8_open(t3 & 0xFFu, (t3 >> 8) & 0xFFu, t3 >> 16);
                        }
                        if (bad) blame(a.first_inv, conn, (uint32_t)f);
                        seg = len > 3;
                    }
                } else if (op == 8 && (a.flags & UVHTTP_WS_UTF8_CHECK_CLOSE) && len > 2) {
                    if (!range_ok(a.wire_len, off, len)) {
                        blame(a.first_bad, conn, (uint32_t)f);
                    } else {
                        // a delivered control frame has at most 125 bytes
                        const uint32_t n = len > 125 ? 125u : (uint32_t)len;
                        uint32_t p1 = 0, p2 = 0, p3 = 0, bad = 0;
                        for (uint32_t t = 2; t < n; ++t) {
                            const uint32_t b = a.wire[off + t];
                            bad |= uvws_utf8_bad(b, p1, p2, p3);
                            p3 = p2, p2 = p1, p1 = b;
                        }
                        bad |= uvws_utf8_open(p1, p2, p3);
                        if (bad) blame(a.first_inv, conn, (uint32_t)f);
                    }
                }
            }
        }
    }
    if (live)
        a.elem[f] = (seg ? kInfoSeg : 0) | (text ? kInfoText : 0) | (judged ? kInfoJudged : 0) | ((uint64_t)conn << 32);

    // the workgroup's segments and text frames, for the second scan
    const uint64_t wc = (uint64_t)__popcll(__ballot(seg)) | ((uint64_t)__popcll(__ballot(text)) << 32);
    if (lane == 0) s_cnt[threadIdx.x >> 6] = wc;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t c = 0;
        for (int k = 0; k < kWaves; ++k) c += s_cnt[k];
        a.agg2[blockIdx.x] = c;
    }
}

__global__ __launch_bounds__(kBlock) void k_fu_segs(FuArgs a) {
    __shared__ uint64_t s_wave[kWaves];
    const uint64_t f = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    const uint64_t info = f < a.max_frames ? a.elem[f] : 0;
    const uint64_t mine = ((info & kInfoSeg) ? 1ull : 0ull) | ((info & kInfoText) ? 1ull << 32 : 0ull);
    uint64_t tot;
    const uint64_t inc = (blockIdx.x ? a.agg2[blockIdx.x - 1] : 0ull) + block_scan(mine, AddOp(), 0, s_wave, &tot);
    if (info & kInfoJudged) {
        // the connection's text frames = the running count at its last frame - before its first
        const uint32_t conn = (uint32_t)(info >> 32);
        const Range r = conn_range(a, conn);
        if (f == r.ff) a.tbeg[conn] = (uint32_t)((inc - mine) >> 32);
        if (f - r.ff == r.nd - 1) a.tend[conn] = (uint32_t)(inc >> 32);
    }
    if (info & kInfoSeg) {
        const uint32_t idx = (uint32_t)inc - 1;
        const uvhttp_ws_frame_desc_t& d = a.desc[f];
        a.seg_start[idx] = d.payload_off + 3;
        a.seg_end[idx] = d.payload_off + d.payload_len;
        a.seg_fc[idx] = (uint64_t)(uint32_t)f | (info & ~kStLow);
    }
}

// entries of key[0, n) <= x, for the whole wave at once: every round probes 64 evenly spaced
// entries (one per lane) and keeps the gap x falls in.  All 64 lanes call it.  Whatever the
// column holds, the result stays in [0, n] and only entries below n are read.
__device__ __forceinline__ uint32_t wave_upper_bound(const uint64_t* key, uint32_t n, uint64_t x, int lane) {
    uint64_t lo = 0, hi = n;
    while (hi > lo) {
        const uint64_t step = (hi - lo + 63) / 64;
        const uint64_t idx = lo + (uint64_t)(lane + 1) * step - 1;
        const bool le = idx < hi && key[idx] <= x;
        const uint64_t c = (uint64_t)__popcll(__ballot(le));
        const uint64_t nhi = lo + (c + 1) * step - 1;
        lo += c * step;
        if (nhi < hi) hi = nhi;
    }
    return (uint32_t)lo;
}

__device__ __forceinline__ uint32_t lane_upper_bound(const uint64_t* key, uint32_t lo, uint32_t hi, uint64_t x) {
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (key[mid] <= x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// 16 bytes at p; bytes at or past wire_len read as 0
__device__ __forceinline__ u32x4 load16(const FuArgs& a, uint64_t p) {
    if (p + 16 <= a.wire_len) return __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(a.wire + p));
    u32x4 r = {0u, 0u, 0u, 0u};
    for (int j = 0; j < 16; ++j) {
        if (p + j < a.wire_len) r[j >> 2] |= (uint32_t)a.wire[p + j] << (8 * (j & 3));
    }
    return r;
}

__global__ __launch_bounds__(kBlock) void k_fu_tiles(FuArgs a, uint64_t tile_base, uint32_t n_blocks) {
    const int lane = threadIdx.x & 63;
    const uint64_t wbase = ((tile_base + blockIdx.x) * kWaves + (threadIdx.x >> 6)) * kWaveBytes;
    if (wbase >= a.wire_len) return;

    u32x4 d[kVpt];
#pragma unroll
    for (int v = 0; v < kVpt; ++v) d[v] = load16(a, wbase + ((uint64_t)v * 64 + lane) * 16);
    const uint32_t pw0 = wbase ? *reinterpret_cast<const uint32_t*>(a.wire + wbase - 4) : 0u;

    uint32_t any = 0;
#pragma unroll
    for (int v = 0; v < kVpt; ++v) any |= d[v][0] | d[v][1] | d[v][2] | d[v][3];
    // all ASCII, the four bytes before the share included (a lead there would make the share's
    // first bytes break a rule): no byte of the share can
    if (lane == 0) any |= pw0;
    if (!__any((any & kHigh) != 0)) return;

    const uint32_t n = (uint32_t)a.agg2[n_blocks - 1];
    if (n == 0) return;

    // the packed-word verdicts of every vector, taken with the real bytes before each byte:
    // one bit per byte
    uint32_t fm[kVpt];
    uint32_t anyf = 0;
#pragma unroll
    for (int v = 0; v < kVpt; ++v) {
        const u32x4 w = d[v];
        const uint32_t up = __shfl_up(w[3], 1);
        const uint32_t last = v ? __shfl(d[v ? v - 1 : 0][3], 63) : pw0;
        const uint32_t pw = lane ? up : last;
        fm[v] = 0;
        if ((((w[0] | w[1]) | (w[2] | w[3])) | pw) & kHigh) {
            uvws_utf8_flags_t pf = uvws_utf8_flags(pw);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const uvws_utf8_flags_t fl = uvws_utf8_flags(w[i]);
                // bit 7 of every byte -> four bits (the product puts byte k's at bit 21 + k, no carries)
                fm[v] |= (((uvws_utf8_bad4(w[i], fl, pf) >> 7) * 0x00204081u) >> 21 & 0xFu) << (4 * i);
                pf = fl;
            }
        }
        anyf |= fm[v];
    }
    if (!__any(anyf != 0)) return;  // nothing in the share breaks a rule, inside a segment or not

    // the wave's place in the table: `ub` segments start at or before wbase.  Lane j takes
    // segment k0 + j: the one that may reach into the share from below, then those that start
    // in it (`inside` of the 64 start before its end; 64 = there may be more), their bounds
    // relative to wbase
    const uint32_t ub = wave_upper_bound(a.seg_start, n, wbase, lane);
    const uint32_t k0 = ub ? ub - 1 : 0u;
    const bool have = (uint64_t)k0 + lane < n;
    const uint64_t sj = have ? a.seg_start[k0 + lane] : ~0ull;
    const uint64_t zj = have ? a.seg_end[k0 + lane] : 0ull;
    const uint64_t fj = have ? a.seg_fc[k0 + lane] : 0ull;
    const uint32_t inside = (uint32_t)__popcll(__ballot(sj < wbase + kWaveBytes));
    constexpr int kFar = 1 << 30;
    const int rs = sj < wbase ? -1 : sj - wbase > (uint64_t)kFar ? kFar : (int)(sj - wbase);
    const int rz = zj <= wbase ? -1 : zj - wbase > (uint64_t)kFar ? kFar : (int)(zj - wbase);

    if (inside < 64) {
        // per vector: the last held segment starting at or before it (the first if none does) ...
        int cur[kVpt];
#pragma unroll
        for (int v = 0; v < kVpt; ++v) cur[v] = -1;
        for (uint32_t j = 0; j < inside; ++j) {
            const int s = __shfl(rs, (int)j);
#pragma unroll
            for (int v = 0; v < kVpt; ++v) cur[v] += s <= (v * 64 + lane) * 16 ? 1 : 0;
        }
        // ... and that one and the next three are all that can meet its 16 bytes: segments are
        // at least a byte long and at least five bytes apart.  Every lane takes part in every
        // round, so the cross-lane reads see all lanes.
#pragma unroll
        for (int v = 0; v < kVpt; ++v) {
            if (!__any(fm[v] != 0)) continue;
            const int pv = (v * 64 + lane) * 16;
            const int c0 = cur[v] < 0 ? 0 : cur[v];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int idx = c0 + r;
                const bool held = idx < (int)inside;
                const int src = held ? idx : 0;
                const int s = __shfl(rs, src), z = __shfl(rz, src);
                const uint64_t fc = __shfl(fj, src);
                if (held && fm[v] && s < pv + 16 && z > pv) {
                    const int lo = s > pv ? s - pv : 0, hi = z < pv + 16 ? z - pv : 16;
                    if (fm[v] & ((1u << hi) - 1u) & ~((1u << lo) - 1u)) {
                        const uint32_t conn = (uint32_t)(fc >> 32);
                        if (conn < a.n_streams) blame(a.first_inv, conn, (uint32_t)fc);
                    }
                }
            }
        }
        return;
    }
    // more than a wave's worth of segments in 4 KiB (frames of a few bytes): every lane finds
    // and walks its own.  They are disjoint, at least one byte long and at least five bytes
    // apart, so a vector meets a few at most.
#pragma unroll
    for (int v = 0; v < kVpt; ++v) {
        if (fm[v] == 0) continue;
        const uint64_t p = wbase + ((uint64_t)v * 64 + lane) * 16;
        const uint32_t ubp = lane_upper_bound(a.seg_start, ub, n, p);
        for (uint32_t k = ubp ? ubp - 1 : 0u; k < n; ++k) {
            const uint64_t sg = a.seg_start[k], z = a.seg_end[k];
            if (sg >= p + 16) break;
            if (z <= p) continue;
            const int lo = sg > p ? (int)(sg - p) : 0, hi = z < p + 16 ? (int)(z - p) : 16;
            if (fm[v] & ((1u << hi) - 1u) & ~((1u << lo) - 1u)) {
                const uint64_t fc = a.seg_fc[k];
                const uint32_t conn = (uint32_t)(fc >> 32);
                if (conn < a.n_streams) blame(a.first_inv, conn, (uint32_t)fc);
            }
        }
    }
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

__global__ __launch_bounds__(kBlock) void k_fu_finish(FuArgs a) {
    __shared__ uint32_t s_text, s_inv, s_first, s_open;
    if (threadIdx.x == 0) s_text = 0, s_inv = 0, s_first = kNone, s_open = 0;
    __syncthreads();
    const uint64_t s = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    uint32_t nt = 0;
    bool inv = false, open = false;
    if (s < a.n_streams) {
        const uint32_t fi = a.first_inv[s], fb = a.first_bad[s];
        nt = a.tend[s] - a.tbeg[s];
        uvhttp_ws_utf8_conn_verdict_t v;
        v.first_invalid = kNone;
        v.n_text_frames = nt;
        v.state.pend[0] = v.state.pend[1] = v.state.pend[2] = 0;
        v.state.n = 0;
        v.status = UVHTTP_WS_UTF8_VALID;
        v.reserved[0] = v.reserved[1] = v.reserved[2] = 0;
        if (fb != kNone && fb <= fi) {
            v.status = UVHTTP_WS_UTF8_BAD_RANGE;
            v.first_invalid = fb;
        } else if (fi != kNone) {
            v.status = UVHTTP_WS_UTF8_INVALID;
            v.first_invalid = fi;
        } else {
            const uint32_t st = a.open[s];
            if (((st >> kStOpShift) & 3u) == 1u) {
                const uint32_t p1 = st & 0xFFu, p2 = (st >> 8) & 0xFFu, p3 = (st >> 16) & 0xFFu;
                const uint32_t n = uvws_utf8_open(p1, p2, p3);
                v.status = UVHTTP_WS_UTF8_PREFIX;
                v.state.n = (uint8_t)n;
                v.state.pend[0] = (uint8_t)(n == 1 ? p1 : n == 2 ? p2 : n == 3 ? p3 : 0);
                v.state.pend[1] = (uint8_t)(n == 2 ? p1 : n == 3 ? p2 : 0);
                v.state.pend[2] = (uint8_t)(n == 3 ? p1 : 0);
            }
        }
        a.verdict[s] = v;
        inv = v.status == UVHTTP_WS_UTF8_INVALID || v.status == UVHTTP_WS_UTF8_BAD_RANGE;
        open = v.status == UVHTTP_WS_UTF8_PREFIX;
    }
    // one LDS atomic per wave, then one device atomic per workgroup and field
    const uint32_t wt = wave_sum(nt);
    const uint64_t mi = __ballot(inv), mo = __ballot(open);
    if ((threadIdx.x & 63) == 0) {
        if (wt) atomicAdd(&s_text, wt);
        if (mi) {
            atomicAdd(&s_inv, (uint32_t)__popcll(mi));
            atomicMin(&s_first, (uint32_t)s + (uint32_t)(__ffsll((unsigned long long)mi) - 1));
        }
        if (mo) atomicAdd(&s_open, (uint32_t)__popcll(mo));
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (s_text) atomicAdd(&a.out->n_text_frames, s_text);
        if (s_inv) atomicAdd(&a.out->n_invalid_conns, s_inv), atomicMin(&a.out->first_invalid_conn, s_first);
        if (s_open) atomicAdd(&a.out->n_open_conns, s_open);
    }
}

void fu_carve(Carver& c, FuArgs& a, uint64_t nb) {
    const uint64_t F = a.max_frames, S = a.n_streams;
    a.elem = c.take<uint64_t>(F);
    a.seg_start = c.take<uint64_t>(F);
    a.seg_end = c.take<uint64_t>(F);
    a.seg_fc = c.take<uint64_t>(F);
    a.agg1 = c.take<uint64_t>(nb);
    a.marks = c.take<uint32_t>(F);
    a.agg2 = c.take<uint64_t>(nb);
    a.first_inv = c.take<uint32_t>(S);
    a.first_bad = c.take<uint32_t>(S);
    a.tbeg = c.take<uint32_t>(S);
    a.tend = c.take<uint32_t>(S);
    a.open = c.take<uint32_t>(S);
}

int fu_run(uvhttp_ws_gpu_engine_t* e, FuArgs a, void* stream, const char* what) {
    static_assert(sizeof(uvhttp_ws_utf8_conn_verdict_t) == 16 && sizeof(uvhttp_ws_utf8_frames_summary_t) == 16, "ABI");
    const uint32_t blocks = (uint32_t)(((uint64_t)a.max_frames + kBlock - 1) / kBlock);
    Carver count{nullptr};
    fu_carve(count, a, blocks ? blocks : 1);

    hipStream_t s = (hipStream_t)stream;
    const int prev = uvws_call_enter(e, s);
    char* mem = static_cast<char*>(uvws_utf8_scratch(e, count.bytes(), s));
    if (!mem) {
        (void)uvws_call_leave(e, prev, what);
        return uvws_set_err(e, UVHTTP_WS_GPU_ENOMEM, "validate_utf8 frame scratch (a captured call must not grow it)");
    }
    Carver carve{mem};
    fu_carve(carve, a, blocks ? blocks : 1);

    const uint32_t grid_s = (uint32_t)(((uint64_t)a.n_streams + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(k_fu_init, dim3(blocks ? blocks : 1), dim3(kBlock), 0, s, a);
    if (grid_s) hipLaunchKernelGGL(k_fu_conns, dim3(grid_s), dim3(kBlock), 0, s, a);
    if (blocks && grid_s) {
        hipLaunchKernelGGL(k_fu_reduce, dim3(blocks), dim3(kBlock), 0, s, a);
        hipLaunchKernelGGL((k_scan_top<StateOp>), dim3(1), dim3(kBlock), 0, s, a.agg1, a.agg1, blocks);
        hipLaunchKernelGGL(k_fu_apply, dim3(blocks), dim3(kBlock), 0, s, a);
        hipLaunchKernelGGL((k_scan_top<AddOp>), dim3(1), dim3(kBlock), 0, s, a.agg2, a.agg2, blocks);
        hipLaunchKernelGGL(k_fu_segs, dim3(blocks), dim3(kBlock), 0, s, a);
        const uint64_t tiles = (a.wire_len + kTileBytes - 1) / kTileBytes;
        engine_grid_chunks(e, tiles, [&](uint32_t grid, uint64_t tb) {
            hipLaunchKernelGGL(k_fu_tiles, dim3(grid), dim3(kBlock), 0, s, a, tb, blocks);
        });
    }
    if (grid_s) hipLaunchKernelGGL(k_fu_finish, dim3(grid_s), dim3(kBlock), 0, s, a);
    return uvws_call_leave(e, prev, what);
}

int fu_check(uvhttp_ws_gpu_engine_t* e, const FuArgs& a, const char* null_msg, const char* align_msg,
             const char* size_msg) {
    if (!a.desc || !a.verdict || !a.out || (!a.wire && a.wire_len) || (a.streams ? !a.results : !a.bsum))
        return uvws_set_err(e, UVHTTP_WS_GPU_EINVAL, null_msg);
    if (((uintptr_t)a.wire & 15u) || ((uintptr_t)a.desc & 7u) || ((uintptr_t)a.streams & 7u) ||
        ((uintptr_t)a.results & 7u) || ((uintptr_t)a.bsum & 7u) || ((uintptr_t)a.state_in & 3u) ||
        ((uintptr_t)a.verdict & 3u) || ((uintptr_t)a.out & 3u))
        return uvws_set_err(e, UVHTTP_WS_GPU_EINVAL, align_msg);
    if (a.max_frames > (1u << 28) || a.n_streams > (1u << 31))
        return uvws_set_err(e, UVHTTP_WS_GPU_EINVAL, size_msg);
    return UVHTTP_WS_GPU_OK;
}

}  // namespace

extern "C" int uvhttp_ws_gpu_validate_utf8_streams(uvhttp_ws_gpu_engine_t* e, const uint8_t* d_wire, uint64_t wire_len,
                                                   const uvhttp_ws_frame_desc_t* d_desc, uint32_t max_frames,
                                                   const uvhttp_ws_stream_t* d_streams,
                                                   const uvhttp_ws_stream_result_t* d_results, uint32_t n_streams,
                                                   const uvhttp_ws_utf8_state_t* d_state_in, uint32_t flags,
                                                   uvhttp_ws_utf8_conn_verdict_t* d_verdict,
                                                   uvhttp_ws_utf8_frames_summary_t* d_summary, void* stream) {
    if (!e) return UVHTTP_WS_GPU_EINVAL;
    if (!d_streams) return uvws_set_err(e, UVHTTP_WS_GPU_EINVAL, "validate_utf8_streams: NULL argument");
    FuArgs a = {};
    a.wire = d_wire;
    a.wire_len = wire_len;
    a.desc = d_desc;
    a.max_frames = max_frames;
    a.n_streams = n_streams;
    a.streams = d_streams;
    a.results = d_results;
    a.state_in = d_state_in;
    a.flags = flags;
    a.verdict = d_verdict;
    a.out = d_summary;
    const int rc = fu_check(e, a, "validate_utf8_streams: NULL argument", "validate_utf8_streams: misaligned argument",
                            "validate_utf8_streams: max_frames > 2^28 or n_streams > 2^31");
    if (rc != UVHTTP_WS_GPU_OK) return rc;
    return fu_run(e, a, stream, "validate_utf8_streams launch");
}

extern "C" int uvhttp_ws_gpu_validate_utf8_inplace(uvhttp_ws_gpu_engine_t* e, const uint8_t* d_wire, uint64_t wire_len,
                                                   const uvhttp_ws_frame_desc_t* d_desc, uint32_t n_frames,
                                                   const uvhttp_ws_batch_summary_t* d_batch_summary, uint32_t flags,
                                                   uvhttp_ws_utf8_conn_verdict_t* d_verdict,
                                                   uvhttp_ws_utf8_frames_summary_t* d_summary, void* stream) {
    if (!e) return UVHTTP_WS_GPU_EINVAL;
    FuArgs a = {};
    a.wire = d_wire;
    a.wire_len = wire_len;
    a.desc = d_desc;
    a.max_frames = n_frames;
    a.n_streams = 1;
    a.bsum = d_batch_summary;
    a.flags = flags;
    a.verdict = d_verdict;
    a.out = d_summary;
    const int rc = fu_check(e, a, "validate_utf8_inplace: NULL argument", "validate_utf8_inplace: misaligned argument",
                            "validate_utf8_inplace: n_frames > 2^28");
    if (rc != UVHTTP_WS_GPU_OK) return rc;
    return fu_run(e, a, stream, "validate_utf8_inplace launch");
}
