// ws_replies_gpu.hip — PONG and CLOSE-echo frames built on the device after a decode
// (include/uvhttp_ws_amd.h: uvhttp_ws_gpu_control_replies_streams / _inplace): the reply half of
// uvhttp_ws_process_data (src/uvhttp_websocket.c:1016-1084) for a whole decoded batch, laid out as
// uvhttp_tls_gpu_seal_frames reads it.  Twelve short launches, scratch in the engine, no waiting
// between workgroups and no epoch tags:
//
//   k_rp_init      marks[f] = 0 per descriptor; the summary zeroed
//   k_rp_conns     one lane per connection: its scratch words, and a head mark (connection + 1)
//                  at its first delivered descriptor
//   k_mark_reduce  one lane per descriptor: the workgroup's last head mark (ws_scan.h)
//   k_scan_top     one workgroup: the aggregates' inclusive prefixes (ws_scan.h)
//   k_rp_classify  one lane per descriptor, 32 bytes read each: its connection from the scan of
//                  the marks (the last head at or before it); inside the connection's delivered
//                  range it writes a word — the connection, first / last frame of the range, and
//                  for a delivered PING / CLOSE the reply's opcode, payload length and masking —
//                  else 0.  A CLOSE lowers first_close[connection] (atomicMin); a reply payload
//                  outside the wire sets bad[connection].  Only the descriptor is read, no payload
//   k_rp_size      one lane per descriptor, 8 bytes read: a candidate is answered when its
//                  connection is not bad and it is not after the connection's first CLOSE (or the
//                  flag says to go on); the workgroup's replies and bytes
//   k_scan_top     both aggregates (two workgroups)
//   k_rp_emit      one lane per descriptor, 8 bytes read: reply index and byte offset from the
//                  scan; the running totals before a connection's first frame and after its last
//                  (its replies and bytes are their difference: no atomics, in place every frame
//                  shares one connection); d_out_off[j]; and the frame bytes, written by the whole
//                  wave for one answered lane after another: 64 byte stores side by side per round,
//                  at most three rounds per reply, at whatever alignment the offset has.  So the
//                  payload is touched only for replies and the emit costs by the reply
//   k_rp_tail      d_out_off[n_replies .. max_replies] = the total (all 0 on capacity)
//   k_rp_creduce / k_scan_top / k_rp_finish  one lane per connection: first_reply as the
//                  exclusive sum of the connections' replies, the 16-byte result, the run, the
//                  summary
//
// Descriptors after a connection's delivered frames may hold anything: they lie outside every
// range, so their word is 0.  A table whose connections' ranges overlap gets unspecified replies,
// but nothing outside the wire, the descriptors below max_frames, the n_streams entries, d_out
// below out_cap and d_out_off up to max_replies is read or written: the capacity test uses the
// totals the emit itself goes by.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "uvhttp_ws_amd.h"
#include "ws_engine_int.h"
#include "ws_scan.h"

namespace {

// the word per descriptor (elem): bits 0-6 the reply's payload length, then
constexpr uint64_t kLenMask = 0x7F;
constexpr uint64_t kCand = 1ull << 8;    // a delivered PING / CLOSE of an enabled connection
constexpr uint64_t kClose = 1ull << 9;   // ... a CLOSE (the reply is a CLOSE, else a PONG)
constexpr uint64_t kMasked = 1ull << 10; // a client connection: key + masked payload
constexpr uint64_t kAns = 1ull << 11;    // answered (k_rp_size)
constexpr uint64_t kIn = 1ull << 12;     // inside its connection's delivered range
constexpr uint64_t kFirst = 1ull << 13;  // the range's first frame
constexpr uint64_t kLast = 1ull << 14;   // the range's last frame
// bits 32-63: the connection

struct RpArgs {
    const uint8_t* wire;
    uint64_t wire_len;
    const uvhttp_ws_frame_desc_t* desc;
    uint32_t max_frames;
    uint32_t n_streams;
    const uvhttp_ws_stream_t* streams;           // null: the in-place form (one connection)
    const uvhttp_ws_stream_result_t* results;
    const uvhttp_ws_batch_summary_t* bsum;       // the in-place form's n_delivered
    int32_t is_server;                           // the in-place form's
    const uint8_t* enable;                       // or null
    const uint32_t* keys;                        // or null
    uint32_t flags;
    uint8_t* out;
    uint64_t out_cap;
    uint64_t* out_off;
    uint32_t max_replies;
    uint32_t* runs;                              // or null
    uint32_t run_stride;                         // bytes
    uvhttp_ws_reply_conn_t* conn;
    uvhttp_ws_reply_summary_t* sum;
    // engine scratch
    uint32_t* marks;        // [max_frames] connection + 1 at its first delivered descriptor
    uint64_t* elem;         // [max_frames] the word above
    uint64_t* agg_mark;     // [blocks] last head mark, then inclusive
    uint64_t* agg_cnt;      // [blocks] replies, then inclusive
    uint64_t* agg_bytes;    // [blocks] reply bytes, then inclusive
    uint64_t* agg_conn;     // [connection blocks] replies, then inclusive
    const uint64_t* tot_cnt;   // &agg_cnt[blocks - 1], null when there is no descriptor
    const uint64_t* tot_bytes;
    uint32_t* first_close;  // [n_streams] the connection's first delivered CLOSE, kNone if none
    uint32_t* bad;          // [n_streams] a reply payload outside the wire
    uint32_t* cbeg;         // [n_streams] replies before the connection's first frame ...
    uint32_t* cend;         // ... and up to its last
    uint64_t* bbeg;         // the same in bytes
    uint64_t* bend;
};

// connection s's considered descriptors, inside [0, max_frames)
__device__ __forceinline__ Range conn_range(const RpArgs& a, uint32_t s) {
    Range r;
    if (!a.results) {
        r.ff = 0;
        r.nd = a.bsum->n_delivered;
    } else {
        const uvhttp_ws_stream_result_t& q = a.results[s];
        r.ff = q.first_frame;
        r.nd = q.n_delivered;
        if (call_failed(q.first_status)) r.nd = 0;
    }
    return clamp_range(r, a.max_frames);
}

__device__ __forceinline__ bool conn_enabled(const RpArgs& a, uint32_t s) { return !a.enable || a.enable[s] != 0; }
__device__ __forceinline__ bool conn_server(const RpArgs& a, uint32_t s) {
    return a.streams ? a.streams[s].is_server != 0 : a.is_server != 0;
}

__global__ __launch_bounds__(kBlock) void k_rp_init(RpArgs a) {
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i == 0) {
        uvhttp_ws_reply_summary_t z = {};
        *a.sum = z;
    }
    if (i < a.max_frames) a.marks[i] = 0;
}

__global__ __launch_bounds__(kBlock) void k_rp_conns(RpArgs a) {
    const uint64_t s = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (s >= a.n_streams) return;
    a.first_close[s] = kNone;
    a.bad[s] = 0;
    a.cbeg[s] = 0;
    a.cend[s] = 0;
    a.bbeg[s] = 0;
    a.bend[s] = 0;
    const Range r = conn_range(a, (uint32_t)s);
    if (r.nd) a.marks[r.ff] = (uint32_t)s + 1;
}

__global__ __launch_bounds__(kBlock) void k_rp_classify(RpArgs a) {
    __shared__ uint64_t s_wave[kWaves];
    const uint64_t f = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    const bool live = f < a.max_frames;
    const uint64_t head = head_mark(a.marks, a.max_frames, a.agg_mark, blockIdx.x, s_wave);
    if (!live) return;
    uint64_t e = 0;
    if (head != 0 && head - 1 < a.n_streams) {
        const uint32_t conn = (uint32_t)(head - 1);
        const Range r = conn_range(a, conn);
        if (f >= r.ff && f - r.ff < r.nd) {
            e = kIn | ((uint64_t)conn << 32) | (f == r.ff ? kFirst : 0) | (f - r.ff == r.nd - 1 ? kLast : 0);
            const uvhttp_ws_frame_desc_t& d = a.desc[f];
            const uint32_t op = d.opcode;
            if (d.status == UVHTTP_WS_FRAME_OK && (op == UVHTTP_WS_OPCODE_PING || op == UVHTTP_WS_OPCODE_CLOSE)) {
                if (op == UVHTTP_WS_OPCODE_CLOSE) atomicMin(&a.first_close[conn], (uint32_t)f);
                const bool srv = conn_server(a, conn);
                if (conn_enabled(a, conn) && (srv || a.keys)) {
                    uint64_t len = d.payload_len;
                    if (op == UVHTTP_WS_OPCODE_CLOSE && len < 2) len = 0;
                    if (len > 125) len = 125;  // a delivered control frame has at most 125 bytes
                    if (len != 0 && !range_ok(a.wire_len, d.payload_off, len)) a.bad[conn] = 1;
                    else e |= kCand | (op == UVHTTP_WS_OPCODE_CLOSE ? kClose : 0) | (srv ? 0 : kMasked) | len;
                }
            }
        }
    }
    a.elem[f] = e;
}

__device__ __forceinline__ uint32_t reply_bytes(uint64_t e) {
    return (e & kAns) ? 2u + ((e & kMasked) ? 4u : 0u) + (uint32_t)(e & kLenMask) : 0u;
}

__global__ __launch_bounds__(kBlock) void k_rp_size(RpArgs a) {
    __shared__ uint64_t s_wave[kWaves];
    const uint64_t f = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    uint64_t e = f < a.max_frames ? a.elem[f] : 0;
    if (e & kCand) {
        const uint32_t conn = (uint32_t)(e >> 32);
        const bool ans = a.bad[conn] == 0 &&
                         ((a.flags & UVHTTP_WS_REPLY_AFTER_CLOSE) || (uint32_t)f <= a.first_close[conn]);
        if (ans) {
            e |= kAns;
            a.elem[f] = e;
        }
    }
    // replies << 32 | bytes: a workgroup holds at most 256 replies of at most 131 bytes
    uint64_t tot;
    (void)block_scan(((e & kAns) ? 1ull << 32 : 0ull) | reply_bytes(e), AddOp(), 0, s_wave, &tot);
    if (threadIdx.x == 0) {
        a.agg_cnt[blockIdx.x] = tot >> 32;
        a.agg_bytes[blockIdx.x] = tot & 0xFFFFFFFFull;
    }
}

__global__ __launch_bounds__(kBlock) void k_rp_emit(RpArgs a) {
    __shared__ uint64_t s_wave[kWaves];
    const int lane = threadIdx.x & 63;
    const uint64_t f = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    const uint64_t e = f < a.max_frames ? a.elem[f] : 0;
    const uint32_t mine = reply_bytes(e);
    const bool ans = (e & kAns) != 0;
    uint64_t tot;
    const uint64_t inc = block_scan((ans ? 1ull << 32 : 0ull) | mine, AddOp(), 0, s_wave, &tot);
    const uint64_t cnt = (blockIdx.x ? a.agg_cnt[blockIdx.x - 1] : 0) + (inc >> 32);       // inclusive
    const uint64_t bytes = (blockIdx.x ? a.agg_bytes[blockIdx.x - 1] : 0) + (inc & 0xFFFFFFFFull);
    if (e & kIn) {
        const uint32_t conn = (uint32_t)(e >> 32);
        if (e & kFirst) {
            a.cbeg[conn] = (uint32_t)(cnt - (ans ? 1 : 0));
            a.bbeg[conn] = bytes - mine;
        }
        if (e & kLast) {
            a.cend[conn] = (uint32_t)cnt;
            a.bend[conn] = bytes;
        }
    }
    const bool fits = *a.tot_cnt <= a.max_replies && *a.tot_bytes <= a.out_cap;
    if (!fits) return;  // the same in every lane

    const uint64_t j = cnt - 1, off = bytes - mine;  // an answered lane's slot and start
    uint64_t poff = 0;
    uint32_t key = 0;
    if (ans) {
        a.out_off[j] = off;
        poff = a.desc[f].payload_off;
        if (e & kMasked) key = a.keys[j];
    }
    // the wave writes one reply after another: lane i byte i, i + 64, i + 128
    uint64_t todo = __ballot(ans);
    while (todo) {
        const int src = __ffsll((unsigned long long)todo) - 1;
        todo &= todo - 1;
        const uint64_t se = __shfl(e, src), so = __shfl(off, src), sp = __shfl(poff, src);
        const uint32_t sk = __shfl(key, src);
        const uint32_t len = (uint32_t)(se & kLenMask), hdr = (se & kMasked) ? 6u : 2u;
        const uint32_t total = hdr + len;
        for (uint32_t i = lane; i < total; i += 64) {
            uint32_t b;
            if (i == 0) b = 0x80u | ((se & kClose) ? UVHTTP_WS_OPCODE_CLOSE : UVHTTP_WS_OPCODE_PONG);
            else if (i == 1) b = ((se & kMasked) ? 0x80u : 0u) | len;
            else if (i < hdr) b = sk >> (8 * (i - 2));
            else b = a.wire[sp + (i - hdr)] ^ (sk >> (8 * ((i - hdr) & 3)));
            a.out[so + i] = (uint8_t)b;
        }
    }
}

__global__ __launch_bounds__(kBlock) void k_rp_tail(RpArgs a) {
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i > a.max_replies) return;
    const uint64_t n = a.tot_cnt ? *a.tot_cnt : 0, bytes = a.tot_bytes ? *a.tot_bytes : 0;
    if (n > a.max_replies || bytes > a.out_cap) a.out_off[i] = 0;
    else if (i >= n) a.out_off[i] = bytes;
}

__global__ __launch_bounds__(kBlock) void k_rp_creduce(RpArgs a) {
    __shared__ uint64_t s_wave[kWaves];
    const uint64_t s = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    const uint64_t n = s < a.n_streams ? a.cend[s] - a.cbeg[s] : 0;
    uint64_t tot;
    (void)block_scan(n, AddOp(), 0, s_wave, &tot);
    if (threadIdx.x == 0) a.agg_conn[blockIdx.x] = tot;
}

__global__ __launch_bounds__(kBlock) void k_rp_finish(RpArgs a) {
    __shared__ uint64_t s_wave[kWaves];
    const uint64_t s = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    const bool live = s < a.n_streams;
    const uint32_t n = live ? a.cend[s] - a.cbeg[s] : 0;
    uint64_t tot;
    const uint64_t inc = (blockIdx.x ? a.agg_conn[blockIdx.x - 1] : 0) + block_scan(n, AddOp(), 0, s_wave, &tot);
    const uint64_t tn = a.tot_cnt ? *a.tot_cnt : 0, tb = a.tot_bytes ? *a.tot_bytes : 0;
    const bool fits = tn <= a.max_replies && tb <= a.out_cap;
    bool closed = false;
    if (live) {
        closed = a.first_close[s] != kNone;
        uvhttp_ws_reply_conn_t r = {};
        r.closed = closed ? 1 : 0;
        if (!fits) {
            r.status = UVHTTP_WS_REPLY_ERR_CAPACITY;
        } else {
            const uint64_t len = a.bend[s] - a.bbeg[s];
            r.first_reply = (uint32_t)(inc - n);
            r.n_replies = n;
            r.out_len = len > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)len;
            if (conn_enabled(a, (uint32_t)s) && !conn_server(a, (uint32_t)s) && !a.keys) r.status = UVHTTP_WS_REPLY_NO_KEYS;
            else if (a.bad[s]) r.status = UVHTTP_WS_REPLY_BAD_RANGE;
        }
        a.conn[s] = r;
        if (a.runs) {
            uint32_t* run = reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(a.runs) + s * a.run_stride);
            run[0] = r.first_reply;
            run[1] = r.n_replies;
        }
    }
    const uint64_t mc = __ballot(closed);
    if ((threadIdx.x & 63) == 0 && mc) atomicAdd(&a.sum->n_closed_conns, (uint32_t)__popcll(mc));
    if (s == 0) {
        a.sum->out_bytes = tb;
        a.sum->n_replies = (uint32_t)tn;
        a.sum->status = fits ? UVHTTP_WS_REPLY_OK : UVHTTP_WS_REPLY_ERR_CAPACITY;
    }
}

void rp_carve(Carver& c, RpArgs& a, uint64_t nb, uint64_t ns) {
    const uint64_t F = a.max_frames, S = a.n_streams;
    a.elem = c.take<uint64_t>(F);
    a.agg_mark = c.take<uint64_t>(nb);
    a.agg_cnt = c.take<uint64_t>(nb);
    a.agg_bytes = c.take<uint64_t>(nb);
    a.agg_conn = c.take<uint64_t>(ns);
    a.bbeg = c.take<uint64_t>(S);
    a.bend = c.take<uint64_t>(S);
    a.marks = c.take<uint32_t>(F);
    a.first_close = c.take<uint32_t>(S);
    a.bad = c.take<uint32_t>(S);
    a.cbeg = c.take<uint32_t>(S);
    a.cend = c.take<uint32_t>(S);
}

int rp_run(uvhttp_ws_gpu_engine_t* e, RpArgs a, void* stream, const char* what) {
    static_assert(sizeof(uvhttp_ws_reply_conn_t) == 16 && sizeof(uvhttp_ws_reply_summary_t) == 32, "ABI");
    const uint32_t blocks = (uint32_t)(((uint64_t)a.max_frames + kBlock - 1) / kBlock);
    const uint32_t grid_s = (uint32_t)(((uint64_t)a.n_streams + kBlock - 1) / kBlock);
    const uint64_t nb = blocks ? blocks : 1, ns = grid_s ? grid_s : 1;
    Carver count{nullptr};
    rp_carve(count, a, nb, ns);

    hipStream_t s = (hipStream_t)stream;
    const int prev = uvws_call_enter(e, s);
    char* mem = static_cast<char*>(uvws_replies_scratch(e, count.bytes(), s));
    if (!mem) {
        (void)uvws_call_leave(e, prev, what);
        return uvws_set_err(e, UVHTTP_WS_GPU_ENOMEM, "control_replies scratch (a captured call must not grow it)");
    }
    Carver carve{mem};
    rp_carve(carve, a, nb, ns);
    const bool frames = blocks && grid_s;  // else no reply: the totals are 0
    a.tot_cnt = frames ? a.agg_cnt + (blocks - 1) : nullptr;
    a.tot_bytes = frames ? a.agg_bytes + (blocks - 1) : nullptr;

    hipLaunchKernelGGL(k_rp_init, dim3(blocks ? blocks : 1), dim3(kBlock), 0, s, a);
    if (grid_s) hipLaunchKernelGGL(k_rp_conns, dim3(grid_s), dim3(kBlock), 0, s, a);
    if (frames) {
        hipLaunchKernelGGL((k_mark_reduce<>), dim3(blocks), dim3(kBlock), 0, s, a.marks, a.max_frames, a.agg_mark, (uint64_t)0);
        hipLaunchKernelGGL((k_scan_top<LastOp>), dim3(1), dim3(kBlock), 0, s, a.agg_mark, a.agg_mark, blocks);
        hipLaunchKernelGGL(k_rp_classify, dim3(blocks), dim3(kBlock), 0, s, a);
        hipLaunchKernelGGL(k_rp_size, dim3(blocks), dim3(kBlock), 0, s, a);
        hipLaunchKernelGGL((k_scan_top<AddOp>), dim3(2), dim3(kBlock), 0, s, a.agg_cnt, a.agg_bytes, blocks);
        hipLaunchKernelGGL(k_rp_emit, dim3(blocks), dim3(kBlock), 0, s, a);
    }
    const uint32_t grid_t = (uint32_t)(((uint64_t)a.max_replies + 1 + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(k_rp_tail, dim3(grid_t), dim3(kBlock), 0, s, a);
    if (grid_s) {
        hipLaunchKernelGGL(k_rp_creduce, dim3(grid_s), dim3(kBlock), 0, s, a);
        hipLaunchKernelGGL((k_scan_top<AddOp>), dim3(1), dim3(kBlock), 0, s, a.agg_conn, a.agg_conn, grid_s);
        hipLaunchKernelGGL(k_rp_finish, dim3(grid_s), dim3(kBlock), 0, s, a);
    }
    return uvws_call_leave(e, prev, what);
}

int rp_check(uvhttp_ws_gpu_engine_t* e, const RpArgs& a, const char* null_msg, const char* align_msg,
             const char* size_msg) {
    if (!a.desc || !a.out_off || !a.conn || !a.sum || (!a.wire && a.wire_len) || (!a.out && a.out_cap) ||
        (a.streams ? !a.results : !a.bsum))
        return uvws_set_err(e, UVHTTP_WS_GPU_EINVAL, null_msg);
    if (((uintptr_t)a.wire & 15u) || ((uintptr_t)a.desc & 7u) || ((uintptr_t)a.streams & 7u) ||
        ((uintptr_t)a.results & 7u) || ((uintptr_t)a.bsum & 7u) || ((uintptr_t)a.out_off & 7u) ||
        ((uintptr_t)a.keys & 3u) || ((uintptr_t)a.runs & 3u) || ((uintptr_t)a.conn & 3u) || ((uintptr_t)a.sum & 7u))
        return uvws_set_err(e, UVHTTP_WS_GPU_EINVAL, align_msg);
    if (a.max_frames > (1u << 28) || a.max_replies > (1u << 28) || a.n_streams > (1u << 31) ||
        (a.runs && (a.run_stride < 8 || (a.run_stride & 3u))))
        return uvws_set_err(e, UVHTTP_WS_GPU_EINVAL, size_msg);
    return UVHTTP_WS_GPU_OK;
}

}  // namespace

extern "C" int uvhttp_ws_gpu_control_replies_streams(
    uvhttp_ws_gpu_engine_t* e, const uint8_t* d_wire, uint64_t wire_len, const uvhttp_ws_frame_desc_t* d_desc,
    uint32_t max_frames, const uvhttp_ws_stream_t* d_streams, const uvhttp_ws_stream_result_t* d_results,
    uint32_t n_streams, const uint8_t* d_enable, const uint32_t* d_mask_keys, uint32_t flags, uint8_t* d_out,
    uint64_t out_cap, uint64_t* d_out_off, uint32_t max_replies, uint32_t* d_runs, uint32_t run_stride,
    uvhttp_ws_reply_conn_t* d_conn, uvhttp_ws_reply_summary_t* d_summary, void* stream) {
    if (!e) return UVHTTP_WS_GPU_EINVAL;
    if (!d_streams) return uvws_set_err(e, UVHTTP_WS_GPU_EINVAL, "control_replies_streams: NULL argument");
    RpArgs a = {};
    a.wire = d_wire;
    a.wire_len = wire_len;
    a.desc = d_desc;
    a.max_frames = max_frames;
    a.n_streams = n_streams;
    a.streams = d_streams;
    a.results = d_results;
    a.enable = d_enable;
    a.keys = d_mask_keys;
    a.flags = flags;
    a.out = d_out;
    a.out_cap = out_cap;
    a.out_off = d_out_off;
    a.max_replies = max_replies;
    a.runs = d_runs;
    a.run_stride = run_stride;
    a.conn = d_conn;
    a.sum = d_summary;
    const int rc = rp_check(e, a, "control_replies_streams: NULL argument", "control_replies_streams: misaligned argument",
                            "control_replies_streams: max_frames or max_replies > 2^28, n_streams > 2^31 or a bad run_stride");
    if (rc != UVHTTP_WS_GPU_OK) return rc;
    return rp_run(e, a, stream, "control_replies_streams launch");
}

extern "C" int uvhttp_ws_gpu_control_replies_inplace(
    uvhttp_ws_gpu_engine_t* e, const uint8_t* d_wire, uint64_t wire_len, const uvhttp_ws_frame_desc_t* d_desc,
    uint32_t n_frames, const uvhttp_ws_batch_summary_t* d_batch_summary, int32_t is_server,
    const uint32_t* d_mask_keys, uint32_t flags, uint8_t* d_out, uint64_t out_cap, uint64_t* d_out_off,
    uint32_t max_replies, uint32_t* d_runs, uint32_t run_stride, uvhttp_ws_reply_conn_t* d_conn,
    uvhttp_ws_reply_summary_t* d_summary, void* stream) {
    if (!e) return UVHTTP_WS_GPU_EINVAL;
    RpArgs a = {};
    a.wire = d_wire;
    a.wire_len = wire_len;
    a.desc = d_desc;
    a.max_frames = n_frames;
    a.n_streams = 1;
    a.bsum = d_batch_summary;
    a.is_server = is_server;
    a.keys = d_mask_keys;
    a.flags = flags;
    a.out = d_out;
    a.out_cap = out_cap;
    a.out_off = d_out_off;
    a.max_replies = max_replies;
    a.runs = d_runs;
    a.run_stride = run_stride;
    a.conn = d_conn;
    a.sum = d_summary;
    const int rc = rp_check(e, a, "control_replies_inplace: NULL argument", "control_replies_inplace: misaligned argument",
                            "control_replies_inplace: n_frames or max_replies > 2^28 or a bad run_stride");
    if (rc != UVHTTP_WS_GPU_OK) return rc;
    return rp_run(e, a, stream, "control_replies_inplace launch");
}
