// ws_close_gpu.hip — the server's own CLOSE frames built on the device after a decode
// (include/uvhttp_ws_amd.h: uvhttp_ws_gpu_close_frames_streams): the 1002 close on_websocket_read
// sends when a process_data call fails (src/uvhttp_connection.c:1166-1174 ->
// src/uvhttp_websocket.c:627-666) and the 1007 close the UTF-8 verdicts exist for, for a whole
// decoded batch, laid out as uvhttp_tls_gpu_seal_parts reads a part.  One lane per connection, no
// descriptor and no wire byte read.  Three short passes, scratch in the engine, no waiting between
// workgroups:
//
//   k_cl_size   one lane per connection: its code and frame bytes from its stream, result,
//               verdict and reply result; the workgroup's closes (1002 and 1007) and bytes
//   k_scan_top  both aggregates' inclusive prefixes (two workgroups; ws_scan.h)
//   k_cl_emit   one lane per connection: the same code again, its frame index and byte offset
//               from the scan, then the frame (at most 22 bytes, written by the lane), d_out_off,
//               the run, the cleared runs of a 1007 connection, the 16-byte result; the first
//               connection's lane writes the summary, the last one's the total at the table's end
//
// The size and emit passes go through engine_grid_chunks, tile base in hand.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "uvhttp_ws_amd.h"
#include "ws_engine_int.h"
#include "ws_scan.h"

namespace {

constexpr uint32_t kReasonLen = 14;  // "protocol error"

struct ClArgs {
    const uvhttp_ws_stream_t* streams;
    const uvhttp_ws_stream_result_t* results;
    uint32_t n_streams;
    const uvhttp_ws_utf8_conn_verdict_t* verdict;  // or null
    const uvhttp_ws_reply_conn_t* reply;           // or null
    const uint8_t* enable;                         // or null
    const uint32_t* keys;                          // or null
    uint8_t* out;
    uint64_t out_cap;
    uint64_t* out_off;
    uint32_t* runs;                                // or null
    uint32_t run_stride;
    uint32_t n_clear;
    uint32_t* clear_runs[UVHTTP_WS_CLOSE_MAX_CLEAR];
    uint32_t clear_stride[UVHTTP_WS_CLOSE_MAX_CLEAR];
    uvhttp_ws_close_conn_t* conn;
    uvhttp_ws_close_summary_t* sum;
    // engine scratch
    uint64_t* agg_cnt;    // [blocks] 1002 closes << 32 | 1007 closes, then inclusive
    uint64_t* agg_bytes;  // [blocks] frame bytes, then inclusive
    uint32_t blocks;
};

// connection s: the code it is closed with (0 = none), whether only the key is missing
struct ClConn {
    uint32_t code;
    uint32_t len;  // frame bytes
    bool masked, no_keys;
};

__device__ __forceinline__ ClConn conn_close(const ClArgs& a, uint64_t s) {
    ClConn c = {0, 0, false, false};
    if (s >= a.n_streams) return c;
    if (a.enable && a.enable[s] == 0) return c;
    const int32_t fs = a.results[s].first_status;
    if (call_failed(fs)) return c;
    if (a.reply && a.reply[s].closed) return c;
    uint32_t code = 0;
    if (a.verdict && a.verdict[s].status == UVHTTP_WS_UTF8_INVALID) code = 1007;
    else if (fs < 0) code = 1002;
    if (!code) return c;
    c.masked = a.streams[s].is_server == 0;
    if (c.masked && !a.keys) {
        c.no_keys = true;
        return c;
    }
    c.code = code;
    c.len = 2u + (c.masked ? 4u : 0u) + 2u + (code == 1002 ? kReasonLen : 0u);
    return c;
}

__device__ __forceinline__ uint64_t count_word(const ClConn& c) {
    return c.code == 1002 ? 1ull << 32 : c.code == 1007 ? 1ull : 0ull;
}

__global__ __launch_bounds__(kBlock) void k_cl_size(ClArgs a, uint64_t tb) {
    __shared__ uint64_t s_wave[kWaves];
    const uint64_t b = tb + blockIdx.x;
    const ClConn c = conn_close(a, b * kBlock + threadIdx.x);
    uint64_t tc, tl;
    (void)block_scan(count_word(c), AddOp(), 0, s_wave, &tc);
    (void)block_scan(c.len, AddOp(), 0, s_wave, &tl);
    if (threadIdx.x == 0) {
        a.agg_cnt[b] = tc;
        a.agg_bytes[b] = tl;
    }
}

__global__ __launch_bounds__(kBlock) void k_cl_emit(ClArgs a, uint64_t tb) {
    __shared__ uint64_t s_wave[kWaves];
    const uint64_t b = tb + blockIdx.x;
    const uint64_t s = b * kBlock + threadIdx.x;
    const ClConn c = conn_close(a, s);
    uint64_t tc, tl;
    const uint64_t ic = (b ? a.agg_cnt[b - 1] : 0) + block_scan(count_word(c), AddOp(), 0, s_wave, &tc);  // inclusive
    const uint64_t il = (b ? a.agg_bytes[b - 1] : 0) + block_scan(c.len, AddOp(), 0, s_wave, &tl);
    const uint64_t all_cnt = a.agg_cnt[a.blocks - 1], all_bytes = a.agg_bytes[a.blocks - 1];
    const uint32_t n1002 = (uint32_t)(all_cnt >> 32), n1007 = (uint32_t)all_cnt;
    const bool fits = all_bytes <= a.out_cap;
    if (s >= a.n_streams) return;
    if (s == 0) {
        uvhttp_ws_close_summary_t sm = {};
        sm.out_bytes = all_bytes;
        sm.n_closes = n1002 + n1007;
        sm.n_1002 = n1002;
        sm.n_1007 = n1007;
        sm.status = fits ? UVHTTP_WS_CLOSE_OK : UVHTTP_WS_CLOSE_ERR_CAPACITY;
        *a.sum = sm;
    }
    uvhttp_ws_close_conn_t r = {};
    uint32_t* run = a.runs ? reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(a.runs) + s * a.run_stride) : nullptr;
    if (!fits) {
        r.status = UVHTTP_WS_CLOSE_ERR_CAPACITY;
        a.conn[s] = r;
        a.out_off[s] = 0;
        if (s == a.n_streams - 1) a.out_off[a.n_streams] = 0;
        if (run) run[0] = run[1] = 0;
        return;
    }
    const uint64_t n_all = (uint64_t)n1002 + n1007;
    // the table's tail: entries from the frame count on hold the total; entry j < count is
    // written by the connection whose frame j is
    if (s >= n_all) a.out_off[s] = all_bytes;
    if (s == a.n_streams - 1) a.out_off[a.n_streams] = all_bytes;
    const uint64_t before = (ic >> 32) + (ic & 0xFFFFFFFFull) - (c.code ? 1 : 0);  // closes before s
    if (run) {
        run[0] = (uint32_t)before;
        run[1] = c.code ? 1u : 0u;
    }
    if (c.no_keys) r.status = UVHTTP_WS_CLOSE_NO_KEYS;
    if (c.code) {
        const uint64_t off = il - c.len;
        const uint32_t key = c.masked ? a.keys[s] : 0u;
        const uint32_t hdr = c.masked ? 6u : 2u, plen = c.len - hdr;
        const char reason[kReasonLen + 1] = "protocol error";
        uint8_t* o = a.out + off;
        o[0] = (uint8_t)(0x80u | UVHTTP_WS_OPCODE_CLOSE);
        o[1] = (uint8_t)((c.masked ? 0x80u : 0u) | plen);
        if (c.masked)
            for (uint32_t k = 0; k < 4; ++k) o[2 + k] = (uint8_t)(key >> (8 * k));
        for (uint32_t i = 0; i < plen; ++i) {
            const uint32_t v = i == 0 ? c.code >> 8 : i == 1 ? c.code & 0xFFu : (uint8_t)reason[i - 2];
            o[hdr + i] = (uint8_t)(v ^ (key >> (8 * (i & 3))));
        }
        a.out_off[before] = off;
        r.code = c.code;
        r.out_len = c.len;
        if (c.code == 1007)
            for (uint32_t k = 0; k < a.n_clear; ++k)
                reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(a.clear_runs[k]) + s * a.clear_stride[k])[1] = 0;
    }
    a.conn[s] = r;
}

void cl_carve(Carver& c, ClArgs& a) {
    a.agg_cnt = c.take<uint64_t>(a.blocks);
    a.agg_bytes = c.take<uint64_t>(a.blocks);
}

}  // namespace

extern "C" int uvhttp_ws_gpu_close_frames_streams(
    uvhttp_ws_gpu_engine_t* e, const uvhttp_ws_stream_t* d_streams, const uvhttp_ws_stream_result_t* d_results,
    uint32_t n_streams, const uvhttp_ws_utf8_conn_verdict_t* d_verdict, const uvhttp_ws_reply_conn_t* d_reply_conn,
    const uint8_t* d_enable, const uint32_t* d_mask_keys, uint32_t flags, uint8_t* d_out, uint64_t out_cap,
    uint64_t* d_out_off, uint32_t* d_runs, uint32_t run_stride, uint32_t* const* d_clear_runs,
    const uint32_t* clear_stride, uint32_t n_clear, uvhttp_ws_close_conn_t* d_conn,
    uvhttp_ws_close_summary_t* d_summary, void* stream) {
    static_assert(sizeof(uvhttp_ws_close_conn_t) == 16 && sizeof(uvhttp_ws_close_summary_t) == 32, "ABI");
    if (!e) return UVHTTP_WS_GPU_EINVAL;
    if (!d_streams || !d_results || !d_out_off || !d_conn || !d_summary || (!d_out && out_cap) ||
        (n_clear && (!d_clear_runs || !clear_stride)))
        return uvws_set_err(e, UVHTTP_WS_GPU_EINVAL, "close_frames_streams: NULL argument");
    if (((uintptr_t)d_streams & 7u) || ((uintptr_t)d_results & 7u) || ((uintptr_t)d_out_off & 7u) ||
        ((uintptr_t)d_summary & 7u) || ((uintptr_t)d_verdict & 3u) || ((uintptr_t)d_reply_conn & 3u) ||
        ((uintptr_t)d_mask_keys & 3u) || ((uintptr_t)d_runs & 3u) || ((uintptr_t)d_conn & 3u))
        return uvws_set_err(e, UVHTTP_WS_GPU_EINVAL, "close_frames_streams: misaligned argument");
    if (n_streams > (1u << 31) || flags != 0 || n_clear > UVHTTP_WS_CLOSE_MAX_CLEAR ||
        (d_runs && (run_stride < 8 || (run_stride & 3u))))
        return uvws_set_err(e, UVHTTP_WS_GPU_EINVAL,
                            "close_frames_streams: n_streams > 2^31, flags, n_clear > 4 or a bad run_stride");
    ClArgs a = {};
    for (uint32_t k = 0; k < n_clear; ++k) {
        if (!d_clear_runs[k] || ((uintptr_t)d_clear_runs[k] & 3u) || clear_stride[k] < 8 || (clear_stride[k] & 3u))
            return uvws_set_err(e, UVHTTP_WS_GPU_EINVAL, "close_frames_streams: a bad clear table or stride");
        a.clear_runs[k] = d_clear_runs[k];
        a.clear_stride[k] = clear_stride[k];
    }
    a.streams = d_streams;
    a.results = d_results;
    a.n_streams = n_streams;
    a.verdict = d_verdict;
    a.reply = d_reply_conn;
    a.enable = d_enable;
    a.keys = d_mask_keys;
    a.out = d_out;
    a.out_cap = out_cap;
    a.out_off = d_out_off;
    a.runs = d_runs;
    a.run_stride = run_stride;
    a.n_clear = n_clear;
    a.conn = d_conn;
    a.sum = d_summary;
    const uint64_t blocks = ((uint64_t)n_streams + kBlock - 1) / kBlock;
    a.blocks = (uint32_t)blocks;

    hipStream_t s = (hipStream_t)stream;
    const int prev = uvws_call_enter(e, s);
    if (!n_streams) {  // no connection: an empty table and a zeroed summary
        (void)hipMemsetAsync(d_summary, 0, sizeof(*d_summary), s);
        (void)hipMemsetAsync(d_out_off, 0, sizeof(uint64_t), s);
        return uvws_call_leave(e, prev, "close_frames_streams launch");
    }
    Carver count{nullptr};
    cl_carve(count, a);
    char* mem = static_cast<char*>(uvws_close_scratch(e, count.bytes(), s));
    if (!mem) {
        (void)uvws_call_leave(e, prev, "close_frames_streams launch");
        return uvws_set_err(e, UVHTTP_WS_GPU_ENOMEM, "close_frames scratch (a captured call must not grow it)");
    }
    Carver carve{mem};
    cl_carve(carve, a);
    engine_grid_chunks(e, blocks, [&](uint32_t grid, uint64_t tb) {
        hipLaunchKernelGGL(k_cl_size, dim3(grid), dim3(kBlock), 0, s, a, tb);
    });
    hipLaunchKernelGGL((k_scan_top<AddOp>), dim3(2), dim3(kBlock), 0, s, a.agg_cnt, a.agg_bytes, a.blocks);
    engine_grid_chunks(e, blocks, [&](uint32_t grid, uint64_t tb) {
        hipLaunchKernelGGL(k_cl_emit, dim3(grid), dim3(kBlock), 0, s, a, tb);
    });
    return uvws_call_leave(e, prev, "close_frames_streams launch");
}
