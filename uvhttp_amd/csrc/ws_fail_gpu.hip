// ws_fail_gpu.hip — fail points found on the device after a decode and its UTF-8 verdicts
// (include/uvhttp_ws_amd.h: uvhttp_ws_gpu_fail_points_streams): the frame at which a server that
// follows RFC 6455 §7.1.7 fails each connection, and the two outcome tables rewritten into what
// that server would have seen, so that the echo, relay, reply and close passes run unchanged on
// them.  A descriptor pass like the replies' scan.  Six short launches, scratch in the engine, no
// waiting between workgroups:
//
//   k_fp_init      marks[f] = 0 per descriptor; the summary zeroed
//   k_fp_conns     one lane per connection: first_close = none, and a head mark (connection + 1)
//                  at the first considered descriptor of a judged connection
//   k_mark_reduce  one lane per descriptor: the workgroup's last head mark (ws_scan.h)
//   k_scan_top     one workgroup: the aggregates' inclusive prefixes (ws_scan.h)
//   k_fp_classify  one lane per descriptor, 32 bytes read each: its connection from the scan of
//                  the marks (the last head at or before it); a CLOSE with status OK inside the
//                  connection's considered range lowers first_close[connection] (atomicMin)
//   k_fp_judge     one lane per connection: its result, verdict and first CLOSE (that frame's
//                  descriptor and 2 wire bytes when the CLOSE is judged) -> the rewritten result
//                  and verdict and the 16-byte fail entry; the wave's counts go to the summary
//                  (one atomic per wave and counter that is not zero)
//
// The chunked launches go through engine_grid_chunks, tile base in hand.  Descriptors outside every
// considered range are read but change nothing.  A table whose connections' ranges overlap gets
// unspecified fail points, but nothing outside the wire, the descriptors below max_frames and the
// n_streams entries is read or written.  In place (d_results_out == d_results, d_verdict_out ==
// d_verdict) only k_fp_judge writes the tables, every lane its own entry after reading it.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "uvhttp_ws_amd.h"
#include "ws_engine_int.h"
#include "ws_scan.h"

namespace {

struct FpArgs {
    const uint8_t* wire;
    uint64_t wire_len;
    const uvhttp_ws_frame_desc_t* desc;
    uint32_t max_frames;
    uint32_t n_streams;
    const uvhttp_ws_stream_result_t* results;
    const uvhttp_ws_utf8_conn_verdict_t* verdict;  // or null
    const uint8_t* enable;                         // or null
    uint32_t flags;
    uvhttp_ws_stream_result_t* results_out;
    uvhttp_ws_utf8_conn_verdict_t* verdict_out;    // null with verdict
    uvhttp_ws_fail_conn_t* fail;
    uvhttp_ws_fail_summary_t* sum;
    // engine scratch
    uint32_t* marks;        // [max_frames] connection + 1 at its first considered descriptor
    uint64_t* agg_mark;     // [blocks] last head mark, then inclusive
    uint32_t* first_close;  // [n_streams] the connection's first considered CLOSE, kNone if none
};

// connection s's considered descriptors, inside [0, max_frames); none when the connection is not
// judged: the call failed, or (this call alone) the connection is not enabled
__device__ __forceinline__ Range conn_range(const FpArgs& a, uint32_t s) {
    const uvhttp_ws_stream_result_t& q = a.results[s];
    Range r = {q.first_frame, q.n_delivered};
    if (call_failed(q.first_status) || (a.enable && a.enable[s] == 0)) r.nd = 0;
    return clamp_range(r, a.max_frames);
}

__device__ __forceinline__ bool code_valid(uint32_t c) {
    return (c >= 1000 && c <= 1003) || (c >= 1007 && c <= 1014) || (c >= 3000 && c <= 4999);
}

__global__ __launch_bounds__(kBlock) void k_fp_init(FpArgs a, uint64_t tb) {
    const uint64_t i = (tb + blockIdx.x) * kBlock + threadIdx.x;
    if (i == 0) {
        uvhttp_ws_fail_summary_t z = {};
        z.first_failed = kNone;
        *a.sum = z;
    }
    if (i < a.max_frames) a.marks[i] = 0;
}

__global__ __launch_bounds__(kBlock) void k_fp_conns(FpArgs a, uint64_t tb) {
    const uint64_t s = (tb + blockIdx.x) * kBlock + threadIdx.x;
    if (s >= a.n_streams) return;
    a.first_close[s] = kNone;
    const Range r = conn_range(a, (uint32_t)s);
    if (r.nd) a.marks[r.ff] = (uint32_t)s + 1;
}

__global__ __launch_bounds__(kBlock) void k_fp_classify(FpArgs a, uint64_t tb) {
    __shared__ uint64_t s_wave[kWaves];
    const uint64_t b = tb + blockIdx.x;
    const uint64_t f = b * kBlock + threadIdx.x;
    const bool live = f < a.max_frames;
    const uint64_t head = head_mark(a.marks, a.max_frames, a.agg_mark, b, s_wave);
    if (!live || head == 0 || head - 1 >= a.n_streams) return;
    const uvhttp_ws_frame_desc_t& d = a.desc[f];
    if (d.opcode != UVHTTP_WS_OPCODE_CLOSE || d.status != UVHTTP_WS_FRAME_OK) return;
    const uint32_t conn = (uint32_t)(head - 1);
    const Range r = conn_range(a, conn);
    if (f >= r.ff && f - r.ff < r.nd) atomicMin(&a.first_close[conn], (uint32_t)f);
}

__global__ __launch_bounds__(kBlock) void k_fp_judge(FpArgs a, uint64_t tb) {
    const uint64_t s = (tb + blockIdx.x) * kBlock + threadIdx.x;
    const bool live = s < a.n_streams;
    uint32_t reason = UVHTTP_WS_FAIL_NONE, dropped = 0;
    bool bad = false;
    if (live) {
        uvhttp_ws_stream_result_t r = a.results[s];  // read whole before the write: in place
        uvhttp_ws_utf8_conn_verdict_t v = {};
        if (a.verdict) v = a.verdict[s];
        uvhttp_ws_fail_conn_t fl = {};
        fl.frame = kNone;
        const int32_t fs = r.first_status;
        const bool judged = !call_failed(fs) && !(a.enable && a.enable[s] == 0);
        if (judged) {
            const Range in = clamp_range({r.first_frame, r.n_delivered}, a.max_frames);
            const uint32_t ff = in.ff, nd = in.nd;
            const uint32_t c = nd ? a.first_close[s] : kNone;  // (no mark, no CLOSE found)
            uint32_t k = kNone;
            if ((a.flags & UVHTTP_WS_FAIL_CHECK_CLOSE) && c != kNone) {
                const uint64_t len = a.desc[c].payload_len, off = a.desc[c].payload_off;
                if (len == 1) {
                    reason = UVHTTP_WS_FAIL_CLOSE_LEN;
                } else if (len >= 2) {
                    if (len > a.wire_len || off > a.wire_len - len) bad = true;
                    else if (!code_valid((uint32_t)a.wire[off] << 8 | a.wire[off + 1])) reason = UVHTTP_WS_FAIL_CLOSE_CODE;
                }
                if (reason != UVHTTP_WS_FAIL_NONE) k = c;
            }
            if (bad) {
                fl.status = UVHTTP_WS_FAIL_BAD_RANGE;
            } else {
                const uint32_t u = v.first_invalid;
                const bool close_cut = k != kNone;
                if (a.verdict && v.status == UVHTTP_WS_UTF8_INVALID && u >= ff && u - ff < nd && (c == kNone || u <= c) &&
                    (k == kNone || u < k)) {
                    k = u;
                    reason = UVHTTP_WS_FAIL_UTF8;
                }
                if (k != kNone) {
                    dropped = nd - (k - ff);
                    fl.frame = k;
                    fl.n_dropped = dropped;
                    fl.code = reason == UVHTTP_WS_FAIL_UTF8 ? 1007 : 1002;
                    r.n_delivered = k - ff;
                    r.n_frames = r.n_delivered + 1;
                    r.status = UVHTTP_ERROR_INVALID_PARAM;
                    r.first_status = reason == UVHTTP_WS_FAIL_UTF8 ? UVHTTP_WS_FRAME_ERR_UTF8 : UVHTTP_WS_FRAME_ERR_CLOSE;
                } else if (fs < 0) {
                    reason = UVHTTP_WS_FAIL_DECODE;
                    fl.frame = r.first_frame + r.n_delivered;
                    fl.code = 1002;
                }
                fl.reason = (uint8_t)reason;
                // the verdict over the kept frames
                if (a.verdict && u != kNone && c != kNone && (u > c || (close_cut && u == c))) {
                    v.status = UVHTTP_WS_UTF8_VALID;
                    v.first_invalid = kNone;
                    v.state = uvhttp_ws_utf8_state_t{};
                }
            }
        }
        a.results_out[s] = r;
        if (a.verdict_out) a.verdict_out[s] = v;
        a.fail[s] = fl;
    }
    // the wave's counts: one atomic per counter that is not zero (failures are rare)
    const int lane = threadIdx.x & 63;
    const uint64_t m_any = __ballot(reason != UVHTTP_WS_FAIL_NONE);
    const uint64_t m_bad = __ballot(bad);
    if (!m_any && !m_bad) return;  // the same in every lane of the wave
    const uint64_t m_dec = __ballot(reason == UVHTTP_WS_FAIL_DECODE), m_utf = __ballot(reason == UVHTTP_WS_FAIL_UTF8);
    const uint64_t m_len = __ballot(reason == UVHTTP_WS_FAIL_CLOSE_LEN);
    const uint64_t m_code = __ballot(reason == UVHTTP_WS_FAIL_CLOSE_CODE);
    uint64_t drop = dropped;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) drop += __shfl_down(drop, d);
    if (lane != 0) return;
    if (drop) atomicAdd(reinterpret_cast<unsigned long long*>(&a.sum->n_dropped), (unsigned long long)drop);
    if (m_dec) atomicAdd(&a.sum->n_decode, (uint32_t)__popcll(m_dec));
    if (m_utf) atomicAdd(&a.sum->n_utf8, (uint32_t)__popcll(m_utf));
    if (m_len) atomicAdd(&a.sum->n_close_len, (uint32_t)__popcll(m_len));
    if (m_code) atomicAdd(&a.sum->n_close_code, (uint32_t)__popcll(m_code));
    if (m_bad) atomicAdd(&a.sum->n_bad_range, (uint32_t)__popcll(m_bad));
    if (m_any) atomicMin(&a.sum->first_failed, (uint32_t)(s + (uint64_t)(__ffsll((unsigned long long)m_any) - 1)));
}

void fp_carve(Carver& c, FpArgs& a, uint64_t blocks) {
    a.agg_mark = c.take<uint64_t>(blocks ? blocks : 1);
    a.marks = c.take<uint32_t>(a.max_frames);
    a.first_close = c.take<uint32_t>(a.n_streams);
}

}  // namespace

extern "C" int uvhttp_ws_gpu_fail_points_streams(
    uvhttp_ws_gpu_engine_t* e, const uint8_t* d_wire, uint64_t wire_len, const uvhttp_ws_frame_desc_t* d_desc,
    uint32_t max_frames, const uvhttp_ws_stream_result_t* d_results, uint32_t n_streams,
    const uvhttp_ws_utf8_conn_verdict_t* d_verdict, const uint8_t* d_enable, uint32_t flags,
    uvhttp_ws_stream_result_t* d_results_out, uvhttp_ws_utf8_conn_verdict_t* d_verdict_out,
    uvhttp_ws_fail_conn_t* d_fail, uvhttp_ws_fail_summary_t* d_summary, void* stream) {
    static_assert(sizeof(uvhttp_ws_fail_conn_t) == 16 && sizeof(uvhttp_ws_fail_summary_t) == 32, "ABI");
    if (!e) return UVHTTP_WS_GPU_EINVAL;
    if (!d_desc || !d_results || !d_results_out || !d_fail || !d_summary || (!d_wire && wire_len) ||
        (d_verdict == nullptr) != (d_verdict_out == nullptr))
        return uvws_set_err(e, UVHTTP_WS_GPU_EINVAL, "fail_points_streams: NULL argument");
    if (((uintptr_t)d_desc & 7u) || ((uintptr_t)d_results & 7u) || ((uintptr_t)d_results_out & 7u) ||
        ((uintptr_t)d_summary & 7u) || ((uintptr_t)d_verdict & 3u) || ((uintptr_t)d_verdict_out & 3u) ||
        ((uintptr_t)d_fail & 3u))
        return uvws_set_err(e, UVHTTP_WS_GPU_EINVAL, "fail_points_streams: misaligned argument");
    if ((flags & ~UVHTTP_WS_FAIL_CHECK_CLOSE) || max_frames > (1u << 28) || n_streams > (1u << 31))
        return uvws_set_err(e, UVHTTP_WS_GPU_EINVAL, "fail_points_streams: unknown flags, max_frames > 2^28 or n_streams > 2^31");
    FpArgs a = {};
    a.wire = d_wire;
    a.wire_len = wire_len;
    a.desc = d_desc;
    a.max_frames = max_frames;
    a.n_streams = n_streams;
    a.results = d_results;
    a.verdict = d_verdict;
    a.enable = d_enable;
    a.flags = flags;
    a.results_out = d_results_out;
    a.verdict_out = d_verdict_out;
    a.fail = d_fail;
    a.sum = d_summary;
    const uint64_t blocks = ((uint64_t)max_frames + kBlock - 1) / kBlock;
    const uint64_t grid_s = ((uint64_t)n_streams + kBlock - 1) / kBlock;
    Carver count{nullptr};
    fp_carve(count, a, blocks);

    hipStream_t s = (hipStream_t)stream;
    const int prev = uvws_call_enter(e, s);
    char* mem = static_cast<char*>(uvws_fail_scratch(e, count.bytes(), s));
    if (!mem) {
        (void)uvws_call_leave(e, prev, "fail_points_streams launch");
        return uvws_set_err(e, UVHTTP_WS_GPU_ENOMEM, "fail_points scratch (a captured call must not grow it)");
    }
    Carver carve{mem};
    fp_carve(carve, a, blocks);
    // (one workgroup at least: it zeroes the summary)
    engine_grid_chunks(e, blocks ? blocks : 1, [&](uint32_t grid, uint64_t tb) {
        hipLaunchKernelGGL(k_fp_init, dim3(grid), dim3(kBlock), 0, s, a, tb);
    });
    engine_grid_chunks(e, grid_s, [&](uint32_t grid, uint64_t tb) {
        hipLaunchKernelGGL(k_fp_conns, dim3(grid), dim3(kBlock), 0, s, a, tb);
    });
    if (blocks && grid_s) {
        engine_grid_chunks(e, blocks, [&](uint32_t grid, uint64_t tb) {
            hipLaunchKernelGGL((k_mark_reduce<>), dim3(grid), dim3(kBlock), 0, s, a.marks, a.max_frames, a.agg_mark, tb);
        });
        hipLaunchKernelGGL((k_scan_top<LastOp>), dim3(1), dim3(kBlock), 0, s, a.agg_mark, a.agg_mark, (uint32_t)blocks);
        engine_grid_chunks(e, blocks, [&](uint32_t grid, uint64_t tb) {
            hipLaunchKernelGGL(k_fp_classify, dim3(grid), dim3(kBlock), 0, s, a, tb);
        });
    }
    engine_grid_chunks(e, grid_s, [&](uint32_t grid, uint64_t tb) {
        hipLaunchKernelGGL(k_fp_judge, dim3(grid), dim3(kBlock), 0, s, a, tb);
    });
    return uvws_call_leave(e, prev, "fail_points_streams launch");
}
