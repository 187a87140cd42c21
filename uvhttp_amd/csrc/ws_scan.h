// ws_scan.h — what the device calls that run after a decode share (utf8_frames_gpu.hip,
// ws_replies_gpu.hip, ws_echo_gpu.hip, ws_close_gpu.hip, ws_fail_gpu.hip): the two-level scan over
// descriptors or connections, the head marks that give a descriptor its connection, a
// connection's descriptor range, and the carve of a call's engine scratch.  Everything here has
// internal linkage: every object that includes it holds its own copy.
//
// The scan's shape, the same in every call: a workgroup of kBlock lanes scans its kBlock entries
// (block_scan) and lane 0 writes the workgroup's total to agg[block]; k_scan_top turns agg[0, n)
// into inclusive prefixes; a second pass scans its entries again with agg[block - 1] in front.
// An operator is a default-constructible functor on 64-bit words, associative, with identity 0.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "uvhttp_ws_amd.h"

namespace {

constexpr int kBlock = 256;  // the scan block: descriptors (or connections) per workgroup
constexpr int kWaves = kBlock / 64;
constexpr uint32_t kNone = 0xFFFFFFFFu;

struct LastOp {  // the later mark (0 = no mark)
    __device__ __forceinline__ uint64_t operator()(uint64_t a, uint64_t b) const { return b ? b : a; }
};
struct AddOp {  // also two counts in one word, where neither can carry into the other
    __device__ __forceinline__ uint64_t operator()(uint64_t a, uint64_t b) const { return a + b; }
};

template <typename T>
struct ScanWord {  // (keeps v and identity out of T's deduction: s_wave decides the type)
    typedef T type;
};

// Inclusive scan over the workgroup's kBlock lanes; *total = all of them.  Every lane of the
// workgroup must call it, outside divergent control flow.  s_wave holds kWaves words of LDS; a
// kernel may pass the same s_wave to one call after another, because the first barrier in here
// lets every lane finish reading the previous call's words before any is overwritten.
template <typename T, typename Op>
__device__ __forceinline__ T block_scan(typename ScanWord<T>::type v, Op op, typename ScanWord<T>::type identity,
                                        T* s_wave, T* total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const T o = __shfl_up(v, d);
        if (lane >= d) v = op(o, v);
    }
    __syncthreads();  // s_wave may still be read from the previous use
    if (lane == 63) s_wave[w] = v;
    __syncthreads();
    T pre = identity, tot = identity;
#pragma unroll
    for (int k = 0; k < kWaves; ++k) {
        if (k < w) pre = op(pre, s_wave[k]);
        tot = op(tot, s_wave[k]);
    }
    *total = tot;
    return op(pre, v);
}

// One workgroup per column (blockIdx.x picks agg0 or agg1; a caller with one column launches one
// workgroup and passes it twice): agg[0, n) -> inclusive prefixes.  Every lane folds its own run
// of entries, the runs' totals are scanned once, and the lane writes its run back with the prefix
// in front.  Launched with kBlock lanes; n entries must be readable and writable.
template <typename Op>
__global__ __launch_bounds__(kBlock) void k_scan_top(uint64_t* agg0, uint64_t* agg1, uint32_t n) {
    __shared__ uint64_t s_wave[kWaves];
    __shared__ uint64_t s_last[kWaves];
    uint64_t* agg = blockIdx.x ? agg1 : agg0;
    const uint32_t per = (n + kBlock - 1) / kBlock;
    const uint64_t lo = (uint64_t)threadIdx.x * per;
    const uint64_t hi = lo + per < n ? lo + per : n;
    uint64_t run = 0;
    for (uint64_t i = lo; i < hi; ++i) run = Op()(run, agg[i]);
    uint64_t tot;
    const uint64_t inc = block_scan(run, Op(), 0, s_wave, &tot);
    const uint64_t left = __shfl_up(inc, 1);  // the runs before this lane's
    if ((threadIdx.x & 63) == 63) s_last[threadIdx.x >> 6] = inc;
    __syncthreads();
    uint64_t acc = (threadIdx.x & 63) ? left : (threadIdx.x ? s_last[(threadIdx.x >> 6) - 1] : 0);
    for (uint64_t i = lo; i < hi; ++i) {
        acc = Op()(acc, agg[i]);
        agg[i] = acc;
    }
}

// The head marks: marks[f] = connection + 1 at a connection's first considered descriptor, else
// 0, so the last mark at or before f names f's connection.  One lane per descriptor of workgroup
// tb + blockIdx.x: agg_mark[workgroup] = its last mark.  marks holds max_frames entries.  (A template
// over the tile base's type only so that a source which does not launch it holds no copy.)
template <typename B = uint64_t>
__global__ __launch_bounds__(kBlock) void k_mark_reduce(const uint32_t* marks, uint32_t max_frames, uint64_t* agg_mark,
                                                        B tb) {
    __shared__ uint64_t s_wave[kWaves];
    const uint64_t b = (uint64_t)tb + blockIdx.x;
    const uint64_t f = b * kBlock + threadIdx.x;
    const uint64_t m = f < max_frames ? marks[f] : 0;
    uint64_t tot;
    (void)block_scan(m, LastOp(), 0, s_wave, &tot);
    if (threadIdx.x == 0) agg_mark[b] = tot;
}

// ... and, after k_scan_top<LastOp> over agg_mark: the last mark at or before this lane's
// descriptor b * kBlock + threadIdx.x (0: none).  Every lane of workgroup b calls it.
template <typename B>
__device__ __forceinline__ uint64_t head_mark(const uint32_t* marks, uint32_t max_frames, const uint64_t* agg_mark,
                                              B b, uint64_t* s_wave) {
    const uint64_t f = (uint64_t)b * kBlock + threadIdx.x;
    const uint64_t m = f < max_frames ? marks[f] : 0;
    const uint64_t pre = b ? agg_mark[b - 1] : 0;
    uint64_t tot;
    return LastOp()(pre, block_scan(m, LastOp(), 0, s_wave, &tot));
}

// a connection's considered descriptors [ff, ff + nd)
struct Range {
    uint32_t ff, nd;
};

// ... kept inside [0, max_frames), whatever the result table holds
__device__ __forceinline__ Range clamp_range(Range r, uint32_t max_frames) {
    if (r.ff >= max_frames) r.nd = 0;
    else if (r.nd > max_frames - r.ff) r.nd = max_frames - r.ff;
    return r;
}

// the decode call failed, not the connection: its descriptors say nothing.  (The UTF-8 verdicts
// alone still judge a connection under ERR_DEVICE, as their header says; they do not use this.)
__device__ __forceinline__ bool call_failed(int32_t first_status) {
    return first_status == UVHTTP_WS_FRAME_ERR_CAPACITY || first_status == UVHTTP_WS_FRAME_ERR_LAYOUT ||
           first_status == UVHTTP_WS_FRAME_ERR_DEVICE;
}

// [off, off + len) lies inside [0, limit).  (limit by reference: a field of the kernel's arguments
// is then read here, where it is used, and the callers' code stays what it was)
__device__ __forceinline__ bool range_ok(const uint64_t& limit, uint64_t off, uint64_t len) {
    return len <= limit && off <= limit - len;
}

// ---- the host side: a call's arrays in its engine scratch ------------------------------------------

inline size_t align_up(size_t x) { return (x + 255) / 256 * 256; }

// A stage lists its arrays once, in a function of take<T>(count) calls.  Run over a null base it
// only adds up bytes() to ask the engine for; run again over the block the engine returned it
// hands out the pointers.  Every array starts 256-byte aligned.
struct Carver {
    char* base;
    size_t off = 0;
    template <typename T>
    T* take(size_t count) {
        T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
        off = align_up(off + count * sizeof(T));
        return p;
    }
    size_t bytes() const { return off ? off : 256; }
};

}  // namespace
