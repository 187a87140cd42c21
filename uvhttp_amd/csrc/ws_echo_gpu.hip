// ws_echo_gpu.hip — the echo server's data frames built on the device after a decode
// (include/uvhttp_ws_amd.h: uvhttp_ws_gpu_echo_messages_streams / _inplace): for every message
// whose FIN frame was delivered, the one frame on_message -> uvhttp_ws_send_text / _send_binary
// puts on the wire (src/uvhttp_websocket.c:509-608), gathered from the message's fragments where
// they lie in the decoded wire and from the bytes carried in from earlier calls; and the bytes of
// every message still open, laid out as the next call's carry.  Short launches over descriptors
// and connections, scratch in the engine, no waiting between workgroups, then one byte mover:
//
//   k_echo_init     marks[f] = 0 per descriptor; the summary zeroed
//   k_echo_conns    one lane per connection: its state word (enabled, NO_KEYS, NO_CARRY, carries
//                   in), its scratch words, a head mark at its first considered descriptor
//   k_mark_reduce / k_scan_top   the scan of the head marks (ws_scan.h)
//   k_echo_classify one lane per descriptor, 32 bytes read: its connection; a word — in range,
//                   first / last of the range, a delivered data frame, start of a message, FIN;
//                   first_close[connection] (atomicMin), bad[connection] for a payload outside
//                   the wire.  The workgroup's data-payload bytes and its last message marker
//   k_scan_top      both aggregates, one launch each
//   k_echo_prefix   one lane per descriptor: dsum[f] = data-payload bytes before f (a message's
//                   length is a difference of two of them plus its carry), and view[f] = the
//                   message f belongs to: the nearest earlier start frame, or the head of the
//                   connection's range when a message was carried in, unless a FIN lies between
//   k_echo_size     one lane per descriptor: the lane of a FIN frame decides whether its message
//                   is echoed (not after the first CLOSE, not empty under SERVER_SEND, connection
//                   not bad) and sizes the frame; the lane of a range's last frame sizes the
//                   message still open.  The workgroup's echoes and bytes
//   k_scan_top, k_echo_creduce, k_scan_top   the totals: echoes, bytes, open bytes — the one set
//                   every writer goes by
//   k_echo_offsets  one lane per descriptor: slot and offset from the scan; d_out_off[j] and the
//                   echo's record (where its bytes come from), written by the FIN frame's lane;
//                   the running totals before a connection's first frame and after its last
//   k_echo_tail     d_out_off[n_echoes .. max_echoes] = the total (all 0 on capacity)
//   k_echo_creduce / k_scan_top / k_echo_finish   one lane per connection: first_echo and
//                   d_open_off as exclusive sums, the 32-byte result, the run, the open message's
//                   record, the summary
//   k_echo_emit     the hot path: P bytes read, H + P written.  One workgroup per 64 KiB tile of
//                   d_out, then of d_open (tile counts from out_cap / open_cap; tiles past the
//                   totals return).  The record of a tile's first byte is in a map k_echo_offsets
//                   / k_echo_finish wrote (the lane of a record notes it for every tile that
//                   starts inside it), so the tile's records are map[tile] .. map[tile + 1].
//                   Every lane owns aligned 16-byte vectors of the tile, four side by side so
//                   that their loads overlap: it finds each vector's record inside that window
//                   (a search over d_out_off / d_open_off, the same number of steps in every
//                   lane), and stores the whole vector — an unaligned 16-byte source window
//                   XOR-ed with the rotated key — when it is payload of the record's carry or of
//                   its only fragment.  Other vectors go the long way: the source frame by a
//                   search over dsum inside the record's frames, or byte by byte (headers,
//                   fragment joins, record joins).  A tile that is payload of one record from one
//                   source skips all of it: one record read, sixteen loads per lane in flight.
//                   Only the last vector of an output may take byte stores
//
// The descriptor order is the output order: records ascend in their destination, and so do a
// record's frames (dsum), so nothing is sorted.  A table whose connections' ranges overlap gets
// unspecified bytes, but nothing outside the wire, the carry, the descriptors below max_frames,
// the n_streams entries, d_out below out_cap, d_open below open_cap and the offset tables is read
// or written: every source frame is one whose range k_echo_classify checked, and the emit is
// bounded by the totals the capacity test used.
//
// The relay (uvhttp_ws_gpu_relay_messages_streams) is the same sizing and the same emit with
// another order: server frames laid out by (room, connection, frame).  Nothing in the emit depends
// on descriptor order, only on records that ascend in their destination by output slot, so what
// is added lies between k_echo_size and the record writes:
//
//   k_echo_offsets  run once for the connections' counts and bytes only (cbeg .. bend)
//   k_relay_hist / _hreduce / k_scan_top / k_relay_hscan / k_relay_scatter   per 8 bits of n_rooms:
//                   the connections sorted by (min(room, n_rooms), index), see "the relay's order"
//   k_relay_oreduce / k_scan_top x 2 / k_relay_obase   counts and bytes scanned in that order:
//                   every connection's first slot and offset, and the sums by place for the rooms
//   k_echo_offsets  again: each record, d_out_off[j] and the tile map at the connection's base
//   k_relay_rooms   one lane per room: two searches over the sorted keys, d_rooms[r]
//   k_relay_recv    one lane per receiver: its room's run
//
// The kernels both calls use and the relay changes (init, conns, size, offsets, finish, emit) are
// templates over the argument type, EcArgs or RlArgs: the echo's instances are the kernels they
// were, launched as they were, and only the relay's carry the room order and its arguments.
//
// The answers (uvhttp_ws_gpu_answer_messages_streams / _inplace) are the echo's launch sequence
// over a third argument type, AnArgs: a PONG or a CLOSE echo is one more record of the same scan,
// in the slot its frame's descriptor gives it, so a connection's run is its echoes and its control
// replies in frame order.  What AnArgs' instances add:
//
//   k_echo_classify  also marks a delivered PING / CLOSE of an active connection (kCtl, the
//                    reply's payload length in the word) and range-checks the reply's payload
//   k_echo_size      the lane of such a frame decides whether it is answered (not after the first
//                    CLOSE unless the flag says so, connection not bad) and sizes the reply: 2
//                    header bytes, 4 more when masked, the payload.  A third aggregate, replies
//                    << 35 | their payload bytes, for the per-connection reply counts
//   k_scan_top       ... its prefixes
//   k_echo_offsets   the reply's record on its own lane: b0 = 0x8A or 0x88, one = 1, g = fend = f,
//                    src0 = the control frame's payload_off; rbeg / rend per connection
//   k_echo_finish    the answer result (closed, n_replies), the optional reply table that
//                    close_frames_streams reads, the answer summary
//   k_echo_emit      the same byte mover.  dsum counts data payloads only, so a control record's
//                    bytes are never looked up there: every path that locates a source byte of a
//                    record with one = 1 — the vector path, and in this instance the long way's
//                    whole-vector and byte-wise paths (emit_vector<true>, payload_byte<true>) —
//                    takes it from src0
//
// k_echo_classify became a template for this (its EcArgs instance is the kernel it was, and the
// relay still launches that one); no other instance of the echo or the relay changed.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "uvhttp_ws_amd.h"
#include "ws_engine_int.h"
#include "ws_scan.h"

namespace {

constexpr int kBatch = 4;     // vectors a lane of the emit handles side by side
constexpr int kBatches = 4;   // ... this many times
constexpr int kVecPerLane = kBatch * kBatches;
constexpr uint64_t kTile = (uint64_t)kBlock * 16 * kVecPerLane;  // output bytes per emit workgroup: 64 KiB

// the word per descriptor (elem)
constexpr uint64_t kIn = 1ull << 0;      // inside its connection's considered range
constexpr uint64_t kFirst = 1ull << 1;   // the range's first frame
constexpr uint64_t kLast = 1ull << 2;    // the range's last frame
constexpr uint64_t kData = 1ull << 3;    // a delivered data frame of an active connection, range checked
constexpr uint64_t kStart = 1ull << 4;   // ... with opcode 1 or 2
constexpr uint64_t kFin = 1ull << 5;     // ... with FIN
constexpr uint64_t kCarryHead = 1ull << 6;  // kFirst of a connection that carries a message in
constexpr uint64_t kEcho = 1ull << 7;    // the FIN frame of an echoed message (k_echo_size)
// ... and the answers' (AnArgs) only:
constexpr uint64_t kCtl = 1ull << 8;     // a delivered PING / CLOSE of an active connection, range checked
constexpr uint64_t kCtlClose = 1ull << 9;  // ... a CLOSE (the reply is a CLOSE, else a PONG)
constexpr uint64_t kReply = 1ull << 10;  // answered (k_echo_size)
constexpr int kCtlLenShift = 16;         // bits 16-22: the reply's payload length
constexpr uint64_t kCtlLenMask = 0x7F;
// bits 32-63: the connection

// the word per connection (cstate): bits 0-7 the static status, then
constexpr uint32_t kCActive = 1u << 8;   // enabled and neither NO_KEYS nor NO_CARRY
constexpr uint32_t kCCarry = 1u << 9;    // active and pending_bytes != 0 (the carry is usable)

// a message marker: (frame + 1) << 2 | kind; 0 = no marker
constexpr uint64_t kMsgNone = 0, kMsgStart = 1, kMsgCarried = 2, kMsgCarryOnly = 3;
__device__ __forceinline__ uint64_t marker(uint64_t f, uint64_t kind) { return ((f + 1) << 2) | kind; }

struct EcRec {  // where one output frame's (or one open message's) bytes come from
    uint64_t dbase;      // dsum of the first frame that can hold a fragment
    uint64_t len;        // payload bytes: carry + fragments
    uint64_t carry_src;  // offset of the carried bytes in d_carry
    uint64_t carry_len;
    uint64_t src0;       // one: the single fragment's payload_off
    uint32_t g, fend;    // the fragments lie in desc[g, fend]
    uint32_t key;
    uint8_t hdr, b0, masked, one;  // header bytes (key included; 0 for an open message), first byte;
                                   // one: desc[g] is the message's only fragment (g == fend)
    uint64_t pad;
};
static_assert(sizeof(EcRec) == 64, "record");

struct EcArgs {
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
    const uint8_t* carry;                        // or null
    uint64_t carry_len;
    const uint64_t* carry_off;                   // or null
    uint8_t* out;
    uint64_t out_cap;
    uint64_t* out_off;
    uint32_t max_echoes;
    uint32_t* runs;                              // or null
    uint32_t run_stride;                         // bytes
    uint8_t* open;                               // or null
    uint64_t open_cap;
    uint64_t* open_off;
    uvhttp_ws_echo_conn_t* conn;
    uvhttp_ws_echo_summary_t* sum;
    // engine scratch
    uint32_t* marks;        // [max_frames] connection + 1 at its first considered descriptor
    uint64_t* elem;         // [max_frames] the word above
    uint64_t* dsum;         // [max_frames] data-payload bytes of the descriptors before f
    uint64_t* view;         // [max_frames] the marker of the message f belongs to
    uint64_t* agg_mark;     // [blocks] last head mark, then inclusive
    uint64_t* agg_d;        // [blocks] data-payload bytes, then inclusive
    uint64_t* agg_post;     // [blocks] last message marker, then inclusive
    uint64_t* agg_cnt;      // [blocks] echoes, then inclusive
    uint64_t* agg_bytes;    // [blocks] echo bytes, then inclusive
    uint64_t* agg_cn;       // [connection blocks] echoes, then inclusive
    uint64_t* agg_co;       // [connection blocks] open bytes, then inclusive
    const uint64_t* tot_cnt;    // &agg_cnt[blocks - 1], null when there is no descriptor
    const uint64_t* tot_bytes;
    const uint64_t* tot_open;   // &agg_co[connection blocks - 1], null when there is no connection
    uint32_t* cstate;       // [n_streams] the word above
    uint32_t* first_close;  // [n_streams] the connection's first delivered CLOSE, kNone if none
    uint32_t* bad;          // [n_streams] a data payload outside the wire
    uint32_t* cbeg;         // [n_streams] echoes before the connection's first frame ...
    uint32_t* cend;         // ... and up to its last
    uint64_t* bbeg;         // the same in bytes
    uint64_t* bend;
    uint64_t* olen;         // [n_streams] bytes of the message still open
    uint64_t* omark;        // [n_streams] its marker (frame g and kind)
    uint32_t* ofend;        // [n_streams] the range's last frame
    EcRec* rec;             // [max_echoes] the echoes' records
    EcRec* orec;            // [n_streams] the open messages' records
    uint32_t* tmap;         // [tiles of d_out] the record that holds the tile's first byte
    uint32_t* omap;         // [tiles of d_open] likewise
    static constexpr bool kRelay = false;
    static constexpr bool kAnswer = false;
};

// The relay's arguments (uvhttp_ws_gpu_relay_messages_streams): the echo's and its own.  The
// kernels both calls share are templates over the argument type, so the echo's instances are the
// kernels they were, with the arguments they had.
struct RlArgs : EcArgs {
    static constexpr bool kRelay = true;  // server frames in (room, connection) order
    uint32_t count_only;        // k_echo_offsets: the connections' counts and bytes, nothing else
    const uint32_t* room;       // [n_streams] the sender's room
    uint32_t n_rooms;
    uint32_t n_receivers;
    uvhttp_ws_relay_room_t* rooms;  // [n_rooms]
    const uint32_t* recv_room;  // [n_receivers]
    uint32_t* sends;            // (first_frame, n_frames) per receiver, send_stride bytes apart
    uint32_t send_stride;
    // ... its scratch
    uint32_t* skey[2];      // [n_streams] sort keys min(room, n_rooms), in and out of a radix pass
    uint32_t* sidx[2];      // [n_streams] the connections that go with them
    const uint32_t* okey;   // the sorted keys and connections: skey / sidx [passes & 1]
    const uint32_t* oidx;
    uint32_t* hist;         // [256 digits][connection blocks] digit counts, then exclusive sums
    uint64_t* agg_h;        // [connection blocks] sums of 256 hist entries, then inclusive
    uint64_t* agg_pc;       // [connection blocks] frames of 256 places of the order, then inclusive
    uint64_t* agg_pb;       // the same in bytes
    uint64_t* pcnt;         // [n_streams + 1] frames before place p of the order; the last: all
    uint64_t* pbytes;       // the same in bytes
    uint32_t* rcnt;         // [n_streams] pcnt at the connection's place: its first frame's slot
    uint64_t* rbytes;       // likewise its first frame's offset
    uint32_t* written;      // [1] records k_echo_offsets wrote: the emit runs only when all were
};

// The answers' arguments (uvhttp_ws_gpu_answer_messages_streams / _inplace): the echo's, with
// PONGs and CLOSE echoes as records of the same scan.  conn / sum point at the answer structs,
// which begin as the echo's.
struct AnArgs : EcArgs {
    static constexpr bool kAnswer = true;
    uvhttp_ws_reply_conn_t* reply_conn;  // or null
    // ... its scratch
    uint64_t* agg_rep;      // [blocks] replies << 35 | their payload bytes, then inclusive
    const uint64_t* tot_rep;  // &agg_rep[blocks - 1], null when there is no descriptor
    uint64_t* rbeg;         // [n_streams] that sum before the connection's first frame ...
    uint64_t* rend;         // ... and up to its last
};
// replies << 35 | payload bytes: at most 2^28 replies of at most 125 bytes
constexpr int kRepShift = 35;

// connection s's considered descriptors, inside [0, max_frames)
__device__ __forceinline__ Range conn_range(const EcArgs& a, uint32_t s) {
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

__device__ __forceinline__ bool conn_server(const EcArgs& a, uint32_t s) {
    return a.streams ? a.streams[s].is_server != 0 : a.is_server != 0;
}
// whether the connection's output frames are masked: a client's echoes; relayed frames never are
template <class A>
__device__ __forceinline__ bool conn_masked(const A& a, uint32_t s) {
    return !A::kRelay && !conn_server(a, s);
}
__device__ __forceinline__ uint64_t conn_pending(const EcArgs& a, uint32_t s) {
    return a.streams ? a.streams[s].pending_bytes : 0;
}
__device__ __forceinline__ uint32_t conn_pending_opcode(const EcArgs& a, uint32_t s) {
    return a.streams ? (uint32_t)a.streams[s].pending_opcode & 0x0Fu : 0u;
}

// the connection's frames and their bytes, after k_echo_offsets (0 where a broken table left its
// end before its beginning)
__device__ __forceinline__ uint64_t conn_frames(const EcArgs& a, uint32_t s) {
    return a.cend[s] >= a.cbeg[s] ? a.cend[s] - a.cbeg[s] : 0u;
}
__device__ __forceinline__ uint64_t conn_bytes(const EcArgs& a, uint32_t s) {
    return a.bend[s] >= a.bbeg[s] ? a.bend[s] - a.bbeg[s] : 0u;
}

// the three totals and the capacity test every writer goes by
struct EcTotals {
    uint64_t cnt, bytes, open;
    bool fits;
};
__device__ __forceinline__ EcTotals totals(const EcArgs& a) {
    EcTotals t;
    t.cnt = a.tot_cnt ? *a.tot_cnt : 0;
    t.bytes = a.tot_bytes ? *a.tot_bytes : 0;
    t.open = a.tot_open ? *a.tot_open : 0;
    t.fits = t.cnt <= a.max_echoes && t.bytes <= a.out_cap && (!a.open || t.open <= a.open_cap);
    return t;
}

// the reply of a control frame the answers' classify marked
__device__ __forceinline__ uint64_t ctl_len(uint64_t e) { return (e >> kCtlLenShift) & kCtlLenMask; }

__device__ __forceinline__ uint32_t header_bytes(uint64_t len, bool masked) {
    return (len <= 125 ? 2u : len <= 65535 ? 4u : 10u) + (masked ? 4u : 0u);
}

template <class A>
__global__ __launch_bounds__(kBlock) void k_echo_init(A a) {
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i == 0) {
        uvhttp_ws_echo_summary_t z = {};
        *a.sum = z;
        a.open_off[0] = 0;
        if constexpr (A::kRelay) *a.written = 0;
    }
    static_assert(sizeof(uvhttp_ws_answer_summary_t) == sizeof(uvhttp_ws_echo_summary_t), "zeroed through the echo's type");
    if (i < a.max_frames) a.marks[i] = 0;
}

template <class A>
__global__ __launch_bounds__(kBlock) void k_echo_conns(A a) {
    const uint64_t s = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (s >= a.n_streams) return;
    a.first_close[s] = kNone;
    a.bad[s] = 0;
    a.cbeg[s] = 0;
    a.cend[s] = 0;
    a.bbeg[s] = 0;
    a.bend[s] = 0;
    a.ofend[s] = 0;
    if constexpr (A::kAnswer) {
        a.rbeg[s] = 0;
        a.rend[s] = 0;
    }
    uint32_t st = 0;
    const uint64_t pend = conn_pending(a, (uint32_t)s);
    if (!a.enable || a.enable[s] != 0) {
        if (conn_masked(a, (uint32_t)s) && !a.keys) {
            st = UVHTTP_WS_ECHO_NO_KEYS;
        } else if (pend != 0) {
            bool usable = false;
            if (a.carry && a.carry_off) {
                const uint64_t lo = a.carry_off[s], hi = a.carry_off[s + 1];
                usable = hi >= lo && hi <= a.carry_len && hi - lo == pend;
            }
            st = usable ? (kCActive | kCCarry) : (uint32_t)UVHTTP_WS_ECHO_NO_CARRY;
        } else {
            st = kCActive;
        }
        if constexpr (A::kRelay) {
            if ((st & kCActive) && a.room[s] >= a.n_rooms) {  // after NO_CARRY, before BAD_RANGE
                st = UVHTTP_WS_RELAY_BAD_ROOM;
                atomicAdd(&a.sum->reserved[0], 1u);  // uvhttp_ws_relay_summary_t: n_bad_rooms
            }
        }
    }
    if constexpr (A::kRelay) {  // the radix sort's input: every connection, in its room or after the last
        const uint32_t room = a.room[s];
        a.skey[0][s] = room < a.n_rooms ? room : a.n_rooms;
        a.sidx[0][s] = (uint32_t)s;
    }
    a.cstate[s] = st;
    const Range r = conn_range(a, (uint32_t)s);
    if (r.nd) a.marks[r.ff] = (uint32_t)s + 1;
    // a connection that considers no frame passes its carry through
    const bool through = !r.nd && (st & kCCarry);
    a.olen[s] = through ? pend : 0;
    a.omark[s] = through ? marker(0, kMsgCarryOnly) : 0;
}

// what frame f posts for the frames after it: a FIN data frame ends the message, a start frame
// begins one, the head of a range begins the carried-in one (or none)
__device__ __forceinline__ uint64_t posted_of(uint64_t e, uint64_t f) {
    if (!(e & kIn)) return 0;
    if ((e & kData) && (e & kFin)) return marker(f, kMsgNone);
    if (e & kStart) return marker(f, kMsgStart);
    if (e & kFirst) return marker(f, (e & kCarryHead) ? kMsgCarried : kMsgNone);
    return 0;
}

template <class A>
__global__ __launch_bounds__(kBlock) void k_echo_classify(A a) {
    __shared__ uint64_t s_wave[kWaves];
    const uint64_t f = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    const bool live = f < a.max_frames;
    const uint64_t head = head_mark(a.marks, a.max_frames, a.agg_mark, blockIdx.x, s_wave);
    uint64_t e = 0, plen = 0;
    if (live && head != 0 && head - 1 < a.n_streams) {
        const uint32_t conn = (uint32_t)(head - 1);
        const Range r = conn_range(a, conn);
        if (f >= r.ff && f - r.ff < r.nd) {
            const uint32_t cs = a.cstate[conn];
            e = kIn | ((uint64_t)conn << 32) | (f == r.ff ? kFirst : 0) | (f - r.ff == r.nd - 1 ? kLast : 0);
            if (f == r.ff && (cs & kCCarry)) e |= kCarryHead;
            const uvhttp_ws_frame_desc_t& d = a.desc[f];
            const uint32_t op = d.opcode;
            if (d.status == UVHTTP_WS_FRAME_OK) {
                if (op == UVHTTP_WS_OPCODE_CLOSE) atomicMin(&a.first_close[conn], (uint32_t)f);
                if ((cs & kCActive) && op <= UVHTTP_WS_OPCODE_BINARY) {
                    const uint64_t len = d.payload_len;
                    if (len != 0 && !range_ok(a.wire_len, d.payload_off, len)) {
                        a.bad[conn] = 1;
                    } else {
                        plen = len;
                        e |= kData | (op != UVHTTP_WS_OPCODE_CONTINUATION ? kStart : 0) |
                             ((d.flags & UVHTTP_WS_FLAG_FIN) ? kFin : 0);
                    }
                }
                if constexpr (A::kAnswer) {
                    if ((cs & kCActive) && (op == UVHTTP_WS_OPCODE_PING || op == UVHTTP_WS_OPCODE_CLOSE)) {
                        uint64_t len = d.payload_len;  // the reply's: k_rp_classify's rule
                        if (op == UVHTTP_WS_OPCODE_CLOSE && len < 2) len = 0;
                        if (len > 125) len = 125;
                        if (len != 0 && !range_ok(a.wire_len, d.payload_off, len)) a.bad[conn] = 1;
                        else e |= kCtl | (op == UVHTTP_WS_OPCODE_CLOSE ? kCtlClose : 0) | (len << kCtlLenShift);
                    }
                }
            }
        }
    }
    if (live) a.elem[f] = e;
    uint64_t tot_d, tot_p;
    (void)block_scan(plen, AddOp(), 0, s_wave, &tot_d);
    (void)block_scan(posted_of(e, f), LastOp(), 0, s_wave, &tot_p);
    if (threadIdx.x == 0) {
        a.agg_d[blockIdx.x] = tot_d;
        a.agg_post[blockIdx.x] = tot_p;
    }
}

__global__ __launch_bounds__(kBlock) void k_echo_prefix(EcArgs a) {
    __shared__ uint64_t s_wave[kWaves];
    __shared__ uint64_t s_inc[kBlock];
    const uint64_t f = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    const bool live = f < a.max_frames;
    const uint64_t e = live ? a.elem[f] : 0;
    const uint64_t plen = (e & kData) ? a.desc[f].payload_len : 0;
    uint64_t tot;
    const uint64_t inc_d = (blockIdx.x ? a.agg_d[blockIdx.x - 1] : 0) + block_scan(plen, AddOp(), 0, s_wave, &tot);
    s_inc[threadIdx.x] = block_scan(posted_of(e, f), LastOp(), 0, s_wave, &tot);
    __syncthreads();
    const uint64_t before = LastOp()(blockIdx.x ? a.agg_post[blockIdx.x - 1] : 0, threadIdx.x ? s_inc[threadIdx.x - 1] : 0);
    if (!live) return;
    a.dsum[f] = inc_d - plen;
    uint64_t v = 0;
    if (e & kIn) {
        if (e & kStart) v = marker(f, kMsgStart);
        else if (e & kFirst) v = marker(f, (e & kCarryHead) ? kMsgCarried : kMsgNone);
        else v = before;
    }
    a.view[f] = v;
}

// the bytes so far, frame f included, of the message `v` names (kind Start or Carried)
__device__ __forceinline__ uint64_t message_len(const EcArgs& a, uint64_t v, uint64_t f, uint64_t plen, uint32_t conn) {
    const uint64_t g = (v >> 2) - 1;
    return a.dsum[f] + plen - a.dsum[g] + ((v & 3) == kMsgCarried ? conn_pending(a, conn) : 0);
}

template <class A>
__global__ __launch_bounds__(kBlock) void k_echo_size(A a) {
    __shared__ uint64_t s_wave[kWaves];
    const uint64_t f = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    uint64_t e = f < a.max_frames ? a.elem[f] : 0;
    uint64_t bytes = 0;
    if (e & kIn) {
        const uint32_t conn = (uint32_t)(e >> 32);
        const uint64_t v = a.view[f];
        const uint64_t plen = (e & kData) ? a.desc[f].payload_len : 0;
        const bool in_msg = (v & 3) != kMsgNone && a.bad[conn] == 0;
        if ((e & kData) && (e & kFin) && in_msg) {
            const uint64_t len = message_len(a, v, f, plen, conn);
            if ((uint32_t)f < a.first_close[conn] && !((a.flags & UVHTTP_WS_ECHO_SERVER_SEND) && len == 0)) {
                e |= kEcho;
                a.elem[f] = e;
                bytes = header_bytes(len, conn_masked(a, conn)) + len;
            }
        }
        if ((e & kLast) && in_msg && !((e & kData) && (e & kFin))) {
            const uint64_t len = message_len(a, v, f, plen, conn);
            if (len != 0) {
                a.olen[conn] = len;
                a.omark[conn] = v;
                a.ofend[conn] = (uint32_t)f;
            }
        }
        if constexpr (A::kAnswer) {
            // a PING or CLOSE is answered on its own lane: not after the first CLOSE unless the
            // flag says to go on, and never for a bad connection
            if ((e & kCtl) && a.bad[conn] == 0 &&
                ((a.flags & UVHTTP_WS_ANSWER_REPLY_AFTER_CLOSE) || (uint32_t)f <= a.first_close[conn])) {
                e |= kReply;
                a.elem[f] = e;
                bytes = 2u + (conn_masked(a, conn) ? 4u : 0u) + ctl_len(e);
            }
        }
    }
    uint64_t tot_c, tot_b;
    bool counts = (e & kEcho) != 0;
    if constexpr (A::kAnswer) counts = (e & (kEcho | kReply)) != 0;
    (void)block_scan(counts ? 1 : 0, AddOp(), 0, s_wave, &tot_c);
    (void)block_scan(bytes, AddOp(), 0, s_wave, &tot_b);
    if (threadIdx.x == 0) {
        a.agg_cnt[blockIdx.x] = tot_c;
        a.agg_bytes[blockIdx.x] = tot_b;
    }
    if constexpr (A::kAnswer) {
        uint64_t tot_r;
        (void)block_scan((e & kReply) ? (1ull << kRepShift) | ctl_len(e) : 0, AddOp(), 0, s_wave, &tot_r);
        if (threadIdx.x == 0) a.agg_rep[blockIdx.x] = tot_r;
    }
}

// record j lies at [o, o + n) of its output: it is the record of every tile that starts inside
__device__ __forceinline__ void map_tiles(uint32_t* map, uint32_t j, uint64_t o, uint64_t n) {
    for (uint64_t t = (o + kTile - 1) / kTile; t * kTile < o + n; ++t) map[t] = j;
}

template <class A>
__global__ __launch_bounds__(kBlock) void k_echo_offsets(A a) {
    __shared__ uint64_t s_wave[kWaves];
    const uint64_t f = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    const uint64_t e = f < a.max_frames ? a.elem[f] : 0;
    bool echo = (e & kEcho) != 0;  // an answer: an echo, or (the answers') a reply
    const uint32_t conn = (uint32_t)(e >> 32);
    uint64_t v = 0, len = 0, mine = 0;
    bool masked = false;
    if (echo) {
        v = a.view[f];
        len = message_len(a, v, f, a.desc[f].payload_len, conn);
        masked = conn_masked(a, conn);
        mine = header_bytes(len, masked) + len;
    }
    bool reply = false;
    if constexpr (A::kAnswer) {
        reply = (e & kReply) != 0;
        if (reply) {
            echo = true;
            len = ctl_len(e);
            masked = conn_masked(a, conn);
            mine = 2u + (masked ? 4u : 0u) + len;
        }
    }
    uint64_t tot;
    const uint64_t cnt = (blockIdx.x ? a.agg_cnt[blockIdx.x - 1] : 0) + block_scan(echo ? 1 : 0, AddOp(), 0, s_wave, &tot);
    const uint64_t bytes = (blockIdx.x ? a.agg_bytes[blockIdx.x - 1] : 0) + block_scan(mine, AddOp(), 0, s_wave, &tot);
    bool bounds = (e & kIn) != 0;
    if constexpr (A::kRelay) bounds = bounds && a.count_only;  // (the relay's second run reads them)
    if (bounds) {
        if (e & kFirst) {
            a.cbeg[conn] = (uint32_t)(cnt - (echo ? 1 : 0));
            a.bbeg[conn] = bytes - mine;
        }
        if (e & kLast) {
            a.cend[conn] = (uint32_t)cnt;
            a.bend[conn] = bytes;
        }
    }
    if constexpr (A::kAnswer) {
        const uint64_t mine_r = reply ? (1ull << kRepShift) | len : 0;
        const uint64_t rep = (blockIdx.x ? a.agg_rep[blockIdx.x - 1] : 0) + block_scan(mine_r, AddOp(), 0, s_wave, &tot);
        if (e & kIn) {
            if (e & kFirst) a.rbeg[conn] = rep - mine_r;
            if (e & kLast) a.rend[conn] = rep;
        }
    }
    if (!echo || !totals(a).fits) return;
    // slot and offset: the running totals, or (the relay) the connection's own place in the room
    // order plus its frames before this one
    uint64_t j = cnt - 1, at = bytes - mine;
    if constexpr (A::kRelay) {
        if (a.count_only) return;
        // (a table whose ranges overlap can break a connection's counts: stay inside its own
        // slots and the totals, and let the emit see that a slot was left out)
        const uint64_t k = j - a.cbeg[conn], kb = at - a.bbeg[conn];
        const EcTotals t = totals(a);
        j = a.rcnt[conn] + k;
        at = a.rbytes[conn] + kb;
        if (k >= conn_frames(a, conn) || kb > conn_bytes(a, conn) || mine > conn_bytes(a, conn) - kb || j >= t.cnt ||
            at > t.bytes || mine > t.bytes - at)
            return;
        atomicAdd(a.written, 1u);
    }
    if constexpr (A::kAnswer) {
        if (reply) {  // one fragment, the control frame's own payload: never looked up in dsum
            a.out_off[j] = at;
            EcRec r;
            r.dbase = a.dsum[f];
            r.len = len;
            r.carry_src = 0;
            r.carry_len = 0;
            r.src0 = a.desc[f].payload_off;
            r.g = (uint32_t)f;
            r.fend = (uint32_t)f;
            r.key = masked ? a.keys[j] : 0u;
            r.hdr = (uint8_t)(masked ? 6 : 2);
            r.b0 = (uint8_t)(0x80u | ((e & kCtlClose) ? UVHTTP_WS_OPCODE_CLOSE : UVHTTP_WS_OPCODE_PONG));
            r.masked = masked ? 1 : 0;
            r.one = 1;
            r.pad = 0;
            a.rec[j] = r;
            map_tiles(a.tmap, (uint32_t)j, at, mine);
            return;
        }
    }
    const uint64_t g = (v >> 2) - 1;
    const bool carried = (v & 3) == kMsgCarried;
    a.out_off[j] = at;
    EcRec r;
    r.dbase = a.dsum[g];
    r.len = len;
    r.carry_src = carried ? a.carry_off[conn] : 0;
    r.carry_len = carried ? conn_pending(a, conn) : 0;
    r.g = (uint32_t)g;
    r.fend = (uint32_t)f;
    r.key = masked ? a.keys[j] : 0u;
    r.hdr = (uint8_t)header_bytes(len, masked);
    const uint32_t op = (a.flags & UVHTTP_WS_ECHO_SERVER_SEND) ? (uint32_t)UVHTTP_WS_OPCODE_TEXT
                        : carried ? conn_pending_opcode(a, conn) : (uint32_t)a.desc[g].opcode;
    r.b0 = (uint8_t)(0x80u | (op & 0x0Fu));
    r.masked = masked ? 1 : 0;
    r.one = g == f ? 1 : 0;
    r.src0 = a.desc[f].payload_off;
    r.pad = 0;
    a.rec[j] = r;
    map_tiles(a.tmap, (uint32_t)j, at, mine);
}

__global__ __launch_bounds__(kBlock) void k_echo_tail(EcArgs a) {
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i > a.max_echoes) return;
    const EcTotals t = totals(a);
    if (!t.fits) a.out_off[i] = 0;
    else if (i >= t.cnt) a.out_off[i] = t.bytes;
}

// which = 0: the connections' echoes (after k_echo_offsets), 1: their open bytes
__global__ __launch_bounds__(kBlock) void k_echo_creduce(EcArgs a, int which) {
    __shared__ uint64_t s_wave[kWaves];
    const uint64_t s = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    uint64_t n = 0;
    if (s < a.n_streams) n = which ? a.olen[s] : (uint64_t)(a.cend[s] - a.cbeg[s]);
    uint64_t tot;
    (void)block_scan(n, AddOp(), 0, s_wave, &tot);
    if (threadIdx.x == 0) (which ? a.agg_co : a.agg_cn)[blockIdx.x] = tot;
}

template <class A>
__global__ __launch_bounds__(kBlock) void k_echo_finish(A a) {
    __shared__ uint64_t s_wave[kWaves];
    const uint64_t s = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    const bool live = s < a.n_streams;
    const uint32_t n = live ? a.cend[s] - a.cbeg[s] : 0;
    const uint64_t ol = live ? a.olen[s] : 0;
    uint64_t tot, inc_n = 0;  // (the relay has every connection's first slot already)
    if constexpr (!A::kRelay) inc_n = (blockIdx.x ? a.agg_cn[blockIdx.x - 1] : 0) + block_scan(n, AddOp(), 0, s_wave, &tot);
    const uint64_t inc_o = (blockIdx.x ? a.agg_co[blockIdx.x - 1] : 0) + block_scan(ol, AddOp(), 0, s_wave, &tot);
    const EcTotals t = totals(a);
    [[maybe_unused]] bool closed = false;
    if (live) {
        uvhttp_ws_echo_conn_t r = {};
        if (!t.fits) {
            r.status = UVHTTP_WS_ECHO_ERR_CAPACITY;
            a.open_off[s] = 0;
            if (s == a.n_streams - 1) a.open_off[s + 1] = 0;
        } else {
            const uint32_t cs = a.cstate[s];
            const uint64_t om = a.omark[s];
            const uint32_t kind = (uint32_t)(om & 3);
            if constexpr (A::kRelay) r.first_echo = a.rcnt[s];
            else r.first_echo = (uint32_t)(inc_n - n);
            r.n_echoes = n;
            r.out_len = a.bend[s] - a.bbeg[s];
            r.open_len = ol;
            r.status = (uint8_t)(cs & 0xFFu);
            if (r.status == UVHTTP_WS_ECHO_OK && a.bad[s]) r.status = UVHTTP_WS_ECHO_BAD_RANGE;
            if (ol != 0)
                r.open_opcode = (uint8_t)(kind == kMsgStart ? (uint32_t)a.desc[(om >> 2) - 1].opcode & 0x0Fu
                                                             : conn_pending_opcode(a, (uint32_t)s));
            a.open_off[s] = inc_o - ol;
            if (s == a.n_streams - 1) a.open_off[s + 1] = inc_o;
            EcRec o = {};
            if (ol != 0) {
                const bool frames = kind != kMsgCarryOnly;
                const bool carried = kind != kMsgStart;
                o.len = ol;
                o.carry_src = carried ? a.carry_off[s] : 0;
                o.carry_len = carried ? conn_pending(a, (uint32_t)s) : 0;
                o.g = frames ? (uint32_t)((om >> 2) - 1) : 1u;  // (1, 0): no frames
                o.fend = frames ? a.ofend[s] : 0u;
                o.dbase = frames ? a.dsum[o.g] : 0;
            }
            a.orec[s] = o;
            if (a.open) map_tiles(a.omap, (uint32_t)s, inc_o - ol, ol);
        }
        if constexpr (A::kAnswer) {
            // the answer's result begins as the echo's; then closed and the replies among the answers
            static_assert(offsetof(uvhttp_ws_answer_conn_t, first_answer) == offsetof(uvhttp_ws_echo_conn_t, first_echo) &&
                              offsetof(uvhttp_ws_answer_conn_t, n_answers) == offsetof(uvhttp_ws_echo_conn_t, n_echoes) &&
                              offsetof(uvhttp_ws_answer_conn_t, out_len) == offsetof(uvhttp_ws_echo_conn_t, out_len) &&
                              offsetof(uvhttp_ws_answer_conn_t, open_len) == offsetof(uvhttp_ws_echo_conn_t, open_len) &&
                              offsetof(uvhttp_ws_answer_conn_t, status) == offsetof(uvhttp_ws_echo_conn_t, status) &&
                              offsetof(uvhttp_ws_answer_conn_t, open_opcode) == offsetof(uvhttp_ws_echo_conn_t, open_opcode),
                          "the answer result begins as the echo's");
            closed = a.first_close[s] != kNone;
            const uint64_t rp = a.rend[s] - a.rbeg[s];
            const uint32_t n_rep = (uint32_t)(rp >> kRepShift);
            const uint64_t rep_bytes = (rp & ((1ull << kRepShift) - 1)) + (uint64_t)n_rep * (conn_masked(a, (uint32_t)s) ? 6u : 2u);
            uvhttp_ws_answer_conn_t w = {};
            w.first_answer = r.first_echo;
            w.n_answers = r.n_echoes;
            w.out_len = r.out_len;
            w.open_len = r.open_len;
            w.status = r.status;
            w.open_opcode = r.open_opcode;
            if (t.fits) {
                w.closed = closed ? 1 : 0;
                w.n_replies = n_rep;
            }
            reinterpret_cast<uvhttp_ws_answer_conn_t*>(a.conn)[s] = w;
            if (a.reply_conn) {
                uvhttp_ws_reply_conn_t q = {};
                q.closed = closed ? 1 : 0;
                if (!t.fits) {
                    q.status = UVHTTP_WS_REPLY_ERR_CAPACITY;
                } else {
                    q.n_replies = n_rep;
                    q.out_len = rep_bytes > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)rep_bytes;
                    q.status = r.status == UVHTTP_WS_ECHO_BAD_RANGE ? UVHTTP_WS_REPLY_BAD_RANGE
                               : r.status == UVHTTP_WS_ECHO_NO_KEYS ? UVHTTP_WS_REPLY_NO_KEYS : UVHTTP_WS_REPLY_OK;
                }
                a.reply_conn[s] = q;
            }
        } else {
            a.conn[s] = r;
        }
        if (a.runs) {
            uint32_t* run = reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(a.runs) + s * a.run_stride);
            run[0] = r.first_echo;
            run[1] = r.n_echoes;
        }
    }
    if constexpr (A::kAnswer) {
        uvhttp_ws_answer_summary_t* sum = reinterpret_cast<uvhttp_ws_answer_summary_t*>(a.sum);
        const uint64_t mc = __ballot(closed);
        if ((threadIdx.x & 63) == 0 && mc) atomicAdd(&sum->n_closed_conns, (uint32_t)__popcll(mc));
        if (s == 0) {
            sum->out_bytes = t.bytes;
            sum->open_bytes = t.open;
            sum->n_answers = (uint32_t)t.cnt;
            sum->n_replies = a.tot_rep ? (uint32_t)(*a.tot_rep >> kRepShift) : 0u;
            sum->status = t.fits ? UVHTTP_WS_ECHO_OK : UVHTTP_WS_ECHO_ERR_CAPACITY;
        }
    } else if (s == 0) {
        a.sum->out_bytes = t.bytes;
        a.sum->open_bytes = t.open;
        a.sum->n_echoes = (uint32_t)t.cnt;
        a.sum->status = t.fits ? UVHTTP_WS_ECHO_OK : UVHTTP_WS_ECHO_ERR_CAPACITY;
    }
}

// ---- the relay's order -----------------------------------------------------------------------------
// The connections sorted by (min(room, n_rooms), index): a least-significant-digit radix sort of
// 8 bits a pass over the bits n_rooms needs.  A pass is k_relay_hist (a workgroup's 256 keys ->
// its count per digit, stored digit-major, so that one exclusive scan of the whole table gives
// every (digit, workgroup) its base), the scan (k_relay_hreduce, k_scan_top, k_relay_hscan) and
// k_relay_scatter, which ranks a key among the equal digits before it in its workgroup: stable,
// so equal rooms keep index order.  Every kernel takes the first workgroup of its piece.

__global__ __launch_bounds__(kBlock) void k_relay_hist(RlArgs a, uint64_t base, uint32_t shift, int from) {
    __shared__ uint32_t s_h[kBlock];
    const uint64_t b = base + blockIdx.x, nblk = ((uint64_t)a.n_streams + kBlock - 1) / kBlock;
    const uint64_t p = b * kBlock + threadIdx.x;
    s_h[threadIdx.x] = 0;
    __syncthreads();
    if (p < a.n_streams) atomicAdd(&s_h[(a.skey[from][p] >> shift) & 255u], 1u);
    __syncthreads();
    a.hist[(uint64_t)threadIdx.x * nblk + b] = s_h[threadIdx.x];
}

__global__ __launch_bounds__(kBlock) void k_relay_hreduce(RlArgs a, uint64_t base) {
    __shared__ uint64_t s_wave[kWaves];
    const uint64_t b = base + blockIdx.x;
    uint64_t tot;
    (void)block_scan(a.hist[b * kBlock + threadIdx.x], AddOp(), 0, s_wave, &tot);
    if (threadIdx.x == 0) a.agg_h[b] = tot;
}

__global__ __launch_bounds__(kBlock) void k_relay_hscan(RlArgs a, uint64_t base) {
    __shared__ uint64_t s_wave[kWaves];
    const uint64_t b = base + blockIdx.x;
    const uint32_t v = a.hist[b * kBlock + threadIdx.x];
    uint64_t tot;
    const uint64_t inc = (b ? a.agg_h[b - 1] : 0) + block_scan(v, AddOp(), 0, s_wave, &tot);
    a.hist[b * kBlock + threadIdx.x] = (uint32_t)(inc - v);
}

__global__ __launch_bounds__(kBlock) void k_relay_scatter(RlArgs a, uint64_t base, uint32_t shift, int from) {
    __shared__ uint32_t s_cnt[kWaves][kBlock];
    const uint64_t b = base + blockIdx.x, nblk = ((uint64_t)a.n_streams + kBlock - 1) / kBlock;
    const uint64_t p = b * kBlock + threadIdx.x;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < kWaves; ++k) s_cnt[k][threadIdx.x] = 0;
    const bool live = p < a.n_streams;
    const uint32_t key = live ? a.skey[from][p] : 0u, idx = live ? a.sidx[from][p] : 0u;
    const uint32_t d = (key >> shift) & 255u;
    uint64_t peers = __ballot(live);  // the wave's live lanes with this lane's digit
#pragma unroll
    for (int bit = 0; bit < 8; ++bit) {
        const bool set = (d >> bit) & 1u;
        const uint64_t m = __ballot(live && set);
        peers &= set ? m : ~m;
    }
    const uint32_t below = (uint32_t)__popcll(peers & ((1ull << lane) - 1));
    __syncthreads();
    if (live && below == 0) s_cnt[w][d] = (uint32_t)__popcll(peers);
    __syncthreads();
    if (!live) return;
    uint32_t rank = below;
    for (int k = 0; k < w; ++k) rank += s_cnt[k][d];
    const uint64_t to = (uint64_t)a.hist[(uint64_t)d * nblk + b] + rank;
    a.skey[from ^ 1][to] = key;
    a.sidx[from ^ 1][to] = idx;
}

// frames and bytes of the connection at place p of the order
__device__ __forceinline__ void place_sizes(const RlArgs& a, uint64_t p, uint32_t* s, uint64_t* n, uint64_t* bytes) {
    *s = 0;
    *n = *bytes = 0;
    if (p >= a.n_streams) return;
    *s = a.oidx[p];
    *n = conn_frames(a, *s);
    *bytes = conn_bytes(a, *s);
}

__global__ __launch_bounds__(kBlock) void k_relay_oreduce(RlArgs a, uint64_t base) {
    __shared__ uint64_t s_wave[kWaves];
    const uint64_t b = base + blockIdx.x;
    uint32_t s;
    uint64_t n, bytes, tot_n, tot_b;
    place_sizes(a, b * kBlock + threadIdx.x, &s, &n, &bytes);
    (void)block_scan(n, AddOp(), 0, s_wave, &tot_n);
    (void)block_scan(bytes, AddOp(), 0, s_wave, &tot_b);
    if (threadIdx.x == 0) {
        a.agg_pc[b] = tot_n;
        a.agg_pb[b] = tot_b;
    }
}

__global__ __launch_bounds__(kBlock) void k_relay_obase(RlArgs a, uint64_t base) {
    __shared__ uint64_t s_wave[kWaves];
    const uint64_t b = base + blockIdx.x, p = b * kBlock + threadIdx.x;
    uint32_t s;
    uint64_t n, bytes, tot;
    place_sizes(a, p, &s, &n, &bytes);
    const uint64_t inc_n = (b ? a.agg_pc[b - 1] : 0) + block_scan(n, AddOp(), 0, s_wave, &tot);
    const uint64_t inc_b = (b ? a.agg_pb[b - 1] : 0) + block_scan(bytes, AddOp(), 0, s_wave, &tot);
    if (p >= a.n_streams) return;
    a.pcnt[p] = inc_n - n;
    a.pbytes[p] = inc_b - bytes;
    a.rcnt[s] = (uint32_t)(inc_n - n);
    a.rbytes[s] = inc_b - bytes;
    if (p == (uint64_t)a.n_streams - 1) {
        a.pcnt[p + 1] = inc_n;
        a.pbytes[p + 1] = inc_b;
    }
}

// the first place of the order whose key is >= x
__device__ __forceinline__ uint64_t first_ge(const uint32_t* keys, uint64_t n, uint32_t x) {
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (keys[mid] < x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// one lane per room: its run of frames and their bytes from the places where its key begins and
// ends, senders or not (all 0 on capacity)
__global__ __launch_bounds__(kBlock) void k_relay_rooms(RlArgs a, uint64_t base) {
    const uint64_t r = (base + blockIdx.x) * kBlock + threadIdx.x;
    if (r >= a.n_rooms) return;
    uvhttp_ws_relay_room_t o = {};
    if (a.n_streams != 0 && totals(a).fits) {
        const uint64_t lo = first_ge(a.okey, a.n_streams, (uint32_t)r);
        const uint64_t hi = first_ge(a.okey, a.n_streams, (uint32_t)r + 1);
        o.first_frame = (uint32_t)a.pcnt[lo];
        o.n_frames = (uint32_t)(a.pcnt[hi] - a.pcnt[lo]);
        o.out_off = a.pbytes[lo];
        o.out_len = a.pbytes[hi] - a.pbytes[lo];
    }
    a.rooms[r] = o;
}

// one lane per receiver: its room's run where uvhttp_tls_gpu_seal_frames reads it
__global__ __launch_bounds__(kBlock) void k_relay_recv(RlArgs a, uint64_t base) {
    const uint64_t k = (base + blockIdx.x) * kBlock + threadIdx.x;
    if (k >= a.n_receivers) return;
    uint32_t first = 0, n = 0;
    const uint32_t r = a.recv_room[k];
    if (r < a.n_rooms) {
        first = a.rooms[r].first_frame;
        n = a.rooms[r].n_frames;
    } else {
        atomicAdd(&a.sum->reserved[1], 1u);  // uvhttp_ws_relay_summary_t: n_bad_receivers
    }
    uint32_t* run = reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(a.sends) + k * a.send_stride);
    run[0] = first;
    run[1] = n;
}

// ---- the emit ------------------------------------------------------------------------------------

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ uint32_t rotr32(uint32_t x, uint32_t s) { return s ? (x >> s) | (x << (32u - s)) : x; }

// 16 bytes at any alignment; the caller has checked that they lie inside the buffer
__device__ __forceinline__ u32x4 load16_any(const uint8_t* p) {
    u32x4 r;
    __builtin_memcpy(&r, p, 16);
    return r;
}

// byte i of the record's header image (uvhttp_ws_build_frame: flags + opcode, mask bit + length
// code, the extended length big-endian, the key)
__device__ __forceinline__ uint32_t header_byte(const EcRec& r, uint32_t i) {
    const uint32_t base = r.hdr - (r.masked ? 4u : 0u);
    if (i == 0) return r.b0;
    if (i == 1) return (r.masked ? 0x80u : 0u) | (base == 2 ? (uint32_t)r.len : base == 4 ? 126u : 127u);
    if (i < base) return (uint32_t)(r.len >> (8 * (base - 1 - i))) & 0xFFu;
    return (r.key >> (8 * (i - base))) & 0xFFu;
}

// the last index in [lo, hi] whose entry is <= x (entries ascend; the caller knows t[lo] <= x)
__device__ __forceinline__ uint64_t last_le(const uint64_t* t, uint64_t lo, uint64_t hi, uint64_t x) {
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo + 1) / 2;
        if (t[mid] <= x) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// the unmasked payload byte at message offset m of record r (0 where a broken table leaves none).
// kOne (the answers'): a record with one fragment takes it from src0 — a control frame's payload
// is not counted in dsum, so it must never be searched for there
template <bool kOne>
__device__ __forceinline__ uint32_t payload_byte(const EcArgs& a, const EcRec& r, uint64_t m) {
    if (m < r.carry_len) return a.carry[r.carry_src + m];
    if constexpr (kOne) {
        if (r.one) return a.wire[r.src0 + (m - r.carry_len)];
    }
    if (r.g > r.fend) return 0;
    const uint64_t q = r.dbase + (m - r.carry_len);
    const uint64_t i = last_le(a.dsum, r.g, r.fend, q);
    const uint64_t within = q - a.dsum[i];
    if (!(a.elem[i] & kData)) return 0;
    const uvhttp_ws_frame_desc_t& d = a.desc[i];
    return within < d.payload_len ? a.wire[d.payload_off + within] : 0u;
}

// the output's destination, offset table and records, and its end inside this tile
struct EcDst {
    uint8_t* dst;
    const uint64_t* offs;
    const EcRec* recs;
    uint64_t n_rec, hi;
};

// one vector the long way: its source frame by a search over dsum when it is payload of one
// fragment, else byte by byte — header bytes, a join of two sources or of two records, or the
// output's last bytes
template <bool kOne>
__device__ __forceinline__ void emit_vector(const EcArgs& a, const EcDst& o, uint64_t x, uint64_t ri) {
    EcRec r = o.recs[ri];
    uint64_t r_off = o.offs[ri];
    const uint64_t rel = x - r_off;
    if (rel >= r.hdr && rel + 16 <= r.hdr + r.len) {  // the whole vector is payload of one record
        const uint64_t m = rel - r.hdr;
        const uint8_t* src = nullptr;
        if (m + 16 <= r.carry_len) {
            src = a.carry + r.carry_src + m;
        } else if (kOne && m >= r.carry_len && r.one) {
            src = a.wire + r.src0 + (m - r.carry_len);
        } else if (m >= r.carry_len && r.g <= r.fend) {
            const uint64_t q = r.dbase + (m - r.carry_len);
            const uint64_t i = last_le(a.dsum, r.g, r.fend, q);
            const uint64_t within = q - a.dsum[i];
            if (a.elem[i] & kData) {
                const uvhttp_ws_frame_desc_t& d = a.desc[i];
                if (within + 16 <= d.payload_len) src = a.wire + d.payload_off + within;
            }
        }
        if (src) {  // ... and of one source
            u32x4 w = load16_any(src);
            if (r.masked) {
                const uint32_t rk = rotr32(r.key, 8u * (uint32_t)(m & 3u));
                w ^= u32x4{rk, rk, rk, rk};
            }
            *reinterpret_cast<u32x4*>(o.dst + x) = w;
            return;
        }
    }
    const uint32_t nb = o.hi - x < 16 ? (uint32_t)(o.hi - x) : 16u;
    uint32_t w[4] = {0, 0, 0, 0};
    for (uint32_t b = 0; b < nb; ++b) {
        const uint64_t p = x + b;
        while (ri + 1 < o.n_rec && o.offs[ri + 1] <= p) {
            ++ri;
            r = o.recs[ri];
            r_off = o.offs[ri];
        }
        const uint64_t q = p - r_off;
        uint32_t v;
        if (q < r.hdr) {
            v = header_byte(r, (uint32_t)q);
        } else {
            const uint64_t m = q - r.hdr;
            v = m < r.len ? payload_byte<kOne>(a, r, m) : 0u;
            if (r.masked) v ^= (r.key >> (8 * (uint32_t)(m & 3u))) & 0xFFu;
        }
        w[b >> 2] |= (v & 0xFFu) << (8 * (b & 3));
    }
    if (nb == 16) {
        *reinterpret_cast<u32x4*>(o.dst + x) = u32x4{w[0], w[1], w[2], w[3]};
    } else {
        for (uint32_t b = 0; b < nb; ++b) o.dst[x + b] = (uint8_t)(w[b >> 2] >> (8 * (b & 3)));
    }
}

template <class A>
__global__ __launch_bounds__(kBlock) void k_echo_emit(A a, uint64_t tile_base, uint64_t tiles_out) {
    const EcTotals t = totals(a);
    if (!t.fits) return;
    if constexpr (A::kRelay) {
        if (*a.written != t.cnt) return;  // (a broken table left a slot without its record)
    }
    uint64_t tile = tile_base + blockIdx.x;
    const bool to_open = tile >= tiles_out;
    if (to_open) tile -= tiles_out;
    const uint64_t total = to_open ? t.open : t.bytes;
    const uint64_t lo = tile * kTile;
    if (lo >= total) return;
    EcDst o;
    o.hi = lo + kTile < total ? lo + kTile : total;
    o.dst = to_open ? a.open : a.out;
    o.offs = to_open ? a.open_off : a.out_off;
    o.recs = to_open ? a.orec : a.rec;
    o.n_rec = to_open ? a.n_streams : t.cnt;  // >= 1: total != 0
    // the records of the tile's first byte and of the next tile's (k_echo_offsets / _finish wrote
    // them down): every vector's record lies between
    const uint32_t* map = to_open ? a.omap : a.tmap;
    uint64_t r_lo = map[tile];
    uint64_t r_hi = lo + kTile < total ? map[tile + 1] : o.n_rec - 1;
    if (r_hi > o.n_rec - 1) r_hi = o.n_rec - 1;  // (a table whose ranges overlap: stay inside)
    if (r_lo > r_hi) r_lo = r_hi;

    // a whole tile that is payload of one record from one source (large messages): one record
    // read for the workgroup, then every lane's kVecPerLane loads in flight before its stores
    if (r_lo == r_hi && o.hi - lo == kTile) {
        const EcRec r = o.recs[r_lo];
        const uint64_t r_off = o.offs[r_lo];
        if (lo >= r_off + r.hdr && o.hi <= r_off + r.hdr + r.len) {
            const uint64_t m = lo - r_off - r.hdr;
            const uint8_t* base = nullptr;
            if (m + kTile <= r.carry_len) base = a.carry + r.carry_src + m;
            else if (m >= r.carry_len && r.one) base = a.wire + r.src0 + (m - r.carry_len);
            if (base) {
                const uint32_t rk = r.masked ? rotr32(r.key, 8u * (uint32_t)(m & 3u)) : 0u;  // every vector's: 16 | its offset
                u32x4 w[kVecPerLane];
#pragma unroll
                for (int k = 0; k < kVecPerLane; ++k) w[k] = load16_any(base + ((uint64_t)k * kBlock + threadIdx.x) * 16);
#pragma unroll
                for (int k = 0; k < kVecPerLane; ++k)
                    *reinterpret_cast<u32x4*>(o.dst + lo + ((uint64_t)k * kBlock + threadIdx.x) * 16) = w[k] ^ u32x4{rk, rk, rk, rk};
                return;
            }
        }
    }

    // else kBatch vectors side by side, so that their loads overlap: the record of each (the same
    // number of search steps in every lane), the records, the sources
#pragma unroll 1
    for (int b = 0; b < kBatches; ++b) {
    const uint64_t lo_b = lo + (uint64_t)b * kBatch * kBlock * 16;
    if (lo_b >= o.hi) break;
    uint64_t x[kBatch], rl[kBatch], rh[kBatch];
#pragma unroll
    for (int k = 0; k < kBatch; ++k) {
        x[k] = lo_b + ((uint64_t)k * kBlock + threadIdx.x) * 16;
        rl[k] = r_lo;
        rh[k] = x[k] < o.hi ? r_hi : r_lo;
    }
    for (uint64_t span = r_hi - r_lo; span; span >>= 1) {
#pragma unroll
        for (int k = 0; k < kBatch; ++k) {
            if (rl[k] < rh[k]) {
                const uint64_t mid = rl[k] + (rh[k] - rl[k] + 1) / 2;
                if (o.offs[mid] <= x[k]) rl[k] = mid;
                else rh[k] = mid - 1;
            }
        }
    }
    const uint8_t* src[kBatch];
    uint32_t rk[kBatch];
#pragma unroll
    for (int k = 0; k < kBatch; ++k) {
        src[k] = nullptr;
        rk[k] = 0;
        if (x[k] >= o.hi) continue;
        const EcRec& r = o.recs[rl[k]];
        const uint64_t rel = x[k] - o.offs[rl[k]];
        const uint64_t hdr = r.hdr, len = r.len, cl = r.carry_len;
        if (rel >= hdr && rel + 16 <= hdr + len) {  // payload of one record ...
            const uint64_t m = rel - hdr;
            if (m + 16 <= cl) src[k] = a.carry + r.carry_src + m;  // ... from its carry
            else if (m >= cl && r.one) src[k] = a.wire + r.src0 + (m - cl);  // ... from its only fragment
            if (r.masked) rk[k] = rotr32(r.key, 8u * (uint32_t)(m & 3u));
        }
    }
    u32x4 w[kBatch];
#pragma unroll
    for (int k = 0; k < kBatch; ++k)
        if (src[k]) w[k] = load16_any(src[k]);
    uint32_t slow = 0;  // the vectors left for the long way
#pragma unroll
    for (int k = 0; k < kBatch; ++k) {
        if (src[k]) *reinterpret_cast<u32x4*>(o.dst + x[k]) = w[k] ^ u32x4{rk[k], rk[k], rk[k], rk[k]};
        else if (x[k] < o.hi) slow |= 1u << k;
    }
#pragma unroll 1
    for (int k = 0; k < kBatch; ++k) {
        if (!(slow >> k & 1u)) continue;
        static_assert(kBatch == 4, "the selects below");
        const uint64_t ri = k == 0 ? rl[0] : k == 1 ? rl[1] : k == 2 ? rl[2] : rl[3];
        emit_vector<A::kAnswer>(a, o, lo_b + ((uint64_t)k * kBlock + threadIdx.x) * 16, ri);
    }
    }
}

template <class A>
void ec_carve(Carver& c, A& a, uint64_t nb, uint64_t ns, uint64_t tiles_out, uint64_t tiles_open) {
    const uint64_t F = a.max_frames, S = a.n_streams;
    a.elem = c.take<uint64_t>(F);
    a.dsum = c.take<uint64_t>(F);
    a.view = c.take<uint64_t>(F);
    a.agg_mark = c.take<uint64_t>(nb);
    a.agg_d = c.take<uint64_t>(nb);
    a.agg_post = c.take<uint64_t>(nb);
    a.agg_cnt = c.take<uint64_t>(nb);
    a.agg_bytes = c.take<uint64_t>(nb);
    a.agg_cn = c.take<uint64_t>(ns);
    a.agg_co = c.take<uint64_t>(ns);
    a.bbeg = c.take<uint64_t>(S);
    a.bend = c.take<uint64_t>(S);
    a.olen = c.take<uint64_t>(S);
    a.omark = c.take<uint64_t>(S);
    a.rec = c.take<EcRec>(a.max_echoes);
    a.orec = c.take<EcRec>(S);
    a.marks = c.take<uint32_t>(F);
    a.tmap = c.take<uint32_t>(tiles_out + 1);
    a.omap = c.take<uint32_t>(tiles_open + 1);
    a.cstate = c.take<uint32_t>(S);
    a.first_close = c.take<uint32_t>(S);
    a.bad = c.take<uint32_t>(S);
    a.cbeg = c.take<uint32_t>(S);
    a.cend = c.take<uint32_t>(S);
    a.ofend = c.take<uint32_t>(S);
    if constexpr (A::kRelay) {
        a.pcnt = c.take<uint64_t>(S + 1);
        a.pbytes = c.take<uint64_t>(S + 1);
        a.rbytes = c.take<uint64_t>(S);
        a.agg_h = c.take<uint64_t>(ns);
        a.agg_pc = c.take<uint64_t>(ns);
        a.agg_pb = c.take<uint64_t>(ns);
        a.skey[0] = c.take<uint32_t>(S);
        a.skey[1] = c.take<uint32_t>(S);
        a.sidx[0] = c.take<uint32_t>(S);
        a.sidx[1] = c.take<uint32_t>(S);
        a.hist = c.take<uint32_t>(ns * kBlock);
        a.rcnt = c.take<uint32_t>(S);
        a.written = c.take<uint32_t>(1);
    }
    if constexpr (A::kAnswer) {
        a.agg_rep = c.take<uint64_t>(nb);
        a.rbeg = c.take<uint64_t>(S);
        a.rend = c.take<uint64_t>(S);
    }
}

template <class A>
int ec_run(uvhttp_ws_gpu_engine_t* e, A a, void* stream, const char* what) {
    constexpr bool relay = A::kRelay;
    static_assert(sizeof(uvhttp_ws_echo_conn_t) == 32 && sizeof(uvhttp_ws_echo_summary_t) == 32, "ABI");
    static_assert(sizeof(uvhttp_ws_answer_conn_t) == 32 && sizeof(uvhttp_ws_answer_summary_t) == 32, "ABI");
    const uint32_t blocks = (uint32_t)(((uint64_t)a.max_frames + kBlock - 1) / kBlock);
    const uint32_t grid_s = (uint32_t)(((uint64_t)a.n_streams + kBlock - 1) / kBlock);
    const uint64_t nb = blocks ? blocks : 1, ns = grid_s ? grid_s : 1;
    const uint64_t tiles_out = (a.out_cap + kTile - 1) / kTile;
    const uint64_t tiles_open = a.open ? (a.open_cap + kTile - 1) / kTile : 0;
    Carver count{nullptr};
    ec_carve(count, a, nb, ns, tiles_out, tiles_open);

    hipStream_t s = (hipStream_t)stream;
    const int prev = uvws_call_enter(e, s);
    char* mem = static_cast<char*>(uvws_echo_scratch(e, count.bytes(), s));
    if (!mem) {
        (void)uvws_call_leave(e, prev, what);
        return uvws_set_err(e, UVHTTP_WS_GPU_ENOMEM, "echo_messages scratch (a captured call must not grow it)");
    }
    Carver carve{mem};
    ec_carve(carve, a, nb, ns, tiles_out, tiles_open);
    // radix passes: the bits of the largest key, n_rooms
    uint32_t passes = 0;
    if constexpr (relay) {
        for (uint64_t top = a.n_rooms; top; top >>= 8) ++passes;
        a.okey = a.skey[passes & 1];
        a.oidx = a.sidx[passes & 1];
    }
    if constexpr (A::kAnswer) a.tot_rep = blocks && grid_s ? a.agg_rep + (blocks - 1) : nullptr;
    const bool frames = blocks && grid_s;  // else no echo: the totals are 0
    a.tot_cnt = frames ? a.agg_cnt + (blocks - 1) : nullptr;
    a.tot_bytes = frames ? a.agg_bytes + (blocks - 1) : nullptr;
    a.tot_open = grid_s ? a.agg_co + (grid_s - 1) : nullptr;

    const EcArgs& base = a;  // the kernels the relay does not change take the echo's arguments
    hipLaunchKernelGGL((k_echo_init<A>), dim3(blocks ? blocks : 1), dim3(kBlock), 0, s, a);
    if (grid_s) hipLaunchKernelGGL((k_echo_conns<A>), dim3(grid_s), dim3(kBlock), 0, s, a);
    if (frames) {
        hipLaunchKernelGGL((k_mark_reduce<>), dim3(blocks), dim3(kBlock), 0, s, a.marks, a.max_frames, a.agg_mark, (uint64_t)0);
        hipLaunchKernelGGL((k_scan_top<LastOp>), dim3(1), dim3(kBlock), 0, s, a.agg_mark, a.agg_mark, blocks);
        // (the relay classifies as the echo does: the echo's instance)
        if constexpr (A::kAnswer) hipLaunchKernelGGL((k_echo_classify<A>), dim3(blocks), dim3(kBlock), 0, s, a);
        else hipLaunchKernelGGL((k_echo_classify<EcArgs>), dim3(blocks), dim3(kBlock), 0, s, base);
        hipLaunchKernelGGL((k_scan_top<AddOp>), dim3(1), dim3(kBlock), 0, s, a.agg_d, a.agg_d, blocks);
        hipLaunchKernelGGL((k_scan_top<LastOp>), dim3(1), dim3(kBlock), 0, s, a.agg_post, a.agg_post, blocks);
        hipLaunchKernelGGL(k_echo_prefix, dim3(blocks), dim3(kBlock), 0, s, base);
        hipLaunchKernelGGL((k_echo_size<A>), dim3(blocks), dim3(kBlock), 0, s, a);
        hipLaunchKernelGGL((k_scan_top<AddOp>), dim3(1), dim3(kBlock), 0, s, a.agg_cnt, a.agg_cnt, blocks);
        hipLaunchKernelGGL((k_scan_top<AddOp>), dim3(1), dim3(kBlock), 0, s, a.agg_bytes, a.agg_bytes, blocks);
        if constexpr (A::kAnswer) hipLaunchKernelGGL((k_scan_top<AddOp>), dim3(1), dim3(kBlock), 0, s, a.agg_rep, a.agg_rep, blocks);
    }
    if (grid_s) {
        hipLaunchKernelGGL(k_echo_creduce, dim3(grid_s), dim3(kBlock), 0, s, base, 1);
        hipLaunchKernelGGL((k_scan_top<AddOp>), dim3(1), dim3(kBlock), 0, s, a.agg_co, a.agg_co, grid_s);
    }
    if constexpr (relay) if (grid_s) {
        // every connection's frames and bytes, the order, and each connection's base in it
        if (frames) {
            a.count_only = 1;
            hipLaunchKernelGGL((k_echo_offsets<A>), dim3(blocks), dim3(kBlock), 0, s, a);
            a.count_only = 0;
        }
        for (uint32_t pass = 0; pass < passes; ++pass) {
            const uint32_t shift = 8 * pass;
            const int from = (int)(pass & 1);
            engine_grid_chunks(e, grid_s, [&](uint32_t grid, uint64_t tb) {
                hipLaunchKernelGGL(k_relay_hist, dim3(grid), dim3(kBlock), 0, s, a, tb, shift, from);
            });
            engine_grid_chunks(e, grid_s, [&](uint32_t grid, uint64_t tb) {
                hipLaunchKernelGGL(k_relay_hreduce, dim3(grid), dim3(kBlock), 0, s, a, tb);
            });
            hipLaunchKernelGGL((k_scan_top<AddOp>), dim3(1), dim3(kBlock), 0, s, a.agg_h, a.agg_h, grid_s);
            engine_grid_chunks(e, grid_s, [&](uint32_t grid, uint64_t tb) {
                hipLaunchKernelGGL(k_relay_hscan, dim3(grid), dim3(kBlock), 0, s, a, tb);
            });
            engine_grid_chunks(e, grid_s, [&](uint32_t grid, uint64_t tb) {
                hipLaunchKernelGGL(k_relay_scatter, dim3(grid), dim3(kBlock), 0, s, a, tb, shift, from);
            });
        }
        engine_grid_chunks(e, grid_s, [&](uint32_t grid, uint64_t tb) {
            hipLaunchKernelGGL(k_relay_oreduce, dim3(grid), dim3(kBlock), 0, s, a, tb);
        });
        hipLaunchKernelGGL((k_scan_top<AddOp>), dim3(1), dim3(kBlock), 0, s, a.agg_pc, a.agg_pc, grid_s);
        hipLaunchKernelGGL((k_scan_top<AddOp>), dim3(1), dim3(kBlock), 0, s, a.agg_pb, a.agg_pb, grid_s);
        engine_grid_chunks(e, grid_s, [&](uint32_t grid, uint64_t tb) {
            hipLaunchKernelGGL(k_relay_obase, dim3(grid), dim3(kBlock), 0, s, a, tb);
        });
    }
    if (frames) hipLaunchKernelGGL((k_echo_offsets<A>), dim3(blocks), dim3(kBlock), 0, s, a);
    const uint32_t grid_t = (uint32_t)(((uint64_t)a.max_echoes + 1 + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(k_echo_tail, dim3(grid_t), dim3(kBlock), 0, s, base);
    if constexpr (relay) {
        engine_grid_chunks(e, ((uint64_t)a.n_rooms + kBlock - 1) / kBlock, [&](uint32_t grid, uint64_t tb) {
            hipLaunchKernelGGL(k_relay_rooms, dim3(grid), dim3(kBlock), 0, s, a, tb);
        });
        engine_grid_chunks(e, ((uint64_t)a.n_receivers + kBlock - 1) / kBlock, [&](uint32_t grid, uint64_t tb) {
            hipLaunchKernelGGL(k_relay_recv, dim3(grid), dim3(kBlock), 0, s, a, tb);
        });
    }
    if (grid_s) {
        if constexpr (!relay) {
            hipLaunchKernelGGL(k_echo_creduce, dim3(grid_s), dim3(kBlock), 0, s, base, 0);
            hipLaunchKernelGGL((k_scan_top<AddOp>), dim3(1), dim3(kBlock), 0, s, a.agg_cn, a.agg_cn, grid_s);
        }
        hipLaunchKernelGGL((k_echo_finish<A>), dim3(grid_s), dim3(kBlock), 0, s, a);
        engine_grid_chunks(e, tiles_out + tiles_open, [&](uint32_t grid, uint64_t tb) {
            hipLaunchKernelGGL((k_echo_emit<A>), dim3(grid), dim3(kBlock), 0, s, a, tb, tiles_out);
        });
    }
    return uvws_call_leave(e, prev, what);
}

int ec_check(uvhttp_ws_gpu_engine_t* e, const EcArgs& a, const char* null_msg, const char* align_msg,
             const char* size_msg) {
    if (!a.desc || !a.out_off || !a.open_off || !a.conn || !a.sum || (!a.wire && a.wire_len) ||
        (!a.out && a.out_cap) || (a.streams ? !a.results : !a.bsum))
        return uvws_set_err(e, UVHTTP_WS_GPU_EINVAL, null_msg);
    if (((uintptr_t)a.wire & 15u) || ((uintptr_t)a.out & 15u) || ((uintptr_t)a.open & 15u) ||
        ((uintptr_t)a.carry & 15u) || ((uintptr_t)a.desc & 7u) || ((uintptr_t)a.streams & 7u) ||
        ((uintptr_t)a.results & 7u) || ((uintptr_t)a.bsum & 7u) || ((uintptr_t)a.out_off & 7u) ||
        ((uintptr_t)a.carry_off & 7u) || ((uintptr_t)a.open_off & 7u) || ((uintptr_t)a.keys & 3u) ||
        ((uintptr_t)a.runs & 3u) || ((uintptr_t)a.conn & 7u) || ((uintptr_t)a.sum & 7u))
        return uvws_set_err(e, UVHTTP_WS_GPU_EINVAL, align_msg);
    if (a.max_frames > (1u << 28) || a.max_echoes > (1u << 28) || a.n_streams > (1u << 31) ||
        (a.runs && (a.run_stride < 8 || (a.run_stride & 3u))))
        return uvws_set_err(e, UVHTTP_WS_GPU_EINVAL, size_msg);
    return UVHTTP_WS_GPU_OK;
}

}  // namespace

extern "C" int uvhttp_ws_gpu_echo_messages_streams(
    uvhttp_ws_gpu_engine_t* e, const uint8_t* d_wire, uint64_t wire_len, const uvhttp_ws_frame_desc_t* d_desc,
    uint32_t max_frames, const uvhttp_ws_stream_t* d_streams, const uvhttp_ws_stream_result_t* d_results,
    uint32_t n_streams, const uint8_t* d_enable, const uint32_t* d_mask_keys, uint32_t flags, const uint8_t* d_carry,
    uint64_t carry_len, const uint64_t* d_carry_off, uint8_t* d_out, uint64_t out_cap, uint64_t* d_out_off,
    uint32_t max_echoes, uint32_t* d_runs, uint32_t run_stride, uint8_t* d_open, uint64_t open_cap,
    uint64_t* d_open_off, uvhttp_ws_echo_conn_t* d_conn, uvhttp_ws_echo_summary_t* d_summary, void* stream) {
    if (!e) return UVHTTP_WS_GPU_EINVAL;
    if (!d_streams) return uvws_set_err(e, UVHTTP_WS_GPU_EINVAL, "echo_messages_streams: NULL argument");
    EcArgs a = {};
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
    a.carry = d_carry;
    a.carry_len = carry_len;
    a.carry_off = d_carry_off;
    a.out = d_out;
    a.out_cap = out_cap;
    a.out_off = d_out_off;
    a.max_echoes = max_echoes;
    a.runs = d_runs;
    a.run_stride = run_stride;
    a.open = d_open;
    a.open_cap = open_cap;
    a.open_off = d_open_off;
    a.conn = d_conn;
    a.sum = d_summary;
    const int rc = ec_check(e, a, "echo_messages_streams: NULL argument", "echo_messages_streams: misaligned argument",
                            "echo_messages_streams: max_frames or max_echoes > 2^28, n_streams > 2^31 or a bad run_stride");
    if (rc != UVHTTP_WS_GPU_OK) return rc;
    return ec_run(e, a, stream, "echo_messages_streams launch");
}

extern "C" int uvhttp_ws_gpu_echo_messages_inplace(
    uvhttp_ws_gpu_engine_t* e, const uint8_t* d_wire, uint64_t wire_len, const uvhttp_ws_frame_desc_t* d_desc,
    uint32_t n_frames, const uvhttp_ws_batch_summary_t* d_batch_summary, int32_t is_server,
    const uint32_t* d_mask_keys, uint32_t flags, uint8_t* d_out, uint64_t out_cap, uint64_t* d_out_off,
    uint32_t max_echoes, uint32_t* d_runs, uint32_t run_stride, uint8_t* d_open, uint64_t open_cap,
    uint64_t* d_open_off, uvhttp_ws_echo_conn_t* d_conn, uvhttp_ws_echo_summary_t* d_summary, void* stream) {
    if (!e) return UVHTTP_WS_GPU_EINVAL;
    EcArgs a = {};
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
    a.max_echoes = max_echoes;
    a.runs = d_runs;
    a.run_stride = run_stride;
    a.open = d_open;
    a.open_cap = open_cap;
    a.open_off = d_open_off;
    a.conn = d_conn;
    a.sum = d_summary;
    const int rc = ec_check(e, a, "echo_messages_inplace: NULL argument", "echo_messages_inplace: misaligned argument",
                            "echo_messages_inplace: n_frames or max_echoes > 2^28 or a bad run_stride");
    if (rc != UVHTTP_WS_GPU_OK) return rc;
    return ec_run(e, a, stream, "echo_messages_inplace launch");
}

extern "C" int uvhttp_ws_gpu_relay_messages_streams(
    uvhttp_ws_gpu_engine_t* e, const uint8_t* d_wire, uint64_t wire_len, const uvhttp_ws_frame_desc_t* d_desc,
    uint32_t max_frames, const uvhttp_ws_stream_t* d_streams, const uvhttp_ws_stream_result_t* d_results,
    uint32_t n_streams, const uint8_t* d_enable, const uint32_t* d_room, uint32_t n_rooms, uint32_t flags,
    const uint8_t* d_carry, uint64_t carry_len, const uint64_t* d_carry_off, uint8_t* d_out, uint64_t out_cap,
    uint64_t* d_out_off, uint32_t max_frames_out, uvhttp_ws_relay_room_t* d_rooms, const uint32_t* d_recv_room,
    uint32_t n_receivers, uint32_t* d_sends, uint32_t send_stride, uint8_t* d_open, uint64_t open_cap,
    uint64_t* d_open_off, uvhttp_ws_echo_conn_t* d_conn, uvhttp_ws_relay_summary_t* d_summary, void* stream) {
    // k_echo_init / k_echo_finish write the summary's first four fields through the echo's type
    static_assert(sizeof(uvhttp_ws_relay_summary_t) == 32 && sizeof(uvhttp_ws_relay_room_t) == 32, "ABI");
    static_assert(offsetof(uvhttp_ws_relay_summary_t, n_frames) == offsetof(uvhttp_ws_echo_summary_t, n_echoes) &&
                      offsetof(uvhttp_ws_relay_summary_t, status) == offsetof(uvhttp_ws_echo_summary_t, status) &&
                      offsetof(uvhttp_ws_relay_summary_t, n_bad_rooms) == offsetof(uvhttp_ws_echo_summary_t, reserved) &&
                      offsetof(uvhttp_ws_relay_summary_t, n_bad_receivers) == offsetof(uvhttp_ws_echo_summary_t, reserved) + 4,
                  "the relay summary begins as the echo's");
    if (!e) return UVHTTP_WS_GPU_EINVAL;
    if (!d_streams || !d_room || (!d_rooms && n_rooms) || ((!d_recv_room || !d_sends) && n_receivers))
        return uvws_set_err(e, UVHTTP_WS_GPU_EINVAL, "relay_messages_streams: NULL argument");
    if (((uintptr_t)d_room & 3u) || ((uintptr_t)d_rooms & 7u) || ((uintptr_t)d_recv_room & 3u) || ((uintptr_t)d_sends & 3u))
        return uvws_set_err(e, UVHTTP_WS_GPU_EINVAL, "relay_messages_streams: misaligned argument");
    if (n_rooms > (1u << 28) || (d_sends && (send_stride < 8 || (send_stride & 3u))))
        return uvws_set_err(e, UVHTTP_WS_GPU_EINVAL, "relay_messages_streams: n_rooms > 2^28 or a bad send_stride");
    RlArgs a = {};
    a.wire = d_wire;
    a.wire_len = wire_len;
    a.desc = d_desc;
    a.max_frames = max_frames;
    a.n_streams = n_streams;
    a.streams = d_streams;
    a.results = d_results;
    a.enable = d_enable;
    a.flags = flags;
    a.carry = d_carry;
    a.carry_len = carry_len;
    a.carry_off = d_carry_off;
    a.out = d_out;
    a.out_cap = out_cap;
    a.out_off = d_out_off;
    a.max_echoes = max_frames_out;
    a.open = d_open;
    a.open_cap = open_cap;
    a.open_off = d_open_off;
    a.conn = d_conn;
    a.sum = reinterpret_cast<uvhttp_ws_echo_summary_t*>(d_summary);
    a.room = d_room;
    a.n_rooms = n_rooms;
    a.rooms = d_rooms;
    a.recv_room = d_recv_room;
    a.n_receivers = n_receivers;
    a.sends = d_sends;
    a.send_stride = send_stride;
    const int rc = ec_check(e, a, "relay_messages_streams: NULL argument", "relay_messages_streams: misaligned argument",
                            "relay_messages_streams: max_frames or max_frames_out > 2^28 or n_streams > 2^31");
    if (rc != UVHTTP_WS_GPU_OK) return rc;
    return ec_run(e, a, stream, "relay_messages_streams launch");
}

// ---- the answers: echoes and control replies in one run ------------------------------------------

namespace {

int an_check(uvhttp_ws_gpu_engine_t* e, const AnArgs& a, const char* flag_msg, const char* align_msg) {
    if (a.flags & ~(UVHTTP_WS_ANSWER_SERVER_SEND | UVHTTP_WS_ANSWER_REPLY_AFTER_CLOSE))
        return uvws_set_err(e, UVHTTP_WS_GPU_EINVAL, flag_msg);
    if ((uintptr_t)a.reply_conn & 3u) return uvws_set_err(e, UVHTTP_WS_GPU_EINVAL, align_msg);
    return UVHTTP_WS_GPU_OK;
}

}  // namespace

extern "C" int uvhttp_ws_gpu_answer_messages_streams(
    uvhttp_ws_gpu_engine_t* e, const uint8_t* d_wire, uint64_t wire_len, const uvhttp_ws_frame_desc_t* d_desc,
    uint32_t max_frames, const uvhttp_ws_stream_t* d_streams, const uvhttp_ws_stream_result_t* d_results,
    uint32_t n_streams, const uint8_t* d_enable, const uint32_t* d_mask_keys, uint32_t flags, const uint8_t* d_carry,
    uint64_t carry_len, const uint64_t* d_carry_off, uint8_t* d_out, uint64_t out_cap, uint64_t* d_out_off,
    uint32_t max_answers, uint32_t* d_runs, uint32_t run_stride, uint8_t* d_open, uint64_t open_cap,
    uint64_t* d_open_off, uvhttp_ws_answer_conn_t* d_conn, uvhttp_ws_answer_summary_t* d_summary,
    uvhttp_ws_reply_conn_t* d_reply_conn, void* stream) {
    static_assert(UVHTTP_WS_ANSWER_SERVER_SEND == UVHTTP_WS_ECHO_SERVER_SEND, "k_echo_size / k_echo_offsets test the echo's bit");
    if (!e) return UVHTTP_WS_GPU_EINVAL;
    if (!d_streams) return uvws_set_err(e, UVHTTP_WS_GPU_EINVAL, "answer_messages_streams: NULL argument");
    AnArgs a = {};
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
    a.carry = d_carry;
    a.carry_len = carry_len;
    a.carry_off = d_carry_off;
    a.out = d_out;
    a.out_cap = out_cap;
    a.out_off = d_out_off;
    a.max_echoes = max_answers;
    a.runs = d_runs;
    a.run_stride = run_stride;
    a.open = d_open;
    a.open_cap = open_cap;
    a.open_off = d_open_off;
    a.conn = reinterpret_cast<uvhttp_ws_echo_conn_t*>(d_conn);
    a.sum = reinterpret_cast<uvhttp_ws_echo_summary_t*>(d_summary);
    a.reply_conn = d_reply_conn;
    int rc = ec_check(e, a, "answer_messages_streams: NULL argument", "answer_messages_streams: misaligned argument",
                      "answer_messages_streams: max_frames or max_answers > 2^28, n_streams > 2^31 or a bad run_stride");
    if (rc == UVHTTP_WS_GPU_OK)
        rc = an_check(e, a, "answer_messages_streams: unknown flags", "answer_messages_streams: misaligned argument");
    if (rc != UVHTTP_WS_GPU_OK) return rc;
    return ec_run(e, a, stream, "answer_messages_streams launch");
}

extern "C" int uvhttp_ws_gpu_answer_messages_inplace(
    uvhttp_ws_gpu_engine_t* e, const uint8_t* d_wire, uint64_t wire_len, const uvhttp_ws_frame_desc_t* d_desc,
    uint32_t n_frames, const uvhttp_ws_batch_summary_t* d_batch_summary, int32_t is_server,
    const uint32_t* d_mask_keys, uint32_t flags, uint8_t* d_out, uint64_t out_cap, uint64_t* d_out_off,
    uint32_t max_answers, uint32_t* d_runs, uint32_t run_stride, uint8_t* d_open, uint64_t open_cap,
    uint64_t* d_open_off, uvhttp_ws_answer_conn_t* d_conn, uvhttp_ws_answer_summary_t* d_summary,
    uvhttp_ws_reply_conn_t* d_reply_conn, void* stream) {
    if (!e) return UVHTTP_WS_GPU_EINVAL;
    AnArgs a = {};
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
    a.max_echoes = max_answers;
    a.runs = d_runs;
    a.run_stride = run_stride;
    a.open = d_open;
    a.open_cap = open_cap;
    a.open_off = d_open_off;
    a.conn = reinterpret_cast<uvhttp_ws_echo_conn_t*>(d_conn);
    a.sum = reinterpret_cast<uvhttp_ws_echo_summary_t*>(d_summary);
    a.reply_conn = d_reply_conn;
    int rc = ec_check(e, a, "answer_messages_inplace: NULL argument", "answer_messages_inplace: misaligned argument",
                      "answer_messages_inplace: n_frames or max_answers > 2^28 or a bad run_stride");
    if (rc == UVHTTP_WS_GPU_OK)
        rc = an_check(e, a, "answer_messages_inplace: unknown flags", "answer_messages_inplace: misaligned argument");
    if (rc != UVHTTP_WS_GPU_OK) return rc;
    return ec_run(e, a, stream, "answer_messages_inplace launch");
}
