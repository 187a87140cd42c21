"""A session model for the whole-server tests (test_session_host.py, test_gpu_sessions.py): one
connection's life over SEVERAL device calls with every pass on and every piece of carried state
live at once, and the property they pin, cut invariance: wherever a connection's byte stream is
cut into calls, what the session observably does is what the reference does when fed the same
reads in one go.

Scripts.  A script is one connection's client traffic as a list of frames (`Fr`): TEXT and BINARY
messages whole or fragmented (empty fragments, PINGs and PONGs between fragments), TEXT built from
1- to 4-byte characters, sometimes an invalid sequence split over two fragments, sometimes a CLOSE
with a reason followed by more frames, sometimes a failing frame (RSV bit, unmasked, CONTINUATION
without a start).  A `Conn` puts a script on a transport: `plain` (the bytes are the wire) or `tls`
(the plaintext cut into records of 1 / 7 / 40 / 500 / 16 384 content bytes, sealed by the oracle
under one of the six key kinds, TLS 1.3 records sometimes padded).

Schedules.  A schedule is a sorted list of wire offsets at which one call ends and the next begins.
On `tls` a call hands the decoder one read per record it completes, so every schedule feeds the
same reads; on `plain` a cut is a read boundary.  `expect()` is the one-shot expectation from the
references alone: OracleConn.process_reads over those reads, _echo_ref / _replies_ref frames of
them, _utf8_frames_ref.judge of the delivered frames.  A connection leaves the session after the
call that fails, that delivers a CLOSE, or whose verdict is INVALID; the reads of later calls are
never fed, so the one-shot runs over the reads up to the end of that call, which the references
name on their own (`Expect.leave_call`).

`classify()` says, from the script only, which kinds of state a call boundary splits.

`run_session()` is the per-call loop of INTEGRATION.md, written once for two backends: `HostBackend`
(the oracle's TLS open and stream decode, the host twins of the three passes, the Python seal
reference) and `DeviceBackend` (one TlsEngine and one GpuEngine for the whole session, every pass
enqueued on one stream, one host read per call).  Both deliver through the product's
uvhttp_ws_deliver_stream into product connections.

The two sends of a connection.  A connection's echo run is sealed before its reply run, by two
seal_frames calls; the second send's `seq` is the first's `next_seq`, copied from the first call's
result table into the second sends table on the device (no host read between the two).  The host
backend does the same with two seal_frames_ref calls.

The carry across a changing set of connections.  d_open / d_open_off are the next call's d_carry /
d_carry_off as they lie only while the stream table keeps its connections; when one leaves with
bytes open, or the order changes, the driver gathers the survivors' ranges into a fresh carry on
the device and writes the offsets from the d_open_off it read at the call's end."""
import bisect
import ctypes as C

import numpy as np

import _echo_ref as ER
import _oracle as O
import _replies_ref as RR
import _tls_send_ref as TS
import _utf8_frames_ref as FR
import _utf8_ref as R

MF, MM = FR.MF, FR.MM          # max_frame_size 16 MiB, max_message_size 64 MiB
NONE = FR.NONE
SIZES = (0, 1, 2, 125, 126, 127, 300, 5000, 20000)
REC_SIZES = (1, 7, 40, 500, 16384)
BAD_VERDICTS = (R.INVALID, R.BAD_RANGE)
KINDS_WS = ("ws_hdr2", "ws_hdr4", "ws_hdr10", "ws_key", "ws_payload", "frame_edge", "utf8_char",
            "msg_open", "ctrl_after_open", "invalid_straddle")
KINDS_TLS = ("tls_header", "tls_body", "tls_tag", "tls_edge")


# ---- scripts ---------------------------------------------------------------------------------

class Fr:
    """one frame: what it is and its wire bytes (rsv: RSV1 set, so it fails)"""

    def __init__(self, op, fin, payload=b"", key=b"\x11\x22\x33\x44", masked=True, rsv=False):
        self.op, self.fin, self.payload, self.masked = op, int(bool(fin)), bytes(payload), bool(masked)
        rc, b = O.build_frame(self.payload, op, 1 if masked else 0, self.fin, key)
        assert rc > 0
        self.bytes = bytes([b[0] | 0x40]) + b[1:] if rsv else b
        self.hs = len(self.bytes) - len(self.payload) - (4 if masked else 0)  # 2 / 4 / 10


def text_bytes(rng, n):
    """n bytes of valid UTF-8 from 1- to 4-byte characters"""
    out = bytearray()
    while len(out) < n:
        c = R._char(rng).encode("utf-8")
        out += c if len(out) + len(c) <= n else b"a"
    return bytes(out)


def message(rng, op, payload, cuts, masked=True, p_ping=0.4, p_pong=0.15):
    """`payload` as one message cut at `cuts` (equal neighbours give empty fragments), PINGs of
    0-125 bytes and PONGs between its fragments"""
    edges = [0] + sorted(cuts) + [len(payload)]
    out = []
    for k in range(len(edges) - 1):
        last = k == len(edges) - 2
        out.append(Fr(op if k == 0 else 0, last, payload[edges[k]:edges[k + 1]], rng.randbytes(4), masked))
        if not last:
            if rng.random() < p_ping:
                out.append(Fr(9, 1, rng.randbytes(rng.choice([0, 1, 5, 125, rng.randint(0, 125)])),
                              rng.randbytes(4), masked))
            if rng.random() < p_pong:
                out.append(Fr(10, 1, rng.randbytes(rng.choice([0, 3, 125])), rng.randbytes(4), masked))
    return out


def random_script(rng, is_server=1, big=False, p_fail=0.12, p_close=0.15, p_invalid=0.12, p_early=0.25):
    """-> ([Fr], priority plaintext offsets): the offsets a schedule should try first (the middle of
    an invalid sequence that two fragments share, the inside of a 10-byte header, the 64 KiB mark of
    the large message)"""
    masked = bool(is_server)
    frames, marks = [], []     # marks: (frame index, offset inside that frame)
    n_msgs = rng.randint(2, 5)
    end_kind = "close" if rng.random() < p_close else "fail" if rng.random() < p_fail else None
    end_at = rng.randrange(n_msgs) if rng.random() < p_early else n_msgs
    for m in range(n_msgs + 1):
        if m == end_at and end_kind == "close":
            reason = (1000 + rng.randrange(4)).to_bytes(2, "big") + text_bytes(rng, rng.choice([0, 3, 40]))
            frames.append(Fr(8, 1, reason, rng.randbytes(4), masked))
        elif m == end_at and end_kind == "fail":
            kind = rng.choice(["rsv", "unmasked", "cont"]) if is_server else rng.choice(["rsv", "cont"])
            frames.append(Fr(0 if kind == "cont" else 2, 1, rng.randbytes(10), rng.randbytes(4),
                             masked and kind != "unmasked", kind == "rsv"))
        if m == n_msgs:
            break
        op = rng.choice([1, 1, 2])
        n = 70000 if big and m == 0 else rng.choice(SIZES[:-1]) if rng.random() < 0.93 else SIZES[-1]
        if big and m == 0:  # a 10-byte header, a fragment edge just past 64 KiB
            payload = text_bytes(rng, n) if op == 1 else rng.randbytes(n)
            cuts = [65536 + rng.randint(1, 40)] + ([rng.randint(66000, 70000)] if rng.random() < 0.5 else [])
            marks += [(len(frames), rng.randint(1, 9)), (len(frames), 65536 + rng.randint(-3, 3))]
            frames += message(rng, op, payload, cuts, masked)
            continue
        if op == 1 and rng.random() < p_invalid:
            # E2 82 ends one fragment, 'A' starts the next: INVALID only with the carried state
            head, tail = text_bytes(rng, rng.choice([0, 1, 40, 300])), text_bytes(rng, rng.choice([0, 5, 200]))
            payload = head + b"\xe2\x82" + b"A" + tail
            cuts = [len(head) + 2] + ([rng.randint(1, len(payload))] if rng.random() < 0.4 else [])
            fr = message(rng, 1, payload, cuts, masked)
            k = next(i for i, f in enumerate(fr) if f.op < 8
                     and sum(len(g.payload) for g in fr[:i + 1] if g.op < 8) == len(head) + 2)
            marks.append((len(frames) + k, len(fr[k].bytes)))
            frames += fr
            continue
        payload = text_bytes(rng, n) if op == 1 else rng.randbytes(n)
        nfrag = 1 if n == 0 or rng.random() < 0.35 else rng.randint(2, 5)
        cuts = [rng.randint(1, n) for _ in range(nfrag - 1)]
        if nfrag > 2 and rng.random() < 0.3:
            cuts[-1] = cuts[0]  # an empty fragment
        if op == 1 and n >= 8 and rng.random() < 0.5:  # one-byte fragments inside a character
            p = next((i for i in range(1, n - 4) if payload[i] >= 0xC0), None)
            if p is not None:
                cuts = [p, p + 1] + [c for c in cuts if c > p + 1][:2]
        frames += message(rng, op, payload, cuts, masked)
    starts = np.cumsum([0] + [len(f.bytes) for f in frames])
    return frames, [int(starts[i]) + o for i, o in marks]


class Conn:
    """a script on a transport; `stops` = plaintext offsets at which a TLS record must end"""

    def __init__(self, rng, frames, is_server=1, transport="plain", kind=None, join=0, stops=(),
                 rec_sizes=REC_SIZES):
        self.frames, self.is_server, self.transport, self.join = frames, is_server, transport, join
        self.plain = b"".join(f.bytes for f in frames)
        self.starts = [int(x) for x in np.cumsum([0] + [len(f.bytes) for f in frames])]
        self.priority = list(stops)
        self.records = []  # (wire start, wire end, plaintext end, content length)
        if transport == "plain":
            self.wire = self.plain
            return
        assert is_server
        kind = TS.KEY_KINDS[rng.randrange(6)] if kind is None else kind
        self.rkey, self.wkey = TS.make_key(rng, kind), TS.make_key(rng, kind)
        self.rseq0, self.wseq0 = rng.randrange(1 << 40), rng.randrange(1 << 40)
        wire, pos, stops = bytearray(), 0, sorted(set(stops))
        while pos < len(self.plain):
            n = min(len(self.plain) - pos, rng.choice(rec_sizes))
            k = bisect.bisect_right(stops, pos)
            if k < len(stops) and stops[k] < pos + n:
                n = stops[k] - pos
            pad = rng.choice([0, 0, 40]) if kind[2] == O.TLS13 and n + 40 <= 16384 else 0
            rec = O.tls_seal(self.rkey, self.rseq0 + len(self.records), 23, self.plain[pos:pos + n], pad)
            self.records.append((len(wire), len(wire) + len(rec), pos + n, n))
            wire += rec
            pos += n
        self.wire = bytes(wire)

    def plain_pos(self, off):
        """plaintext bytes the decoder has been handed once the wire is cut at `off`"""
        if self.transport == "plain":
            return off
        k = bisect.bisect_right([r[1] for r in self.records], off)
        return self.records[k - 1][2] if k else 0

    def reads(self, cuts):
        """per call, the process_data calls it makes: [[bytes]]"""
        edges = [0] + list(cuts) + [len(self.wire)]
        assert edges == sorted(set(edges)), "cuts must be distinct offsets inside the wire"
        if self.transport == "plain":
            return [[self.wire[a:b]] for a, b in zip(edges, edges[1:])]
        out = []
        for a, b in zip(edges, edges[1:]):
            out.append([self.plain[r[2] - r[3]:r[2]] for r in self.records if a < r[1] <= b])
        return out


# ---- the classifier --------------------------------------------------------------------------

def frame_states(frames):
    """per frame index i, the state after frames[:i] were delivered: (open opcode, open bytes,
    open UTF-8 sequence, the last frame was a control frame after a fragment of the open message)"""
    out, op, nbytes, acc, ctrl = [], 0, 0, b"", False
    for f in frames:
        out.append((op, nbytes, acc, ctrl))
        if f.op >= 8:
            ctrl = op != 0 and nbytes > 0
            continue
        ctrl = False
        if f.op in (1, 2):
            op, nbytes, acc = f.op, 0, b""
        if op == 1:
            v, tail = R.prefix_verdict(acc + f.payload)
            acc = (acc + f.payload)[len(acc) + len(f.payload) - tail:] if v == R.PREFIX else b""
        nbytes += len(f.payload)
        if f.fin or (f.op in (1, 2) and not f.payload):  # an empty first fragment opens nothing
            op, nbytes, acc = 0, 0, b""
    out.append((op, nbytes, acc, ctrl))
    return out


def classify(conn, off, states=None):
    """the kinds of state the call boundary at wire offset `off` splits -> set of names"""
    kinds = set()
    if conn.transport == "tls":
        k = bisect.bisect_right([r[1] for r in conn.records], off)
        if k < len(conn.records):
            a, b = conn.records[k][0], conn.records[k][1]
            kinds.add("tls_edge" if off == a else "tls_header" if off < a + 5 else
                      "tls_tag" if off > b - 16 else "tls_body")
    p = conn.plain_pos(off)
    i = bisect.bisect_right(conn.starts, p) - 1
    states = frame_states(conn.frames) if states is None else states
    if i >= len(conn.frames) or p == conn.starts[i]:
        kinds.add("frame_edge")
    else:
        f, o = conn.frames[i], p - conn.starts[i]
        kinds.add("ws_hdr%d" % f.hs if o < f.hs else "ws_key" if f.masked and o < f.hs + 4 else "ws_payload")
    op, nbytes, acc, ctrl = states[min(i, len(conn.frames))]
    if op and nbytes:
        kinds.add("msg_open")
        if ctrl:
            kinds.add("ctrl_after_open")
    if op == 1 and acc:
        kinds.add("utf8_char")
        nxt = next((f for f in conn.frames[i:] if f.op < 8 and f.payload), None)
        if nxt is not None and R.prefix_verdict(acc + nxt.payload[:1])[0] == R.INVALID:
            kinds.add("invalid_straddle")
    return kinds


def interesting_offsets(conn):
    """wire offsets within 2 bytes of every header, key, tag and character edge"""
    edges = set()
    if conn.transport == "tls":
        for a, b, _, _ in conn.records:
            edges.update((a, a + 5, b - 16, b))
    else:
        states = frame_states(conn.frames)
        for i, f in enumerate(conn.frames):
            s = conn.starts[i]
            edges.update((s, s + f.hs, s + f.hs + (4 if f.masked else 0)))
            if states[i + 1][2] or states[i][2]:
                edges.add(s + len(f.bytes))
    out = {e + d for e in edges for d in (-2, -1, 0, 1, 2)}
    return sorted(o for o in out if 0 < o < len(conn.wire))


def wire_offset(conn, p):
    """a wire offset whose plain_pos is the plaintext offset p (tls: p must be a record end)"""
    if conn.transport == "plain":
        return p
    return next(r[1] for r in conn.records if r[2] == p)


def draw_cuts(rng, conn, n_calls):
    """n_calls - 1 distinct cuts: the script's priority offsets first (each with probability
    0.6), then half of the rest from the interesting offsets, half anywhere"""
    n = min(n_calls - 1, len(conn.wire) - 1)
    cuts = set()
    for p in conn.priority:
        if len(cuts) < n and rng.random() < 0.6:
            cuts.add(wire_offset(conn, p))
    hot = interesting_offsets(conn)
    for _ in range(20 * n_calls):
        if len(cuts) >= n:
            break
        cuts.add(rng.choice(hot) if hot and rng.random() < 0.5 else rng.randint(1, len(conn.wire) - 1))
    return sorted(c for c in cuts if 0 < c < len(conn.wire))


# ---- the one-shot expectation ----------------------------------------------------------------

class Expect:
    pass


def expect(conn, cuts, echo_flags=0):
    """what the references alone say of `conn` fed in the calls `cuts` make"""
    e = Expect()
    calls = conn.reads(cuts)
    e.n_calls = len(calls)
    ends = conn.starts[1:]
    # which call delivers frame i: the call whose reads bring its last byte
    fed, e.frame_call = 0, [None] * len(conn.frames)
    probe = O.OracleConn(conn.is_server, MF, MM, record=0, wrapper=True)
    e.leave_call, e.why = None, None
    for j, reads in enumerate(calls):
        rc = probe.process_reads(reads)[0] if reads else 0
        fed += sum(map(len, reads))
        done = bisect.bisect_right(ends, fed - probe.recv_pos)
        for i in range(done):
            if e.frame_call[i] is None:
                e.frame_call[i] = j
        if rc != 0 or probe.state == 3:
            e.leave_call, e.why = j, "failed" if rc != 0 else "closed"
            break
    n_fed = e.n_calls if e.leave_call is None else e.leave_call + 1
    e.n_delivered = sum(1 for c in e.frame_call if c is not None)
    # the first frame at which the connection is INVALID, if it is delivered before it leaves
    v = FR.judge(conn.frames[:e.n_delivered], flags=FR.CHECK_CLOSE)
    e.first_invalid = None
    if v["status"] == R.INVALID:
        g = v["first_invalid"]
        e.first_invalid, e.leave_call, e.why = g, e.frame_call[g], "invalid"
        n_fed = e.leave_call + 1
        assert conn.frames[g].op == 8 or not R.is_valid(_message_bytes(conn.frames, g))
        flat = [conn.plain[:conn.starts[g]]]  # the frames before it, which are all that is delivered
    else:
        flat = [r for reads in calls[:n_fed] for r in reads]
    e.flat = flat
    orc = O.OracleConn(conn.is_server, MF, MM, record=1, wrapper=True)
    e.rc, e.calls = orc.process_reads(flat) if flat else (0, 0)
    ev = orc.events()
    e.events = [(k, a, p if k == "message" else None) for k, a, p in ev if k in ("message", "close")]
    e.recv, e.recv_size = orc.recv_bytes(), orc.recv_size
    e.frag = (orc.frag_opcode, orc.frag_size) if orc.frag_pending and orc.frag_size else (0, 0)
    msgs, still = ER.on_messages(flat, conn.is_server)
    e.messages, e.still = msgs, still
    e.echo_payloads = [(1 if echo_flags & ER.SERVER_SEND else op, p) for op, p in msgs
                       if p or not echo_flags & ER.SERVER_SEND]
    e.replies, e.closed = RR.sink_calls(flat, conn.is_server, 1, 0)
    # the control sink reference is the product's process_data: pin it to the oracle's transcript
    # of the same reads (the oracle's wrapper outlives a CLOSE, the server's does not: the
    # reference server answers nothing after the CLOSE echo)
    sunk = [(op, p) for k, op, p in ev if k in ("pong", "close_echo")]
    stop = next((n + 1 for n, (op, _) in enumerate(sunk) if op == 8), len(sunk))
    assert sunk[:stop] == e.replies
    return e


def _message_bytes(frames, g):
    """the whole bytes of the data message frame g belongs to"""
    i = j = g
    while frames[i].op not in (1, 2) and i > 0:
        i -= 1
    while not (frames[j].op < 8 and frames[j].fin) and j + 1 < len(frames):
        j += 1
    return b"".join(f.payload for f in frames[i:j + 1] if f.op < 8)


def parse_frames(b, masked):
    """[(opcode, fin, payload)] of frames back to back, the key taken off"""
    out, i = [], 0
    while i < len(b):
        n, h = b[i + 1] & 0x7F, 2
        if n == 126:
            n, h = int.from_bytes(b[i + 2:i + 4], "big"), 4
        elif n == 127:
            n, h = int.from_bytes(b[i + 2:i + 10], "big"), 10
        assert bool(b[i + 1] & 0x80) == bool(masked)
        p = b[i + h:i + h + n]
        if masked:
            k = b[i + h:i + h + 4]
            p = b[i + h + 4:i + h + 4 + n]
            p = (np.frombuffer(p, np.uint8) ^ np.resize(np.frombuffer(k, np.uint8), n)).tobytes() if n else b""
            h += 4
        assert len(p) == n
        out.append((b[i] & 0x0F, b[i] >> 7, bytes(p)))
        i += h + n
    return out


# ---- backends --------------------------------------------------------------------------------

def _state_bytes(st):
    pend, n = st
    return bytes(pend).ljust(3, b"\0")[:3] + bytes([n])


def _np(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


class HostBackend:
    """the oracle's TLS open and stream decode, the host twins of the passes, seal_frames_ref"""
    name = "host"

    def call(self, x):
        import uvhttp_amd as U
        S, o = x["S"], {}
        st = [U.Stream.from_buffer_copy(bytes(s)) for s in x["streams"]]
        read_end = None
        if x["transport"] == "tls":
            recs, res, out = O.tls_open_batch(x["wire"], x["keys"], x["tls_st"], x["max_records"], x["out_cap"])
            o["tls_res"], o["tls_recs"] = res.copy(), recs[:int(res["n_records"].sum())].copy()
            read_end = np.zeros(x["max_records"], np.uint64)
            for s in range(S):
                r, pre = res[s], x["prefixes"][s]
                begin = int(r["out_off"]) - len(pre)
                out[begin:begin + len(pre)] = np.frombuffer(pre, np.uint8)
                st[s].begin, st[s].len = begin, len(pre) + int(r["plain_len"])
                st[s].first_read, st[s].n_reads = int(r["first_record"]), int(r["n_delivered"])
                e = len(pre)
                for k in range(int(r["n_delivered"])):
                    e += int(recs[int(r["first_record"]) + k]["content_len"])
                    read_end[int(r["first_record"]) + k] = e
            wire = out[:x["out_cap"]]
        else:
            wire = x["wire"]
        stt = np.frombuffer(b"".join(bytes(s) for s in st), O.STREAM_DT).copy()
        w, desc0, first0, nd, outs = FR.oracle_decode(np.ascontiguousarray(wire), stt, read_end)
        # descriptors with one spare slot per connection: the frame a fragment check rejected,
        # which deliver_stream replays (include/uvhttp_ws_amd.h)
        desc, first, results = np.zeros(len(desc0) + S, FR.DESC_DT), [], []
        at = 0
        for s in range(S):
            first.append(at)
            desc[at:at + nd[s]] = desc0[first0[s]:first0[s] + nd[s]]
            u = outs[s]
            if int(u["reason"]) in (-7, -8):
                p = int(st[s].begin) + int(u["consumed"])
                rc, h, hs = O.parse_frame_header(bytes(w[p:p + 14]))
                assert rc == 0
                key = int.from_bytes(bytes(w[p + hs:p + hs + 4]), "little") if h.mask else 0
                desc[at + nd[s]] = (p + hs + (4 if h.mask else 0), h.payload_length, key, 0, h.opcode,
                                    (1 if h.fin else 0) | (2 if h.mask else 0), hs, 0, 0)
            results.append(U.StreamResult(
                first_frame=at, n_frames=nd[s], n_delivered=nd[s], status=int(u["rc"]),
                first_status=int(u["reason"]), calls=int(u["calls"]), consumed_bytes=int(u["consumed"]),
                recv_buffer_size=int(u["recv_size"]), pending_bytes=int(u["frag_size"]),
                buffered_end=int(u["consumed"]) + int(u["recv_pos"])))
            at += nd[s] + 1
        o.update(streams=st, wire=w, desc=desc, results=results)
        o["verdicts"] = []
        for s in range(S):
            pop, pby = x["pend"][s]
            sin = U.Utf8State.from_buffer_copy(x["state_in"][4 * s:4 * s + 4].tobytes())
            o["verdicts"].append(U.utf8_judge_frames(w, desc, first[s], nd[s], pop if pby else 0, sin,
                                                     FR.CHECK_CLOSE))
        o["usum"] = FR.summary(o["verdicts"])
        o["reply"] = RR.host_batch(U, w, desc, first, nd, x["is_server"], None, x["keys_r"], 0, x["max_replies"])
        o["echo"] = ER.host_batch(U, w, desc, first, nd, x["is_server"], None, x["keys_e"], x["echo_flags"],
                                  [(pop, b"\0" * pby) for pop, pby in x["pend"]], x["carries"], x["max_echoes"])
        if x["transport"] == "tls":
            se = x["sends"].copy()
            for s in range(S):
                se[s]["first_frame"], se[s]["n_frames"] = o["echo"]["conn"][s]["first_echo"], o["echo"]["conn"][s]["n_echoes"]
            a = TS.seal_frames_ref(o["echo"]["out"], o["echo"]["out_off"], se, x["keys"])
            sr = x["sends"].copy()
            sr["seq"] = a["results"]["next_seq"]
            for s in range(S):
                sr[s]["first_frame"], sr[s]["n_frames"] = o["reply"]["conn"][s]["first_reply"], o["reply"]["conn"][s]["n_replies"]
            b = TS.seal_frames_ref(o["reply"]["out"], o["reply"]["out_off"], sr, x["keys"])
            for name, d in (("seal_e", a), ("seal_r", b)):
                o[name] = {"results": d["results"], "summary": d["summary"], "out": d["out"]}
        return o


class DeviceBackend:
    """one TlsEngine and one GpuEngine for the whole session: every pass of a call enqueued on
    one stream, nothing read before the call's end"""
    name = "device"

    def __init__(self, torch, tls_eng, ws_eng):
        self.t, self.tls, self.ws = torch, tls_eng, ws_eng
        self.prev = None  # (ids, d_open, d_open_off, host open_off)

    def dev(self, a, pad=64):
        a = _np(a)
        d = self.t.zeros(max(16, a.size + pad), dtype=self.t.uint8, device="cuda")
        if a.size:
            d[: a.size] = self.t.from_numpy(a.copy()).to("cuda")
        return d

    def _carry(self, x):
        """(d_carry, carry_len, d_carry_off): the last call's d_open as it lies while the table
        keeps its connections, else the survivors' ranges gathered on the device"""
        t, S = self.t, x["S"]
        lens = [len(c) for c in x["carries"]]
        if self.prev is not None and self.prev[0] == x["ids"]:
            _, d_open, d_off, host_off = self.prev
            assert [host_off[s + 1] - host_off[s] for s in range(S)] == lens
            return d_open, host_off[S], d_off
        parts = []
        if self.prev is not None:
            ids, d_open, _, host_off = self.prev
            for s, i in enumerate(x["ids"]):
                if lens[s]:
                    k = ids.index(i)
                    assert host_off[k + 1] - host_off[k] == lens[s]
                    parts.append(d_open[host_off[k]:host_off[k + 1]])
        assert sum(p.numel() for p in parts) == sum(lens)
        d_carry = t.cat(parts + [t.zeros(64, dtype=t.uint8, device="cuda")])
        off = t.tensor([int(v) for v in np.cumsum([0] + lens)], dtype=t.int64, device="cuda")
        return d_carry, sum(lens), off

    def call(self, x):
        import uvhttp_amd as U
        t, S, o = self.t, x["S"], {}
        mf, me, mr = x["max_frames"], x["max_echoes"], x["max_replies"]
        ws_dev = self.dev(np.frombuffer(b"".join(bytes(s) for s in x["streams"]), np.uint8), 0)
        d_state = self.dev(x["state_in"], 0)
        d_carry, carry_len, d_coff = self._carry(x)
        d_ke = self.dev(x["keys_e"], 0) if x["keys_e"] is not None else None
        d_kr = self.dev(x["keys_r"], 0) if x["keys_r"] is not None else None
        d_open = t.zeros(x["open_cap"] + 64, dtype=t.uint8, device="cuda")
        tls = x["transport"] == "tls"
        runs_e = runs_r = None
        if tls:
            dw, d_keys, d_tst = self.dev(x["wire"]), self.dev(x["keys"], 0), self.dev(x["tls_st"], 0)
            out = t.zeros(x["out_cap"] + 64, dtype=t.uint8, device="cuda")
            read_end = t.zeros(x["max_records"], dtype=t.int64, device="cuda")
            poff = np.cumsum([0] + [len(p) for p in x["prefixes"][:-1]]).astype(np.uint64)
            psrc = self.dev(np.frombuffer(b"".join(x["prefixes"]) or b"\0", np.uint8))
            d_se, d_sr = self.dev(x["sends"], 0), self.dev(x["sends"], 0)
            runs_e, runs_r = d_se[8:], d_sr[8:]
            recs, res = self.tls.open_records(dw, d_keys, 2 * S, d_tst, S, x["max_records"], out[:x["out_cap"]],
                                              wire_len=x["wire"].size)
            self.tls.ws_streams(res, recs, S, d_tst, out, ws_dev, read_end, prefix_src=psrc, prefix_off=self.dev(poff))
            wire, wl = out, x["out_cap"]
            desc, wres = self.ws.decode_streams(wire, ws_dev, S, mf, wire_len=wl, read_end=read_end,
                                                n_reads=x["max_records"])
        else:
            wire, wl = self.dev(x["wire"]), x["wire"].size
            desc, wres = self.ws.decode_streams(wire, ws_dev, S, mf, wire_len=wl)
        v, vs = self.ws.validate_utf8_streams(wire, desc, mf, ws_dev, wres, S, state_in=d_state,
                                              flags=U.UTF8_CHECK_CLOSE, wire_len=wl)
        kw = dict(run_stride=32) if tls else {}
        rep, rep_off, rconn, rsum = self.ws.control_replies_streams(
            wire, desc, mf, ws_dev, wres, S, mr, x["reply_cap"], mask_keys=d_kr, runs=runs_r, wire_len=wl, **kw)
        ech, ech_off, open_off, econn, esum = self.ws.echo_messages_streams(
            wire, desc, mf, ws_dev, wres, S, me, x["echo_cap"], mask_keys=d_ke, flags=x["echo_flags"],
            carry=d_carry, carry_len=carry_len, carry_off=d_coff, runs=runs_e, open=d_open,
            open_cap=x["open_cap"], wire_len=wl, **kw)
        if tls:
            nre, nrr = me + x["echo_cap"] // 16384 + 1, mr + x["reply_cap"] // 16384 + 1
            sealed_e = t.zeros(x["echo_cap"] + 64 * nre, dtype=t.uint8, device="cuda")
            sealed_r = t.zeros(x["reply_cap"] + 64 * nrr, dtype=t.uint8, device="cuda")
            _, sres_e, ssum_e = self.tls.seal_frames(ech, ech_off, me, d_se, S, d_keys, 2 * S, nre, sealed_e,
                                                     frames_len=x["echo_cap"])
            # the second send starts where the first ended: next_seq -> seq, on the device
            d_sr[:32 * S].view(t.int64).view(S, 4)[:, 0] = sres_e[:48 * S].view(t.int64).view(S, 6)[:, 2]
            _, sres_r, ssum_r = self.tls.seal_frames(rep, rep_off, mr, d_sr, S, d_keys, 2 * S, nrr, sealed_r,
                                                     frames_len=x["reply_cap"])
        t.cuda.synchronize()  # the call's one host read
        self.ws.sync()
        if tls:
            o["tls_res"] = res.cpu().numpy().view(O.TLS_RESULT_DT)[:S].copy()
            o["tls_recs"] = recs.cpu().numpy().view(O.TLS_RECORD_DT)[:int(o["tls_res"]["n_records"].sum())].copy()
            o["read_end"] = read_end.cpu().numpy().view(np.uint64)
            for name, sr_, ss_, buf, d_s in (("seal_e", sres_e, ssum_e, sealed_e, d_se), ("seal_r", sres_r, ssum_r, sealed_r, d_sr)):
                summ = ss_.cpu().numpy().view(TS.TLS_SEND_SUMMARY_DT).copy()
                o[name] = {"results": sr_.cpu().numpy()[:48 * S].view(TS.TLS_SEND_RESULT_DT).copy(), "summary": summ,
                           "out": buf[:int(summ[0]["out_bytes"])].cpu().numpy().tobytes(),
                           "sends": d_s[:32 * S].cpu().numpy().view(TS.TLS_SEND_DT).copy()}
        raw = ws_dev[:64 * S].cpu().numpy().tobytes()
        o["streams"] = [U.Stream.from_buffer_copy(raw, 64 * s) for s in range(S)]
        o["wire"] = wire[:wl].cpu().numpy()
        o["results"] = self.ws.read_stream_results(wres, S)
        o["desc"] = desc.cpu().numpy()[:32 * mf].view(FR.DESC_DT).copy()
        o["verdicts"] = self.ws.read_utf8_conn_verdicts(v, S)
        o["usum"] = self.ws.read_utf8_frames_summary(vs)
        rs, es = self.ws.read_reply_summary(rsum), self.ws.read_echo_summary(esum)
        o["reply"] = {"out": rep[:rs["out_bytes"]].cpu().numpy().tobytes() if rs["status"] == 0 else b"",
                      "out_off": [int(v_) for v_ in rep_off.cpu().numpy()], "conn": self.ws.read_reply_conns(rconn, S),
                      "summary": rs}
        ok = es["status"] == 0
        host_open_off = [int(v_) for v_ in open_off.cpu().numpy()]
        o["echo"] = {"out": ech[:es["out_bytes"]].cpu().numpy().tobytes() if ok else b"",
                     "out_off": [int(v_) for v_ in ech_off.cpu().numpy()],
                     "open": d_open[:es["open_bytes"]].cpu().numpy().tobytes() if ok else b"",
                     "open_off": host_open_off, "conn": self.ws.read_echo_conns(econn, S), "summary": es}
        self.prev = (list(x["ids"]), d_open, open_off, host_open_off)
        return o


RESULT_FIELDS = ("n_delivered", "first_status", "calls", "consumed_bytes", "recv_buffer_size", "pending_bytes",
                 "buffered_end")
DESC_FIELDS = ("payload_off", "payload_len", "masking_key", "opcode", "flags", "header_size")


def assert_same_call(dev, host, x, where):
    """every output of one call, device against host, field for field and byte for byte.  The two
    lay the descriptors out differently (the host keeps a spare slot per connection), so
    first_frame and the verdict's first_invalid compare relative to the connection's first frame"""
    S = x["S"]
    if x["transport"] == "tls":
        assert dev["tls_res"].tobytes() == host["tls_res"].tobytes(), where
        assert dev["tls_recs"].tobytes() == host["tls_recs"].tobytes(), where
    for s in range(S):
        w = (where, s)
        assert bytes(dev["streams"][s]) == bytes(host["streams"][s]), w
        d, h = dev["results"][s], host["results"][s]
        assert [getattr(d, f) for f in RESULT_FIELDS] == [getattr(h, f) for f in RESULT_FIELDS], (w, d.as_dict(), h.as_dict())
        assert (d.status == 0) == (h.status == 0), w
        dd, hd = dev["desc"][d.first_frame:d.first_frame + d.n_delivered], host["desc"][h.first_frame:h.first_frame + h.n_delivered]
        for f in DESC_FIELDS:
            assert (dd[f] == hd[f]).all(), (w, f)
        st = dev["streams"][s]
        if d.status == 0:
            assert dev["wire"][st.begin:st.begin + st.len].tobytes() == host["wire"][st.begin:st.begin + st.len].tobytes(), w
        for k in range(d.n_delivered):
            a, b = int(dd[k]["payload_off"]), int(dd[k]["payload_off"] + dd[k]["payload_len"])
            assert dev["wire"][a:b].tobytes() == host["wire"][a:b].tobytes(), (w, k)
        if x["transport"] == "tls":
            for k in range(st.n_reads):
                e = sum(int(dev["tls_recs"][st.first_read + i]["content_len"]) for i in range(k + 1))
                assert int(dev["read_end"][st.first_read + k]) == len(x["prefixes"][s]) + e, (w, k)
        dv, hv = dict(dev["verdicts"][s]), dict(host["verdicts"][s])
        for v, r in ((dv, d), (hv, h)):
            if v["first_invalid"] != NONE:
                v["first_invalid"] -= r.first_frame
        assert dv == hv, (w, dv, hv)
    dus, hus = dict(dev["usum"]), dict(host["usum"])
    assert dus == hus, (where, dus, hus)
    for name in ("reply", "echo"):
        for f in host[name]:
            assert dev[name][f] == host[name][f], (where, name, f)
    if x["transport"] == "tls":
        for name, src, first, n in (("seal_e", "echo", "first_echo", "n_echoes"), ("seal_r", "reply", "first_reply", "n_replies")):
            for f in ("results", "summary"):
                assert dev[name][f].tobytes() == host[name][f].tobytes(), (where, name, f)
            assert dev[name]["out"] == host[name]["out"], (where, name)
            runs = [(int(r["first_frame"]), int(r["n_frames"])) for r in dev[name]["sends"]]
            assert runs == [(c[first], c[n]) for c in dev[src]["conn"]], (where, name)


# ---- the driver ------------------------------------------------------------------------------

class Live:
    """what a server keeps for one connection between two calls"""

    def __init__(self, U, conn, cuts):
        self.conn = conn
        self.prod = U.WsConnection(conn.is_server, MF, MM, user_data=False)
        self.prod.ptr.contents.state = ER.STATE_OPEN
        edges = [0] + list(cuts) + [len(conn.wire)]
        self.chunks = [conn.wire[a:b] for a, b in zip(edges, edges[1:])]
        self.left = b""                       # leftover ciphertext
        self.rseq = getattr(conn, "rseq0", 0)
        self.wseq = getattr(conn, "wseq0", 0)
        self.ustate = (b"", 0)                # the open UTF-8 sequence
        self.carry = b""                      # the open message's bytes (the host's copy)
        self.echoes, self.replies, self.sealed, self.verdicts = [], [], [], []
        self.calls, self.rc, self.n_frames, self.first_invalid = 0, 0, 0, None
        self.left_at, self.why = None, None

    def recv(self):
        s = self.prod.struct
        return C.string_at(s.recv_buffer, s.recv_buffer_pos) if s.recv_buffer_pos else b""


def _frames_of(batch, first, n):
    off = batch["out_off"]
    return [batch["out"][off[j]:off[j + 1]] for j in range(first, first + n)]


def run_session(backend, conns, schedules, flags=0, expect_log=None, break_driver=None):
    """the per-call loop of INTEGRATION.md over `conns` cut by `schedules`, on `backend`; `flags` =
    the echo flags.  After every call the carried state is checked (see the asserts); with
    expect_log (another backend's log) every output of every call is compared with it.
    break_driver names one deliberate mistake of the loop, for the test that proves the checks
    catch it.  -> (per-connection Live records, the log of (inputs, outputs) per call)"""
    import uvhttp_amd as U
    lives = [Live(U, c, cuts) for c, cuts in zip(conns, schedules)]
    n_calls = max(c.join + len(lv.chunks) for c, lv in zip(conns, lives))
    transport = conns[0].transport
    assert all(c.transport == transport for c in conns)
    tls = transport == "tls"
    order, log = [], []
    for j in range(n_calls):
        order = [i for i in order if lives[i].left_at is None and j - conns[i].join < len(lives[i].chunks)]
        order += [i for i, c in enumerate(conns) if c.join == j]
        if not order:
            continue
        S = len(order)
        x = {"S": S, "ids": list(order), "transport": transport, "echo_flags": flags,
             "is_server": [conns[i].is_server for i in order]}
        # 1. leftover ciphertext + new bytes (tls) / 2. buffered WebSocket bytes in front
        streams, wire, pieces = [], bytearray(), []
        x["prefixes"] = [lives[i].recv() for i in order]
        if tls:
            st = np.zeros(S, O.TLS_STREAM_DT)
            for s, i in enumerate(order):
                lv = lives[i]
                data = lv.left + lv.chunks[j - conns[i].join]
                st[s] = (len(wire), len(data), lv.rseq, s, len(x["prefixes"][s]))
                pieces.append(data)
                wire += data
                sd = U.Stream()
                U.lib().uvhttp_ws_stream_init(lv.prod.ptr, 0, 0, C.byref(sd))
                streams.append(sd)
            x["tls_st"] = st
            x["keys"] = np.concatenate([conns[i].rkey for i in order] + [conns[i].wkey for i in order])
            x["max_records"] = len(wire) // 5 + 1
            x["out_cap"] = max(16, len(wire) + sum(map(len, x["prefixes"])))
            total = x["out_cap"]
            sends = np.zeros(S, TS.TLS_SEND_DT)
            for s, i in enumerate(order):
                sends[s] = (lives[i].wseq, 0, 0, S + s, 23, 0, 0)
            x["sends"] = sends
        else:
            for s, i in enumerate(order):
                lv = lives[i]
                data = x["prefixes"][s] + lv.chunks[j - conns[i].join]
                sd = U.Stream()
                U.lib().uvhttp_ws_stream_init(lv.prod.ptr, len(wire), len(data), C.byref(sd))
                streams.append(sd)
                pieces.append(data)
                wire += data
            total = len(wire)
        x["wire"] = np.frombuffer(bytes(wire) or b"\0", np.uint8).copy()
        x["streams"] = streams
        x["pend"] = [(int(s.pending_opcode), int(s.pending_bytes)) for s in streams]
        zero = break_driver == "zero_state_in"
        x["state_in"] = np.frombuffer(b"".join(_state_bytes((b"", 0) if zero else lives[i].ustate) for i in order),
                                      np.uint8).copy()
        x["carries"] = [b"" if break_driver == "drop_carry" else lives[i].carry for i in order]
        x["max_frames"] = x["max_echoes"] = x["max_replies"] = total // 2 + S + 1
        carry_len = sum(map(len, x["carries"]))
        x["echo_cap"] = 14 * x["max_echoes"] + total + carry_len
        x["open_cap"] = total + carry_len
        x["reply_cap"] = 131 * min(x["max_replies"], total // 2 + 1) + 16
        clients = not all(x["is_server"])
        krng = np.random.default_rng(1000 + j)
        x["keys_e"] = krng.integers(0, 1 << 32, x["max_echoes"], dtype=np.uint32) if clients else None
        x["keys_r"] = krng.integers(0, 1 << 32, x["max_replies"], dtype=np.uint32) if clients else None

        o = backend.call(x)  # 3.-7. decode, validate, replies, echoes, seal
        if expect_log is not None:
            assert_same_call(o, expect_log[len(log)][1], x, (backend.name, "call", j))
        log.append((x, o))

        hw = np.ascontiguousarray(o["wire"])
        hd = np.ascontiguousarray(o["desc"])
        cw = (C.c_uint8 * max(1, hw.size)).from_buffer(hw)
        cd = (C.c_uint8 * max(1, hd.nbytes)).from_buffer(hd.view(np.uint8).reshape(-1)) if hd.size else None
        assert o["echo"]["summary"]["status"] == ER.OK and o["reply"]["summary"]["status"] == RR.OK
        for s, i in enumerate(order):
            lv, c, r, v = lives[i], conns[i], o["results"][s], o["verdicts"][s]
            w = (backend.name, "call", j, "conn", i)
            sd, ec, rp = o["streams"][s], o["echo"]["conn"][s], o["reply"]["conn"][s]
            assert ec["status"] == ER.OK and rp["status"] == RR.OK, (w, ec, rp)
            if tls:
                tr = o["tls_res"][s]
                assert tr["status"] == 0 and tr["first_status"] == 0, (w, tr)
                lv.left = pieces[s][int(tr["consumed_bytes"]):]
                lv.rseq = int(tr["next_seq"])
                if tr["n_delivered"]:
                    lv.calls += r.calls
            else:
                lv.calls += r.calls
            echoes = _frames_of(o["echo"], ec["first_echo"], ec["n_echoes"])
            replies = _frames_of(o["reply"], rp["first_reply"], rp["n_replies"])
            lv.verdicts.append(v)
            if v["status"] in BAD_VERDICTS:
                # shorten the result to the frames before first_invalid, deliver them, close 1007
                keep = v["first_invalid"] - r.first_frame
                assert 0 <= keep < r.n_delivered or (keep == r.n_delivered == 0), (w, v, r.as_dict())
                lv.first_invalid = lv.n_frames + keep
                pop, pby = x["pend"][s]

                def slots(keys, first):  # the connection's own key slots of this call
                    return None if keys is None else [int(k) for k in keys[first:first + keep + 1]]

                eb, eo, _, er = U.echo_messages(hw, hd, r.first_frame, keep, c.is_server, 1,
                                                slots(x["keys_e"], ec["first_echo"]), flags, pop, pby, x["carries"][s])
                short = [eb[eo[k]:eo[k + 1]] for k in range(er["n_echoes"])]
                assert short == echoes[:len(short)], w  # the echoes before first_invalid
                rb, ro, rr = U.control_replies(hw, hd, r.first_frame, keep, c.is_server, 1,
                                               slots(x["keys_r"], rp["first_reply"]), 0)
                short_r = [rb[ro[k]:ro[k + 1]] for k in range(rr["n_replies"])]
                assert short_r == replies[:len(short_r)], w
                lv.echoes += short
                lv.replies += short_r
                lv.n_frames += keep
                r2 = U.StreamResult.from_buffer_copy(bytes(r))
                r2.n_delivered, r2.status = keep, -1
                U.lib().uvhttp_ws_deliver_stream(lv.prod.ptr, cw, cd, C.byref(sd), C.byref(r2))
                lv.left_at, lv.why = j, "invalid"
                continue
            rc = U.lib().uvhttp_ws_deliver_stream(lv.prod.ptr, cw, cd, C.byref(sd), C.byref(r))  # 8.
            assert (rc == 0) == (r.status == 0), (w, rc, r.as_dict())
            lv.rc = rc
            lv.n_frames += r.n_delivered
            lv.echoes += echoes
            lv.replies += replies
            ps = lv.prod.struct
            frag = (ps.fragmented_opcode, ps.fragmented_size) if ps.fragmented_message and ps.fragmented_size else (0, 0)
            opened = C.string_at(ps.fragmented_message, ps.fragmented_size) if frag[1] else b""
            a, b = o["echo"]["open_off"][s], o["echo"]["open_off"][s + 1]
            if rc == 0:
                # the three outputs that must agree on what is open at the call boundary
                assert frag[1] == r.pending_bytes, (w, frag, r.as_dict())
                assert (ec["open_opcode"], ec["open_len"]) == frag, (w, ec, frag)
                assert o["echo"]["open"][a:b] == opened, w
                if frag[0] == 1:
                    assert v["status"] == R.PREFIX or (v["status"] == R.VALID and v["state"][1] == 0), (w, v)
                    tail = v["state"][1]  # the open sequence is the end of the open message
                    assert not tail or opened[len(opened) - tail:] == v["state"][0], (w, v)
                assert lv.recv() == hw[sd.begin + r.consumed_bytes:sd.begin + r.buffered_end].tobytes(), w
            lv.carry = o["echo"]["open"][a:b]
            lv.ustate = v["state"]
            if tls:
                se, sr = o["seal_e"]["results"][s], o["seal_r"]["results"][s]
                assert se["status"] == 0 and sr["status"] == 0, (w, se, sr)
                sealed = (o["seal_e"]["out"][int(se["out_off"]):int(se["out_off"] + se["out_len"])],
                          o["seal_r"]["out"][int(sr["out_off"]):int(sr["out_off"] + sr["out_len"])])
                lv.sealed.append((lv.wseq, sealed, echoes, replies))
                if break_driver != "reuse_write_seq":
                    lv.wseq = int(sr["next_seq"])
            if rc != 0 or rp["closed"]:
                lv.left_at, lv.why = j, "failed" if rc != 0 else "closed"
    return lives, log


def check_session(conns, schedules, lives, flags=0, expects=None):
    """the end of the session against the one-shot expectation, for every connection"""
    expects = expects or [expect(c, cuts, flags) for c, cuts in zip(conns, schedules)]
    for i, (c, lv, e) in enumerate(zip(conns, lives, expects)):
        w = ("conn", i, e.why, e.leave_call)
        assert (lv.why, None if lv.left_at is None else lv.left_at - c.join) == (e.why, e.leave_call), (w, lv.why, lv.left_at)
        pev = [ev for ev in lv.prod.events if ev[0] in ("message", "close")]
        assert pev == e.events, w
        masked = not c.is_server
        want_echo = [(op, 1, p) for op, p in e.echo_payloads]
        assert parse_frames(b"".join(lv.echoes), masked) == want_echo, w
        assert parse_frames(b"".join(lv.replies), masked) == [(op, 1, p) for op, p in e.replies], w
        if c.is_server:  # byte for byte, too: a server's frames carry no key
            assert lv.echoes == ER.echo_frames(e.messages, 1, None, flags), w
            assert lv.replies == RR.reply_frames(e.replies, 1, None), w
        assert lv.first_invalid == e.first_invalid, (w, lv.first_invalid, e.first_invalid)
        if e.why != "invalid":
            assert all(v["status"] not in BAD_VERDICTS for v in lv.verdicts), w
            ps = lv.prod.struct
            assert ((lv.rc == 0) == (e.rc == 0)) and lv.calls == e.calls, (w, lv.rc, e.rc, lv.calls, e.calls)
            assert lv.recv() == e.recv and ps.recv_buffer_size == e.recv_size, w
            frag = (ps.fragmented_opcode, ps.fragmented_size) if ps.fragmented_message and ps.fragmented_size else (0, 0)
            assert frag == e.frag, (w, frag, e.frag)
            if frag[1]:
                assert C.string_at(ps.fragmented_message, ps.fragmented_size) == e.still[1], w
        if c.transport == "tls":
            # everything sealed for the connection opens under the oracle as ONE record stream from
            # the starting write seq — no gap, no repeat — into each call's echoes, then its replies
            sealed = b"".join(a + b for _, (a, b), _, _ in lv.sealed)
            st = np.zeros(1, O.TLS_STREAM_DT)
            st[0] = (0, len(sealed), c.wseq0, 0, 0)
            recs, res, out = O.tls_open_batch(np.frombuffer(sealed or b"\0", np.uint8)[:len(sealed)], c.wkey, st,
                                              out_cap=len(sealed) + 16)
            r = res[0]
            assert r["status"] == 0 and r["consumed_bytes"] == len(sealed), (w, r)
            plain = out[int(r["out_off"]):int(r["out_off"] + r["plain_len"])].tobytes()
            assert plain == b"".join(b"".join(ec) + b"".join(rp) for _, _, ec, rp in lv.sealed), w
            seq = c.wseq0
            for wseq, (a, b), _, _ in lv.sealed:
                assert wseq == seq, (w, wseq, seq)
                seq += _count_records(a) + _count_records(b)
            assert int(r["next_seq"]) == seq, w
    return expects


def _count_records(b):
    n, i = 0, 0
    while i < len(b):
        i += 5 + int.from_bytes(b[i + 3:i + 5], "big")
        n += 1
    return n


def coverage(conns, schedules, expects):
    """how many call boundaries of each kind the session reaches while the connection is alive"""
    counts = {}
    for c, cuts, e in zip(conns, schedules, expects):
        states = frame_states(c.frames)
        for k, off in enumerate(cuts):
            if e.leave_call is not None and k >= e.leave_call:
                break
            for kind in classify(c, off, states):
                if kind == "invalid_straddle" and (e.why != "invalid" or k != e.leave_call - 1):
                    continue
                counts[kind] = counts.get(kind, 0) + 1
    return counts


# ---- the sessions both test files run ----------------------------------------------------------

def every_cut_session(transport):
    """one fixed script of 350-450 wire bytes; connection k is cut after byte k"""
    import random
    rng = random.Random(77)
    t = "gé世\U0001f600".encode("utf-8")  # 1-, 2-, 3- and 4-byte characters
    k = lambda: rng.randbytes(4)  # noqa: E731
    rep = 2 if transport == "plain" else 1
    frames = [Fr(1, 0, t * rep + t[:2], k()), Fr(9, 1, b"ping-1", k()), Fr(0, 0, t[2:7], k()),
              Fr(0, 1, t[7:] + t * rep, k()), Fr(2, 1, rng.randbytes(126), k()), Fr(2, 1, b"", k()),
              Fr(8, 1, (1000).to_bytes(2, "big") + "bye \u2603".encode("utf-8"), k())]
    if transport == "plain":
        frames.insert(5, Fr(2, 1, rng.randbytes(140), k()))
    starts = np.cumsum([0] + [len(f.bytes) for f in frames])
    # tls: records of 40 content bytes, and of 7 and fewer where a record must end inside the 2-byte
    # header, the 4-byte header and the key, inside a character and after the PING
    stops = [int(starts[1]) + 1, int(starts[2]), int(starts[4]) + 3, int(starts[4]) + 6,
             int(starts[4]) + 13]
    proto = Conn(random.Random(5), frames, 1, transport, TS.KEY_KINDS[5], stops=stops, rec_sizes=(40,))
    assert transport == "plain" or {7, 40} <= {r[3] for r in proto.records}
    assert 350 <= len(proto.wire) <= 450, len(proto.wire)
    cuts = range(1, len(proto.wire))  # every byte offset, none skipped
    return [proto] * len(cuts), [[cut] for cut in cuts]


def random_session(seed, transport, n_conns=32):
    """32 connections over 3-6 calls: late joiners, early leavers, one 70 000-byte message, clients
    among the plain connections"""
    import random
    rng = random.Random(9100 + 17 * seed + (0 if transport == "plain" else 5))
    n_calls = rng.randint(3, 6)
    conns, scheds = [], []
    for i in range(n_conns):
        srv = 1 if transport == "tls" or rng.random() < 0.7 else 0
        join = 0 if i < n_conns - 6 else rng.choice([1, 2]) if n_calls >= 4 else 1
        frames, prio = random_script(rng, srv, big=i == 3)
        c = Conn(rng, frames, srv, transport, join=join, stops=prio)
        conns.append(c)
        scheds.append(draw_cuts(rng, c, n_calls - join))
    return conns, scheds


def long_open_session():
    """one TEXT message of 40 fragments over 8 calls on a TLS connection: every call boundary falls
    after a one-byte fragment inside a 4-byte character (1, 2 or 3 of its bytes delivered), a PING
    comes in every call, so carry, UTF-8 state, replies and both sends are live 8 calls in a row"""
    import random
    rng = random.Random(4040)
    frames, stops, prev, kp = [], [], b"", 0
    k4 = lambda: rng.randbytes(4)  # noqa: E731
    for g in range(8):
        x, k = chr(rng.randrange(0x10000, 0x110000)).encode("utf-8"), 1 + g % 3
        a = prev[kp:kp + 1] if prev else b"a"
        b = (prev[kp + 1:] if prev else b"") + text_bytes(rng, 10)
        last = g == 7
        d, e = (text_bytes(rng, 6), b".") if last else (text_bytes(rng, 6) + x[:k - 1], x[k - 1:k])
        frames += [Fr(1 if g == 0 else 0, 0, a, k4()), Fr(0, 0, b, k4()), Fr(9, 1, b"ping %d" % g, k4()),
                   Fr(0, 0, text_bytes(rng, 20), k4()), Fr(0, 0, d, k4()), Fr(0, last, e, k4())]
        prev, kp = x, k
        if not last:
            stops.append(sum(len(f.bytes) for f in frames))
    conn = Conn(rng, frames, 1, "tls", TS.KEY_KINDS[2], stops=stops, rec_sizes=(7, 40))
    return [conn], [[wire_offset(conn, p) for p in stops]]


def check_long_open_conditions(conns, scheds, log, expects):
    c = conns[0]
    assert sum(1 for f in c.frames if f.op < 8) == 40 and len(log) == 8 and len(scheds[0]) == 7
    assert len(expects[0].messages) == 1 and R.is_valid(expects[0].messages[0][1])
    for g, off in enumerate(scheds[0]):
        assert {"msg_open", "utf8_char", "frame_edge"} <= classify(c, off), g
        o = log[g][1]
        assert o["verdicts"][0]["status"] == R.PREFIX and o["verdicts"][0]["state"][1] == 1 + g % 3, g
        assert len(c.frames[6 * g + 5].payload) == 1 and o["echo"]["conn"][0]["open_len"] > 0
    assert all(o["reply"]["conn"][0]["n_replies"] == 1 for _, o in log)
    assert [o["echo"]["conn"][0]["n_echoes"] for _, o in log] == [0] * 7 + [1]


def shapes_session():
    """calls of 300, 3, 600 and 1 live connections: 297 connections whose only call is the first,
    three that stay (one of them to the end), 597 that join at the third call"""
    import random
    rng = random.Random(606)

    def short(join):
        t = text_bytes(rng, rng.choice([1, 9, 30]))
        frames = [Fr(1, 0, t, rng.randbytes(4)), Fr(9, 1, rng.randbytes(rng.choice([0, 5])), rng.randbytes(4)),
                  Fr(0, rng.random() < 0.7, text_bytes(rng, rng.choice([0, 4])), rng.randbytes(4))]
        return Conn(rng, frames, 1, "tls", join=join, rec_sizes=(7, 40, 500))

    conns, scheds = [], []
    for i in range(3):
        frames, prio = random_script(rng, 1, p_fail=0, p_close=0, p_invalid=0)
        conns.append(Conn(rng, frames, 1, "tls", stops=prio))
        scheds.append(draw_cuts(rng, conns[-1], 4 if i == 0 else 3))
        assert len(scheds[-1]) == (3 if i == 0 else 2)
    for join, n in ((0, 297), (2, 597)):
        for _ in range(n):
            conns.append(short(join))
            scheds.append([])
    return conns, scheds
