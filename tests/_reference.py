"""Shared pieces of the reference differential (test_reference_diff.py), the transcript fixture
(golden/make_reference_transcripts.py, test_reference_transcripts_host.py,
test_gpu_reference_transcripts.py): the binding of oracle/_ref/libws_ref.so (the reference's own
WebSocket unit behind oracle/ref_driver.c), the session grammar, the three runners (reference,
oracle, the product's host surface) that give one transcript format, and the branch census.

A session is a short frame sequence with a configuration (side, limits, context wired or not,
echo hook on or off).  It is cut into reads; a runner feeds the reads one process_data call each
until one fails (the reference's on_websocket_read loop) and returns a transcript:

    reads   [(rc, recv_buffer_pos, recv_buffer_size, events so far)] per call made
    events  ("m", opcode, bytes) on_message | ("c", code) on_close | ("e", code) on_error |
            ("s", bytes) one frame handed to the socket
    end     (state, recv_buffer_pos, recv_buffer_size, fragmented_size, fragmented_opcode,
             fragmented_message is NULL, frames_sent)

Only the reference sends for real (uvhttp_ws_send_frame into the driver's fake socket).  The
oracle and the product's host surface stop where the reference calls uvhttp_ws_send_frame (the
oracle records a PONG / CLOSE-echo event, the product calls the control sink; on_message is the
echo hook's place).  For them the runner is the integration's send: it applies send_frame's own
rule, refuse unless state == OPEN (src/uvhttp_websocket.c:513), builds the frame with the oracle's
build_frame (mask = !is_server, fin = 1, :529-531) and takes the connection's next key.  A refused
send takes no key, as in the reference, where the refusal comes before build_frame.

Keys: word i of a connection's key stream is key_word(key_seed, i) (splitmix64, the driver's
ws_ref_key_word), its bytes low first."""
import ctypes as C
import os
import random

import numpy as np

import _oracle as O

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_SO = os.path.join(REPO, "oracle", "_ref", "libws_ref.so")
# where oracle/ref.mk looks for the reference tree
REFERENCE_DIR = os.environ.get("REFERENCE_DIR", "/root/reference")
DEFAULT_MF, DEFAULT_MM = 16 * 1024 * 1024, 64 * 1024 * 1024
OPEN, CLOSED = 1, 3
M64 = (1 << 64) - 1


def have_reference_tree():
    return os.path.exists(os.path.join(REFERENCE_DIR, "src", "uvhttp_websocket.c"))


_R = None


def load_ref():
    """the reference library, or None where it has not been built"""
    global _R
    if _R is not None:
        return _R
    if not os.path.exists(REF_SO):
        return None
    L = C.CDLL(REF_SO)
    vp, u64, sz = C.c_void_p, C.c_uint64, C.c_size_t
    for name, res, args in [
        ("ws_ref_conn_new", vp, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, u64]),
        ("ws_ref_conn_free", None, [vp]),
        ("ws_ref_feed", C.c_int, [vp, vp, sz]),
        ("ws_ref_events", sz, [vp, vp, sz]),
        ("ws_ref_end_state", None, [vp, C.POINTER(u64 * 8)]),
        ("ws_ref_key_word", C.c_uint32, [u64, u64]),
        ("ws_ref_parse_frame_header", C.c_int, [vp, sz, C.POINTER(u64 * 8), C.POINTER(sz)]),
        ("ws_ref_parse_many", None, [vp, sz, vp, sz, vp, vp, vp]),
        ("ws_ref_apply_mask", None, [vp, sz, vp]),
        ("ws_ref_build_frame", C.c_long, [vp, vp, sz, vp, sz, C.c_int, C.c_int, C.c_int]),
    ]:
        fn = getattr(L, name)
        fn.restype, fn.argtypes = res, args
    _R = L
    return L


def key_word(seed, i):
    z = (seed + (i + 1) * 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    z ^= z >> 31
    return (z >> 16) & 0xFFFFFFFF


def key_bytes(seed, i):
    return key_word(seed, i).to_bytes(4, "little")


def gen_bytes(seed, n):
    """the byte generator of large payloads: byte i = (x >> 8) & 0xFF of
    x = mix(seed * 0x9E3779B1 + i * 0x85EBCA6B mod 2^32), mix(x) = (x ^ x >> 15) * 0x2C1B3C6D mod
    2^32, then x ^ x >> 12"""
    i = np.arange(n, dtype=np.uint64)
    x = (np.uint64(seed * 0x9E3779B1 & 0xFFFFFFFF) + i * np.uint64(0x85EBCA6B)) & np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x2C1B3C6D)) & np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(12)
    return ((x >> np.uint64(8)) & np.uint64(0xFF)).astype(np.uint8).tobytes()


def xor_key(payload, key):
    n = len(payload)
    if not n:
        return b""
    return (np.frombuffer(payload, np.uint8) ^ np.resize(np.frombuffer(key, np.uint8), n)).tobytes()


# ---- frames and sessions ----------------------------------------------------------------------

class F:
    """one frame of a session: what it is, its wire bytes, and the branches it is there for.
    enc: 7 / 16 / 64, the length encoding (None: minimal); declared: the length the header states
    when it is not len(payload) (the frame then carries no payload: it fails at its header);
    gen = (seed, n): the payload is gen_bytes(seed, n)"""

    def __init__(self, op, payload=b"", fin=1, rsv=0, masked=True, key=b"\0\0\0\0", enc=None,
                 declared=None, gen=None, labels=()):
        self.op, self.fin, self.rsv, self.masked, self.key = op, int(bool(fin)), rsv, bool(masked), bytes(key)
        self.gen = gen
        self.payload = gen_bytes(*gen) if gen else bytes(payload)
        self.labels = set(labels)
        n = len(self.payload) if declared is None else declared
        self.declared = declared
        enc = enc or (7 if n < 126 else 16 if n < 65536 else 64)
        b0 = (0x80 if self.fin else 0) | (rsv << 4) | (op & 0xF)
        mb = 0x80 if self.masked else 0
        if enc == 7:
            assert n < 126
            head = bytes([b0, mb | n])
        elif enc == 16:
            assert n < 65536
            head = bytes([b0, mb | 126, n >> 8, n & 0xFF])
        else:
            head = bytes([b0, mb | 127]) + n.to_bytes(8, "big")
        self.head = head + (self.key if self.masked else b"")
        self.body = xor_key(self.payload, self.key) if self.masked else self.payload
        self.bytes = self.head + self.body


class Session:
    def __init__(self, seed, is_server, mfs, mms, wired, echo, frames, template, cut=None):
        self.seed, self.is_server, self.mfs, self.mms = seed, is_server, mfs, mms
        self.wired, self.echo, self.frames, self.template = wired, echo, frames, template
        self.key_seed = 0xC0FFEE00 + seed
        self.cut = cut  # a forced cut position (bytes into the wire) for the "cuts" mode
        self.wire = b"".join(f.bytes for f in frames)

    @property
    def side(self):
        return "server" if self.is_server else "client"

    def config(self):
        return {"is_server": self.is_server, "max_frame_size": self.mfs, "max_message_size": self.mms,
                "wired": int(self.wired), "echo": int(self.echo), "key_seed": self.key_seed}

    def reads(self, mode):
        """mode: "one" (one read), "frame" (a read per frame), "cuts" (seeded cuts, or the forced
        one), "bytes" (a read per byte)"""
        w = self.wire
        if mode == "one":
            return [w]
        if mode == "frame":
            return [f.bytes for f in self.frames]
        if mode == "bytes":
            return [w[i:i + 1] for i in range(len(w))]
        assert mode == "cuts"
        if self.cut is not None:
            cuts = [self.cut]
        else:
            rng = random.Random(0x5C075 + self.seed)
            cuts = sorted({rng.randrange(1, len(w)) for _ in range(rng.randint(1, 4))}) if len(w) > 1 else []
        edges = [0] + cuts + [len(w)]
        return [w[a:b] for a, b in zip(edges, edges[1:])]


LIMITS = [(None, None), (10, None), (12, None), (126, None), (65536, None), (None, 0), (None, 4),
          (None, 70000)]
CLOSE_CODES_VALID = [1000, 1001, 1002, 1003, 1007, 1008, 1009, 1010, 1011, 3000, 4999]
CLOSE_CODES_INVALID = [0, 999, 1004, 1005, 1006, 1015, 2999, 5000, 65535]
N_TEMPLATES = 12
N_SESSIONS = 2304  # 8 configurations x 12 templates x 24


def make_session(seed):
    """the session of `seed`: bits 0-2 choose side / context wired / echo hook, the next field the
    template, the rest varies the template's own choices"""
    rng = random.Random(0x5EF00000 + seed)
    is_server, wired, echo = seed & 1, bool(seed & 2), bool(seed & 4)
    t = (seed >> 3) % N_TEMPLATES
    v = (seed >> 3) // N_TEMPLATES  # the variant within the template
    mfs, mms, cut = None, None, None
    good = bool(is_server)  # the masking the side expects of its peer

    def mk(op, payload=b"", fin=1, labels=(), **kw):
        kw.setdefault("masked", good)
        return F(op, payload, fin, key=rng.randbytes(4), labels=labels, **kw)

    def data(n):
        return rng.randbytes(n)

    def message(n_frag=1, op=None, size=None, inside=None):
        """a data message of n_frag non-empty fragments, `inside` put between them"""
        op = op or rng.choice([1, 2])
        out = []
        for k in range(n_frag):
            last = k == n_frag - 1
            n = size if size is not None else rng.choice([1, 2, 3, 7, 20])
            out.append(mk(op if k == 0 else 0, data(n), fin=last,
                          labels={"op%d" % (op if k == 0 else 0), "fin%d" % int(last)}))
            if not last and inside:
                out += inside()
        return out

    def ctl(op, n=None, labels=()):
        n = rng.choice([0, 1, 5, 30]) if n is None else n
        return mk(op, data(n), labels={"op%d" % op} | set(labels))

    fr = []
    if t == 0:  # a valid mix: messages, fragments with control frames inside, PING / PONG
        mfs, mms = LIMITS[v % len(LIMITS)]
        small = mfs is not None and mfs < 126
        for _ in range(rng.randint(2, 5)):
            r = rng.random()
            if r < 0.35:
                fr += message(1, size=rng.choice([0, 1, 5]) if small else None)
            elif r < 0.65 and mms != 4:
                fr += message(rng.randint(2, 3), size=2 if small else None,
                              inside=lambda: [ctl(rng.choice([9, 10]), 3, {"ctl_in_msg"})] if rng.random() < 0.6 else [])
            elif r < 0.85:
                fr.append(ctl(9, 4 if small else None))
            else:
                fr.append(ctl(10, 4 if small else None))
    elif t == 1:  # every opcode: the reserved ones are consumed silently (3-7) or after the
        #           control checks (11-15)
        ops = [3 + (v + k) % 5 for k in range(2)] + [11 + (v + k) % 5 for k in range(2)]
        rng.shuffle(ops)
        for op in ops:
            fr.append(mk(op, data(rng.choice([0, 3, 125])), labels={"op%d" % op, "reserved"}))
            if rng.random() < 0.5:
                fr += message(1)
        fr.append(ctl(9, 2))
    elif t == 2:  # one violating frame after a valid prefix, a valid frame behind it
        kinds = ["rsv1", "rsv2", "rsv3", "ctl126", "ctl_nonfin", "wrong_mask", "msb64", "cont_nothing_open",
                 "data_in_msg", "res_ctl126", "res_ctl_nonfin", "multi"]
        kind = kinds[v % len(kinds)]
        for _ in range(rng.randint(0, 2)):
            fr += message(1) if rng.random() < 0.6 else [ctl(9)]
        if kind.startswith("rsv"):
            fr.append(mk(rng.choice([1, 2, 9]), data(3), rsv={"rsv1": 4, "rsv2": 2, "rsv3": 1}[kind], labels={kind}))
        elif kind == "ctl126":
            fr.append(mk(rng.choice([8, 9, 10]), data(126), labels={"ctl126"}))
        elif kind == "ctl_nonfin":
            fr.append(mk(rng.choice([8, 9, 10]), data(2), fin=0, labels={"ctl_nonfin"}))
        elif kind == "res_ctl126":
            fr.append(mk(rng.choice([11, 12, 13, 14, 15]), data(126), labels={"ctl126", "reserved_ctl_check"}))
        elif kind == "res_ctl_nonfin":
            fr.append(mk(rng.choice([11, 12, 13, 14, 15]), data(2), fin=0, labels={"ctl_nonfin", "reserved_ctl_check"}))
        elif kind == "wrong_mask":
            # an unmasked frame fails a server; a masked one is unmasked and accepted by a client
            fr.append(mk(rng.choice([1, 2, 9]), data(5), masked=not good,
                         labels={"unmasked_to_server" if is_server else "masked_to_client"}))
        elif kind == "msb64":
            fr.append(mk(2, b"", enc=64, declared=rng.choice([1 << 63, M64, (1 << 63) + 5]), labels={"msb64"}))
        elif kind == "cont_nothing_open":
            fr.append(mk(0, data(3), fin=rng.randint(0, 1), labels={"cont_nothing_open"}))
        elif kind == "data_in_msg":
            fr.append(mk(1, data(3), fin=0, labels={"op1", "fin0"}))
            fr.append(mk(rng.choice([1, 2]), data(2), fin=rng.randint(0, 1), labels={"data_in_msg"}))
        else:  # several violations on one frame: RSV, a long non-FIN control frame, the wrong mask
            fr.append(mk(9, data(126), fin=0, rsv=rng.choice([1, 2, 4, 7]), masked=not good, labels={"multi_violation"}))
        fr += message(1)
    elif t == 3:  # non-minimal length encodings are accepted
        for _ in range(rng.randint(1, 3)):
            if rng.random() < 0.5:
                fr.append(mk(rng.choice([1, 2]), data(rng.choice([0, 1, 125])), enc=16, labels={"nonmin16"}))
            else:
                fr.append(mk(rng.choice([1, 2, 9]), data(rng.choice([0, 5, 125])), enc=64, labels={"nonmin64"}))
            if rng.random() < 0.5:
                fr.append(ctl(9, 125, {"ctl125"}))
        if v % 3 == 0:
            fr.append(mk(2, data(300), enc=64, labels={"nonmin64"}))
    elif t == 4:  # fragments: the zero-length first fragment, max_message_size crossings
        kind = ["zero_first", "mms_first", "mms_middle", "mms_last", "mms0", "single_over_mms", "mms_big"][v % 7]
        if rng.random() < 0.5:
            fr += message(1)
        if kind == "zero_first":
            # fragment_append of 0 bytes allocates nothing: fragmented_message stays NULL (:964),
            # so the CONTINUATION that follows finds nothing open
            fr.append(mk(rng.choice([1, 2]), b"", fin=0, labels={"frag_zero_first"}))
            if rng.random() < 0.5:
                fr.append(ctl(9, 1))
            fr.append(mk(0, data(2), fin=rng.randint(0, 1), labels={"cont_after_zero_first"}))
        elif kind == "mms_first":
            mms = 4
            fr.append(mk(1, data(5), fin=0, labels={"mms_first"}))
        elif kind == "mms_middle":
            mms = 4
            fr += [mk(2, data(2), fin=0, labels={"op2", "fin0"}), mk(0, data(3), fin=0, labels={"mms_middle"})]
        elif kind == "mms_last":
            mms = 4
            fr += [mk(1, data(2), fin=0), mk(0, data(2), fin=0, labels={"mms_exact"}),
                   mk(0, data(1), fin=1, labels={"mms_last"})]
        elif kind == "mms0":  # 0 = no limit
            mms = 0
            fr += message(3, size=rng.choice([5, 200]))
        elif kind == "single_over_mms":  # an unfragmented message is never measured
            mms = 4
            fr.append(mk(rng.choice([1, 2]), data(rng.choice([5, 100])), labels={"single_over_mms"}))
        else:
            mms = 70000
            fr += [mk(2, fin=0, gen=(seed, 65535), labels={"op2", "fin0"}),
                   mk(0, fin=0, gen=(seed + 1, 4465), labels={"mms_exact"}),
                   mk(0, data(1), fin=1, labels={"mms_last"})]
        fr += message(1)
    elif t == 5:  # CLOSE: payload lengths, codes, and what comes after it
        n = [0, 1, 2, 3, 125][v % 5]
        valid = (v // 5) % 2 == 0
        code = rng.choice(CLOSE_CODES_VALID if valid else CLOSE_CODES_INVALID)
        payload = (code.to_bytes(2, "big") + data(123))[:n]
        if rng.random() < 0.6:
            fr += message(1) if rng.random() < 0.5 else [ctl(9)]
        if rng.random() < 0.3:
            fr.append(mk(1, data(3), fin=0, labels={"op1", "fin0"}))  # a message open across the CLOSE
        labels = {"op8", "close_len%d" % n}
        if n >= 2:
            labels.add("close_code_valid" if valid else "close_code_invalid")
        fr.append(mk(8, payload, labels=labels))
        open_msg = any("fin0" in f.labels for f in fr)
        for _ in range(rng.randint(0, 3)):
            r = rng.random()
            if r < 0.4:
                fr.append(mk(9, data(rng.choice([0, 4])), labels={"after_close", "ping_after_close"}))
            elif r < 0.6:
                fr.append(mk(8, b"\x03\xe9x", labels={"after_close", "close_after_close"}))
            elif open_msg:
                fr.append(mk(0, data(2), fin=1, labels={"after_close", "message_after_close"}))
                open_msg = False
            else:
                fr.append(mk(rng.choice([1, 2]), data(4), labels={"after_close", "message_after_close"}))
    elif t == 6:  # a header that fails to parse (64-bit length, top bit set), reached in two
        #           reads: the first leaves k bytes of it buffered (:884-890)
        k = v % 9 + 1
        for _ in range(rng.randint(0, 2)):
            fr += message(1)
        cut = sum(len(f.bytes) for f in fr) + k
        fr.append(mk(rng.choice([1, 2, 9]), b"", enc=64, declared=(1 << 63) | rng.getrandbits(40),
                     labels={"msb64", "partial%d" % k}))
        fr += message(1)
    elif t == 7:  # a read past the 64 KiB receive buffer: doubled under the default limit,
        #           refused where max_frame_size clamps the doubling (:832-857)
        if v % 2 == 0:
            fr.append(mk(2, gen=(seed, [65535, 65536, 70000][(v // 2) % 3]), labels={"op2", "big_read"}))
            fr.append(ctl(9, 3))
        else:
            mfs = 65536
            fr.append(mk(2, gen=(seed, 65536 - 8 * (v // 2 % 2)), labels={"clamp"}))
    elif t == 8:  # the payload lengths at which the frame header changes, as messages
        n = [125, 126, 127, 65535, 65536][v % 5]
        if n >= 4096:
            fr.append(mk(rng.choice([1, 2]), gen=(seed, n), labels={"len%d" % n}))
        else:
            fr.append(mk(rng.choice([1, 2]), data(n), labels={"len%d" % n}))
        fr.append(ctl(9, 125, {"ctl125"}))
    elif t == 9:  # max_frame_size: a length equal to it passes, one past it fails
        mfs = [10, 12, 126, 65536][v % 4]
        fr.append(mk(9, data(min(mfs, 125)), labels={"op9"} | ({"len_eq_mfs"} if mfs < 126 else set())))
        if mfs <= 126:
            fr.append(mk(rng.choice([1, 2]), data(mfs), labels={"len_eq_mfs"}))
        over = rng.choice([mfs + 1, mfs + 1, 1 << 20, (1 << 63) - 1])
        if mfs < 125 and rng.random() < 0.4:
            fr.append(mk(rng.choice([8, 9, 10]), data(mfs + 1), labels={"over_mfs"}))
        else:
            fr.append(mk(rng.choice([0, 1, 2]) if over > mfs + 1 else 2, b"", declared=over,
                         enc=64 if over >= 65536 else None, labels={"over_mfs"}))
        fr += message(1, size=2)
    elif t == 10:  # FIN 0 / 1 on every data opcode, messages of several fragments, empty ones
        fr += message(rng.randint(2, 4))
        fr.append(mk(rng.choice([1, 2]), b"", labels={"empty_message", "fin1"}))
        fr += [mk(1, data(3), fin=0, labels={"op1", "fin0"}), mk(0, b"", fin=0, labels={"op0", "empty_cont"}),
               mk(0, data(2), fin=1, labels={"op0", "fin1"})]
        if v % 2:
            fr.append(mk(2, data(6), fin=0, labels={"op2", "fin0"}))  # left open at the end
    else:  # t == 11: PING / PONG / CLOSE payloads of exactly 125 bytes
        op = [8, 9, 10][v % 3]
        fr += message(1)
        if op == 8:
            fr.append(mk(8, b"\x03\xe8" + data(123), labels={"op8", "ctl125", "close_len125", "close_code_valid"}))
        else:
            fr.append(ctl(op, 125, {"ctl125"}))
            fr.append(ctl(8, 0, {"close_len0"}))
    return Session(seed, is_server, mfs, mms, wired, echo, fr, t, cut)


# ---- runners -----------------------------------------------------------------------------------

def _parse_events(raw, names):
    out, offs, i, n = [], [], 0, len(raw)
    while i < n:
        typ = raw[i]
        a = int.from_bytes(raw[i + 1:i + 5], "little", signed=True)
        ln = int.from_bytes(raw[i + 5:i + 13], "little")
        out.append((names[typ], a, raw[i + 13:i + 13 + ln]))
        offs.append(i)
        i += 13 + ln
    return out, offs


def _transcript(reads, events, end):
    return {"reads": reads, "events": events, "end": tuple(int(x) for x in end)}


def run_reference(sess, reads):
    R = load_ref()
    mf = -1 if sess.mfs is None else sess.mfs
    mm = -1 if sess.mms is None else sess.mms
    c = R.ws_ref_conn_new(sess.is_server, mf, mm, int(sess.wired), int(sess.echo), sess.key_seed)
    assert c
    try:
        st = (C.c_uint64 * 8)()
        per, marks = [], []
        for r in reads:
            buf = (C.c_uint8 * max(1, len(r))).from_buffer_copy(r or b"\0")
            rc = R.ws_ref_feed(c, buf, len(r))
            R.ws_ref_end_state(c, C.byref(st))
            per.append((rc, st[1], st[2]))
            marks.append(R.ws_ref_events(c, None, 0))
            if rc != 0:
                break
        n = R.ws_ref_events(c, None, 0)
        raw = (C.c_uint8 * max(1, n))()
        R.ws_ref_events(c, raw, n)
        evs, offs = _parse_events(bytes(raw)[:n], {1: "m", 2: "c", 3: "e", 4: "s"})
        events = [(k, a, p) if k == "m" else (k, p) if k == "s" else (k, a) for k, a, p in evs]
        offs.append(n)
        counts = [offs.index(m) for m in marks]
        R.ws_ref_end_state(c, C.byref(st))
        assert st[7] == 4 * sum(1 for e in events if e[0] == "s") * (0 if sess.is_server else 1)
        return _transcript([(rc, p, s, k) for (rc, p, s), k in zip(per, counts)], events, list(st)[:7])
    finally:
        R.ws_ref_conn_free(c)


class _Sender:
    """the integration's send for a runner whose implementation stops at the call of
    uvhttp_ws_send_frame: refuse unless OPEN (:513), build with mask = !is_server, fin = 1"""

    def __init__(self, sess, events):
        self.sess, self.events, self.sent = sess, events, 0

    def send(self, state, payload, opcode):
        if state != OPEN:
            return
        s = self.sess
        rc, b = O.build_frame(payload, opcode, 0 if s.is_server else 1, 1,
                              b"\0\0\0\0" if s.is_server else key_bytes(s.key_seed, self.sent))
        assert rc > 0
        self.sent += 1
        self.events.append(("s", b))


def run_oracle(sess, reads):
    mf = DEFAULT_MF if sess.mfs is None else sess.mfs
    mm = DEFAULT_MM if sess.mms is None else sess.mms
    orc = O.OracleConn(sess.is_server, mf, mm, record=1, wrapper=sess.wired)
    per, marks = [], []
    for r in reads:
        rc = orc.process_data(r)
        per.append((rc, orc.recv_pos, orc.recv_size))
        marks.append(int(orc.L.oracle_conn_n_events(orc.c)))
        if rc != 0:
            break
    events, origin = [], []  # origin[j]: raw events consumed when normalised event j existed
    snd = _Sender(sess, events)
    state = OPEN
    for j, (k, a, p) in enumerate(orc.events()):
        if k == "message":
            events.append(("m", a, p))
            if sess.echo:
                snd.send(state, p, a)
        elif k == "close":
            events.append(("c", a))
            if not sess.wired:
                state = CLOSED  # (:1069; with a context the echo event follows and comes first)
        elif k == "close_echo":
            snd.send(state, p, 8)  # sent before the state changes (:1065-1069)
            state = CLOSED
        else:
            snd.send(state, p, 10)
        origin += [j + 1] * (len(events) - len(origin))
    counts = [sum(1 for o in origin if o <= m) for m in marks]
    assert orc.state == state
    end = (orc.state, orc.recv_pos, orc.recv_size, orc.frag_size, orc.frag_opcode,
           int(not orc.frag_pending), snd.sent)
    return _transcript([(rc, p, s, k) for (rc, p, s), k in zip(per, counts)], events, end)


_HOST = [None]  # the host run in progress (the control hooks are process-wide)
_HOOKS = []


def install_host_hooks():
    """the product's control hooks for run_host (leave with remove_host_hooks)"""
    import uvhttp_amd as U

    @U.CONTEXT_RESOLVER
    def resolver(conn):
        return 0x5E  # stands for wrapper->conn->server->context

    @U.CONTROL_SINK
    def sink(ctx, conn, op, p, n):
        run = _HOST[0]
        run["snd"].send(run["conn"].struct.state, C.string_at(p, n) if n else b"", op)

    _HOOKS[:] = [resolver, sink]
    U.lib().uvhttp_ws_amd_set_control_hooks(resolver, sink)


def remove_host_hooks():
    import uvhttp_amd as U
    U.lib().uvhttp_ws_amd_set_control_hooks(U.CONTEXT_RESOLVER(), U.CONTROL_SINK())
    _HOOKS.clear()


class HostConn:
    """a connection of the product's host surface (uvhttp_amd/csrc/ws_host.c) that records a
    transcript: callbacks, the echo hook and, through the process-wide control hooks
    (install_host_hooks), the control sink.  Use as a context manager around the calls that drive
    it: process_data, or a delivery of a device decode."""

    def __init__(self, sess):
        import uvhttp_amd as U
        assert _HOOKS, "install_host_hooks() first"
        self.sess = sess
        self.conn = conn = U.WsConnection(sess.is_server, sess.mfs, sess.mms, callbacks=False,
                                          user_data=sess.wired)
        self.events = events = []
        self.snd = snd = _Sender(sess, events)

        def on_message(c, data, n, opcode):
            p = C.string_at(data, n) if n else b""
            events.append(("m", opcode, p))
            if sess.echo:
                snd.send(conn.struct.state, p, opcode)
            return 0

        def on_close(c, code, reason):
            events.append(("c", code))
            return 0

        def on_error(c, code, msg):
            events.append(("e", code))
            return 0

        self._cbs = (U.ON_MESSAGE(on_message), U.ON_CLOSE(on_close), U.ON_ERROR(on_error))
        U.lib().uvhttp_ws_set_callbacks(conn.ptr, *self._cbs)
        conn.ptr.contents.state = OPEN  # as after the handshake (:503)

    def __enter__(self):
        _HOST[0] = {"conn": self.conn, "snd": self.snd}
        return self

    def __exit__(self, *exc):
        _HOST[0] = None

    def end(self):
        s = self.conn.struct
        return (s.state, s.recv_buffer_pos, s.recv_buffer_size, s.fragmented_size, s.fragmented_opcode,
                int(not s.fragmented_message), self.snd.sent)

    def close(self):
        self.conn.close()


def run_host(sess, reads):
    """the product's uvhttp_ws_process_data; needs install_host_hooks()"""
    h = HostConn(sess)
    try:
        with h:
            per = []
            for r in reads:
                rc = h.conn.process_data(r)
                s = h.conn.struct
                per.append((rc, s.recv_buffer_pos, s.recv_buffer_size, len(h.events)))
                if rc != 0:
                    break
        return _transcript(per, h.events, h.end())
    finally:
        h.close()


def first_difference(a, b):
    """where two transcripts part: a short text, or None"""
    for i, (x, y) in enumerate(zip(a["reads"], b["reads"])):
        if x != y:
            return "read %d: %r != %r" % (i, x, y)
    if len(a["reads"]) != len(b["reads"]):
        return "reads made: %d != %d" % (len(a["reads"]), len(b["reads"]))
    for i, (x, y) in enumerate(zip(a["events"], b["events"])):
        if x != y:
            read = next((k for k, r in enumerate(a["reads"]) if r[3] > i), len(a["reads"]) - 1)
            return "event %d (read %d): %.120r != %.120r" % (i, read, x, y)
    if len(a["events"]) != len(b["events"]):
        return "events: %d != %d" % (len(a["events"]), len(b["events"]))
    if a["end"] != b["end"]:
        return "end state: %r != %r" % (a["end"], b["end"])
    return None


# ---- the branch census -------------------------------------------------------------------------

# labels whose frame must be consumed (rc 0, nothing left buffered) / must fail its read
OK_LABELS = (["op%d" % k for k in range(16)] +
             ["fin0", "fin1", "reserved", "ctl125", "ctl_in_msg", "masked_to_client", "nonmin16", "nonmin64",
              "frag_zero_first", "mms_exact", "single_over_mms", "len_eq_mfs", "empty_message", "empty_cont",
              "len125", "len126", "len127", "len65535", "len65536",
              "close_len0", "close_len1", "close_len2", "close_len3", "close_len125", "close_code_valid",
              "close_code_invalid", "ping_after_close", "close_after_close", "message_after_close"])
FAIL_LABELS = ["rsv1", "rsv2", "rsv3", "ctl126", "ctl_nonfin", "reserved_ctl_check", "unmasked_to_server",
               "msb64", "over_mfs", "data_in_msg", "cont_nothing_open", "cont_after_zero_first", "mms_first",
               "mms_middle", "mms_last", "multi_violation"]
SESSION_BRANCHES = ["after_close_same_read", "after_close_later_read", "big_read", "clamp"] + \
    ["partial%d" % k for k in range(1, 10)]
ONE_SIDED = {"unmasked_to_server": "server", "masked_to_client": "client"}
BRANCHES = OK_LABELS + FAIL_LABELS + SESSION_BRANCHES


def required():
    """every (branch, side) that must occur"""
    return [(b, s) for b in BRANCHES for s in ("server", "client") if ONE_SIDED.get(b, s) == s]


def _events_of_read(tr, i):
    a = tr["reads"][i - 1][3] if i else 0
    return tr["events"][a:tr["reads"][i][3]]


def branches_taken(sess, runs):
    """the branches the reference took in this session, judged from its transcripts alone: runs =
    {mode: transcript} for the modes run ("frame" judges the per-frame branches: read i is frame i)"""
    took = set()
    tr = runs.get("frame")
    if tr is not None:
        n = len(tr["reads"])
        closed_at = None
        for i, f in enumerate(sess.frames[:n]):
            rc, pos = tr["reads"][i][0], tr["reads"][i][1]
            ok, failed = rc == 0 and pos == 0, rc != 0
            evs = _events_of_read(tr, i)
            for lab in f.labels:
                if lab in FAIL_LABELS:
                    if failed:
                        took.add(lab)
                elif lab in OK_LABELS and ok:
                    if lab == "reserved" or (lab.startswith("op") and int(lab[2:]) in (3, 4, 5, 6, 7, 11, 12, 13, 14, 15)):
                        if evs:
                            continue  # consumed silently means no event at all
                    if lab.startswith("close_len") and not any(e[0] == "c" for e in evs):
                        continue
                    if lab.startswith("close_code") and not any(
                            e[0] == "c" and e[1] == int.from_bytes(f.payload[:2], "big") for e in evs):
                        continue
                    if lab in ("ping_after_close", "close_after_close") and (
                            not sess.wired or any(e[0] == "s" for e in evs)):
                        continue  # with a context: send_frame refuses once the state is not OPEN
                    if lab == "message_after_close" and not any(e[0] == "m" for e in evs):
                        continue
                    took.add(lab)
            if ok and closed_at is not None and "after_close" in f.labels:
                took.add("after_close_later_read")
            if ok and f.op == 8 and closed_at is None:
                closed_at = i
    tr = runs.get("one")
    if tr is not None:
        rc, pos, size, _ = tr["reads"][0]
        ci = next((i for i, e in enumerate(tr["events"]) if e[0] == "c"), None)
        if any("after_close" in f.labels for f in sess.frames) and rc == 0 and pos == 0 and ci is not None:
            took.add("after_close_same_read")
        if any("big_read" in f.labels for f in sess.frames) and len(sess.wire) > 65536 and rc == 0 and size > 65536:
            took.add("big_read")
        if any("clamp" in f.labels for f in sess.frames) and len(sess.wire) > 65536 and rc != 0 and pos == 0 \
                and not tr["events"]:
            took.add("clamp")
    tr = runs.get("cuts")
    if tr is not None and sess.cut is not None and len(tr["reads"]) == 2:
        k = next(int(lab[7:]) for f in sess.frames for lab in f.labels if lab.startswith("partial"))
        if tr["reads"][0][:2] == (0, k) and tr["reads"][1][0] != 0:
            took.add("partial%d" % k)
    return took


# ---- the committed transcripts (tests/golden/reference_transcripts.json) ------------------------

BIG = 4096  # payloads, messages and sent frames of this size and more are not stored as bytes
GOLDEN = os.path.join(REPO, "tests", "golden", "reference_transcripts.json")


class Entry:
    """one committed session: its configuration, wire, reads and the reference's transcript.
    Large messages and sent frames are (length, SHA-256) pairs: compare with same_bytes()."""

    def __init__(self, d):
        c = d["config"]
        self.seed, self.mode, self.branches = d["seed"], d["mode"], d["branches"]
        self.is_server, self.wired, self.echo, self.key_seed = c["is_server"], bool(c["wired"]), bool(c["echo"]), c["key_seed"]
        self.mfs, self.mms = c["max_frame_size"], c["max_message_size"]
        wire = bytearray()
        for seg in d["wire"]:
            if isinstance(seg, str):
                wire += bytes.fromhex(seg)
            else:
                b = gen_bytes(*seg["g"])
                wire += xor_key(b, bytes.fromhex(seg["k"])) if seg["k"] else b
        self.wire = bytes(wire)
        assert sum(d["reads"]) == len(self.wire)
        self.read_lens = d["reads"]
        self.keys = d["keys"]
        self.transcript = {
            "reads": [tuple(r) for r in d["results"]],
            "events": [(e[0],) + tuple(bytes.fromhex(x) if isinstance(x, str) else x for x in e[1:])
                       for e in d["events"]],
            "end": tuple(d["end"])}

    @property
    def side(self):
        return "server" if self.is_server else "client"

    def reads(self):
        out, a = [], 0
        for n in self.read_lens:
            out.append(self.wire[a:a + n])
            a += n
        return out


def same_bytes(stored, got):
    """a stored byte field (bytes, or {"n", "sha256"} for a large one) against bytes"""
    import hashlib
    if isinstance(stored, dict):
        return stored["n"] == len(got) and stored["sha256"] == hashlib.sha256(got).hexdigest()
    return stored == got


def same_events(stored, got):
    return len(stored) == len(got) and all(
        len(a) == len(b) and all(same_bytes(x, y) if isinstance(y, bytes) else x == y for x, y in zip(a, b))
        for a, b in zip(stored, got))


def same_transcript(stored, got):
    """None, or where a runner's transcript parts from a committed one"""
    if stored["reads"] != got["reads"]:
        i = next((k for k, (x, y) in enumerate(zip(stored["reads"], got["reads"])) if x != y),
                 min(len(stored["reads"]), len(got["reads"])))
        return "read %d: %r != %r" % (i, stored["reads"][i:i + 1], got["reads"][i:i + 1])
    if not same_events(stored["events"], got["events"]):
        i = next((k for k, (x, y) in enumerate(zip(stored["events"], got["events"])) if not same_events([x], [y])),
                 min(len(stored["events"]), len(got["events"])))
        return "event %d: %.100r != %.100r" % (i, stored["events"][i:i + 1], got["events"][i:i + 1])
    if stored["end"] != got["end"]:
        return "end state: %r != %r" % (stored["end"], got["end"])
    return None


def load_transcripts():
    import json
    with open(GOLDEN) as f:
        doc = json.load(f)
    return doc, [Entry(d) for d in doc["sessions"]]


# ---- a decoded batch against the committed transcripts -------------------------------------------

DESC_DT = np.dtype([("payload_off", "<u8"), ("payload_len", "<u8"), ("masking_key", "<u4"),
                    ("message", "<u4"), ("opcode", "u1"), ("flags", "u1"),
                    ("header_size", "u1"), ("status", "i1"), ("wire_len", "<u4")])


def sent_frames(entry):
    return [e[1] for e in entry.transcript["events"] if e[0] == "s"]


def sender_kind(entry):
    """which of the product's calls builds what this session sent: the control replies (a server
    context, no hook), the echoes (the hook, no context), the answers (both), or None"""
    return {(True, False): "replies", (False, True): "echoes", (True, True): "answers",
            (False, False): None}[(entry.wired, entry.echo)]


def split_frames(out, off, n):
    return [bytes(out[off[j]:off[j + 1]]) for j in range(n)]


def check_sent(entry, frames, what):
    want = sent_frames(entry)
    assert len(frames) == len(want) and all(same_bytes(w, g) for w, g in zip(want, frames)), (
        "session seed %d (%s cut): %s differ from the frames the reference sent: %d built, %d sent, first "
        "difference at frame %s" % (entry.seed, entry.mode, what, len(frames), len(want),
                                    next((j for j, (w, g) in enumerate(zip(want, frames)) if not same_bytes(w, g)),
                                         min(len(frames), len(want)))))


def host_twin_frames(U, entry, wire, desc, first, nd, wire_len=None):
    """the frames the product's host twin of the session's sender builds from a decoded batch"""
    kind = sender_kind(entry)
    keys = None if entry.is_server else [int(k) for k in entry.keys] + [0] * (nd + 1)
    if kind == "replies":
        out, off, r = U.control_replies(wire, desc, first, nd, entry.is_server, 1, keys, wire_len=wire_len)
        n = r["n_replies"]
    elif kind == "echoes":
        out, off, _, r = U.echo_messages(wire, desc, first, nd, entry.is_server, 1, keys, wire_len=wire_len)
        n = r["n_echoes"]
    else:
        out, off, _, r, _ = U.answer_messages(wire, desc, first, nd, entry.is_server, 1, keys, wire_len=wire_len)
        n = r["n_answers"]
    assert r["status"] == 0, (entry.seed, r)
    return split_frames(out, off, n)


def check_delivery(e, h, rc, calls, what, sizes=True):
    """a recording connection (HostConn) after a delivery of a decoded batch against the session's
    committed transcript"""
    tr = e.transcript
    info = "session seed %d (%s cut), %s" % (e.seed, e.mode, what)
    assert rc == tr["reads"][-1][0], info + ": return code"
    if calls is not None:
        assert calls == len(tr["reads"]), info + ": process_data calls that ran"
    assert same_events(tr["events"], h.events), "%s: events: %.300r != %.300r" % (info, tr["events"], h.events)
    end, want = h.end(), tr["end"]
    if not sizes:  # a batch has no receive buffer: its size and what is left in it are not the session's
        end, want = end[:1] + end[3:], want[:1] + want[3:]
    assert end == want, info + ": end state %r != %r" % (end, want)


def batch_sessions(entries):
    """the sessions that are a batch (every frame fed alone, in order, to one server
    connection whose receive buffer is empty): server side, cut one read per frame, and every
    successful call left the receive buffer empty, so every read was one whole frame"""
    out = [e for e in entries if e.is_server and e.mode == "frame"
           and all(r[1] == 0 for r in e.transcript["reads"] if r[0] == 0)]
    assert len(out) >= 40
    return out
