"""uvhttp_ws_gpu_answer_messages_streams / _inplace: device == the host twin
uvhttp_ws_answer_messages == the transcript of process_data with both recorders active
(tests/_answer_ref.py), byte for byte, in d_out, d_out_off, the runs, d_conn, d_reply_conn, d_open,
d_open_off and the summary, inside guarded buffers: the CPU cases as one batch, the 256-connection
and 256-descriptor scan blocks, the 64 KiB emit tile under a PONG, client batches keyed by merged
slot, a three-call session, the emit in pieces, a captured graph, both forms, the capacity
failures, every EINVAL, and the identities with echo_messages_streams and control_replies_streams
when a batch holds only data or only control frames."""
import random

import numpy as np
import pytest

import _answer_ref as AR
import _echo_ref as ER
from test_gpu_echo import FAILED, FILL, GUARD, SCAN_BLOCK, TILE, _dev, _payload, _streams
from test_gpu_epoch_wrap import _engine

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch as t
    if not t.cuda.is_available():
        pytest.skip("no GPU")
    return t


@pytest.fixture(scope="module")
def eng(torch):
    import uvhttp_amd as U
    e = U.GpuEngine(0)
    yield e
    e.close()


class Out:
    """guarded device outputs of one answer call, and their host copies"""

    def __init__(self, torch, S, max_answers, out_cap, open_cap, with_open=True, with_reply=True):
        t = torch
        self.S, self.max_answers, self.out_cap, self.open_cap = S, max_answers, out_cap, open_cap
        self.buf = t.full((GUARD + out_cap + GUARD,), FILL, dtype=t.uint8, device="cuda")
        self.out = self.buf[GUARD:GUARD + out_cap] if out_cap else self.buf[GUARD:GUARD + 1]
        self.obuf = t.full((GUARD + open_cap + GUARD,), FILL, dtype=t.uint8, device="cuda")
        self.open = (self.obuf[GUARD:GUARD + open_cap] if open_cap else self.obuf[GUARD:GUARD + 1]) if with_open else None
        self.off = t.full((max_answers + 2,), -7, dtype=t.int64, device="cuda")
        self.ooff = t.full((S + 2,), -7, dtype=t.int64, device="cuda")
        self.runs = t.full((2 * S + 2,), 0x5A5A5A5A, dtype=t.int32, device="cuda")
        self.conn = t.full((32 * S + 32,), FILL, dtype=t.uint8, device="cuda")
        self.reply = t.full((16 * S + 16,), FILL, dtype=t.uint8, device="cuda") if with_reply else None
        self.summ = t.full((32,), FILL, dtype=t.uint8, device="cuda")

    def kw(self):
        return dict(out=self.out, out_off=self.off, runs=self.runs, open=self.open, open_cap=self.open_cap,
                    open_off=self.ooff, conn=self.conn, summary=self.summ, reply_conn=self.reply)

    def read(self, eng):
        summ = eng.read_answer_summary(self.summ)
        ok = summ["status"] == AR.OK
        buf, obuf = self.buf.cpu().numpy(), self.obuf.cpu().numpy()
        n = summ["out_bytes"] if ok else 0
        m = summ["open_bytes"] if ok and self.open is not None else 0
        assert (buf[:GUARD] == FILL).all() and (buf[GUARD + n:] == FILL).all(), "d_out written outside the answers"
        assert (obuf[:GUARD] == FILL).all() and (obuf[GUARD + m:] == FILL).all(), "d_open written outside the messages"
        off, ooff = self.off.cpu().numpy(), self.ooff.cpu().numpy()
        assert off[-1] == -7 and ooff[-1] == -7, "an offset table written past its end"
        runs = self.runs.cpu().numpy().view(np.uint32)
        assert (runs[2 * self.S:] == 0x5A5A5A5A).all()
        assert (self.conn.cpu().numpy()[32 * self.S:] == FILL).all()
        conn = eng.read_answer_conns(self.conn, self.S)
        assert [(int(runs[2 * s]), int(runs[2 * s + 1])) for s in range(self.S)] == \
            [(c["first_answer"], c["n_answers"]) for c in conn]
        got = {"out": buf[GUARD:GUARD + n].tobytes(), "out_off": [int(x) for x in off[:-1]],
               "open": obuf[GUARD:GUARD + m].tobytes(), "open_off": [int(x) for x in ooff[:-1]], "conn": conn,
               "summary": summ}
        if self.reply is not None:
            assert (self.reply.cpu().numpy()[16 * self.S:] == FILL).all()
            got["reply"] = eng.read_reply_conns(self.reply, self.S)
        return got


def _want(host, max_answers, out_cap, open_cap, with_open=True):
    s = host["summary"]
    if s["n_answers"] > max_answers or s["out_bytes"] > out_cap or (with_open and s["open_bytes"] > open_cap):
        return AR.capacity_failure(host, max_answers)
    return host if with_open else dict(host, open=b"")


def run_streams(torch, eng, conns, is_server=None, enable=None, keys=None, flags=0, reads=None, pending=None,
                carries=None, gap=0, max_frames=None, max_answers=None, out_cap=None, open_cap=None, with_open=True,
                ref=True, silent=None, ref_eng=None, wire_len=None, identity=None):
    """decode_streams (decode_reads with `reads`) then answer_messages_streams, no host sync
    between; everything the call writes against the host twin over the device's own decode, and
    (ref) against the transcript -> (got, stream results).  identity = "echo" / "replies": d_out and
    d_out_off also equal that call's over the same decode"""
    import uvhttp_amd as U
    conns = [AR.raw(c) for c in conns]
    S = len(conns)
    wire, st, read_end = _streams(conns, is_server, reads, pending, gap)
    dw, dst = _dev(torch, wire), _dev(torch, st, 0)
    re_dev = torch.tensor(read_end or [0], dtype=torch.int64, device="cuda") if reads is not None else None
    if max_frames is None:
        max_frames = len(wire) // 2 + 1
    carry, coff = AR.carry_tables(pending, S)
    if carries is not None:
        carry, coff = AR.carry_tables([(0, c) for c in carries], S)
    max_answers = max_frames if max_answers is None else max_answers
    out_cap = 14 * max_answers + len(wire) + len(carry) if out_cap is None else out_cap
    open_cap = len(wire) + len(carry) if open_cap is None else open_cap
    d_en = _dev(torch, np.array(enable, np.uint8), 0) if enable is not None else None
    d_keys = _dev(torch, np.asarray(keys, np.uint32), 0) if keys is not None else None
    d_carry = _dev(torch, np.frombuffer(carry, np.uint8)) if pending is not None or carries is not None else None
    d_coff = torch.tensor(coff, dtype=torch.int64, device="cuda") if d_carry is not None else None
    wl = wire.size if wire_len is None else wire_len
    o = Out(torch, S, max_answers, out_cap, open_cap, with_open)
    desc, res = eng.decode_streams(dw, dst, S, max_frames, wire_len=wire.size, read_end=re_dev,
                                   n_reads=len(read_end))
    common = dict(enable=d_en, mask_keys=d_keys, carry=d_carry, carry_len=len(carry), carry_off=d_coff, wire_len=wl)
    eng.answer_messages_streams(dw, desc, max_frames, dst, res, S, max_answers, out_cap, flags=flags, **common, **o.kw())
    torch.cuda.synchronize()
    got = o.read(eng)
    results = eng.read_stream_results(res, S)
    first = [r.first_frame for r in results]
    nd = [0 if r.first_status in FAILED else r.n_delivered for r in results]
    hw, hd = dw[: wire.size].cpu().numpy(), eng.read_desc(desc, max_frames)
    host = AR.host_batch(U, hw, hd, first, nd, is_server, enable, keys, flags, pending, carries, max_answers, wire_len=wl)
    assert got == _want(host, max_answers, out_cap, open_cap, with_open)
    if got["summary"]["status"] == AR.OK:
        for s, c in enumerate(got["conn"]):  # the open message is the decoder's
            if c["status"] == AR.OK and (enable is None or enable[s]) and results[s].first_status not in FAILED:
                assert c["open_len"] == results[s].pending_bytes, s
    if ref:
        want = AR.expected_batch(conns, is_server, enable, keys, flags, reads, pending, silent or {}, max_answers)
        assert host == want
    if ref_eng is not None:  # the same call on an unsplit engine: byte for byte
        o2 = Out(torch, S, max_answers, out_cap, open_cap, with_open)
        ref_eng.answer_messages_streams(dw, desc, max_frames, dst, res, S, max_answers, out_cap, flags=flags, **common,
                                        **o2.kw())
        torch.cuda.synchronize()
        assert o2.read(ref_eng) == got
    if identity == "echo":
        out2, off2, _, _, _ = eng.echo_messages_streams(dw, desc, max_frames, dst, res, S, max_answers, out_cap,
                                                        flags=flags & 1, **common)
    elif identity == "replies":
        out2, off2, _, _ = eng.control_replies_streams(dw, desc, max_frames, dst, res, S, max_answers, out_cap,
                                                       enable=d_en, mask_keys=d_keys, flags=flags >> 1, wire_len=wl)
    if identity:
        torch.cuda.synchronize()
        n = got["summary"]["out_bytes"]
        assert got["out_off"] == [int(x) for x in off2.cpu().numpy()[:max_answers + 1]]
        assert got["out"] == out2[:n].cpu().numpy().tobytes()
    return got, results


# ---- the CPU cases in one batch of mixed connections --------------------------------------------

def _mixed_conns():
    T, B, K, P, Cl = AR.text, AR.binary, AR.cont, AR.ping, AR.close
    conns = [
        [P(b"first"), T(b"one"), P(b""), B(b"two"), P(b"last")],
        [],
        [T(b"frag", 0), P(b"mid"), K(b"ment", 0), P(b"dle"), K(b"s")],
        [K(b" wor", 0), P(b"p"), K(b"ld"), P(b"q")],
        [T(b"bye"), Cl(b"")],
        [T(b"bye"), Cl(b"\x03")],
        [T(b"bye"), Cl(b"\x03\xe8")],
        [T(b"bye"), Cl((b"\x03\xe8" + _payload(123))[:125])],
        [T(b"open", 0), Cl(b"\x03\xe8"), P(b"late"), K(b"ed"), T(b"after"), Cl(b"\x03\xe9again")],
        [B(b"bin"), T(b""), P(b"p"), B(b""), B(b"l", 0), K(b"ate")],
        [T(b"abcde"), P(b"pingpong"), B(b"fr", 0), K(b"agment")],
        [P(b""), T(_payload(300)), Cl(b"\x03\xe8bye")],
        [T(b"quiet"), P(b"z"), Cl(b"")],
        [P(b"1"), T(b"ok"), B(b"part", 0), P(b"2"), AR.Fr(0, 1, b"bad", rsv=True), P(b"never"), T(b"never")],
        [P(b"only")],
        [P(b"x"), K(b"more", 0)],
        [P(b"a"), B(_payload(62, 1), 0), P(b"b"), K(_payload(63, 2)), P(b"c"), T(_payload(126, 3)), P(_payload(125, 4))],
        [B(_payload(65535, 4)), P(b"between"), T(_payload(65536, 5)), AR.Fr(10, 1, b"pong"), B(_payload(65537, 6))],
    ]
    S = len(conns)
    srv = [1] * S
    srv[10] = srv[11] = 0
    en = [1] * S
    en[12] = 0
    pending = [None] * S
    pending[3], pending[14], pending[15] = (1, b"hello"), (2, b"kept"), (1, b"so far ")
    return conns, srv, en, pending


@pytest.mark.parametrize("flags", [0, 1, 2, 3])
def test_mixed_connections(torch, eng, flags):
    conns, srv, en, pending = _mixed_conns()
    keys = AR.keys_for(random.Random(3), 96)
    got, res = run_streams(torch, eng, conns, srv, en, keys, flags, pending=pending, gap=3)
    assert [r.n_delivered for r in res][13] == 4
    c8 = got["conn"][8]
    assert (c8["n_answers"], c8["n_replies"], c8["closed"]) == ((3, 3, 1) if flags & 2 else (1, 1, 1))
    assert got["conn"][12] == dict(AR.ZERO, first_answer=got["conn"][13]["first_answer"], closed=1)
    assert got["summary"]["n_closed_conns"] == 7 and got["conn"][15]["open_len"] == 11
    lo = got["out_off"][got["conn"][2]["first_answer"]]
    assert got["out"][lo:lo + 21] == b"\x8a\x03mid" b"\x8a\x03dle" b"\x81\x09fragments"  # the PONGs precede the echo


def test_client_connections_without_keys(torch, eng):
    conns, srv, en, pending = _mixed_conns()
    got, _ = run_streams(torch, eng, conns, srv, en, None, pending=pending)
    assert [c["status"] for c in got["conn"]] == [AR.NO_KEYS if s in (10, 11) else AR.OK for s in range(len(conns))]
    assert [q["status"] for q in got["reply"]][10:12] == [3, 3] and got["reply"][11]["closed"] == 1


def test_carry_missing(torch, eng):
    conns, srv, en, pending = _mixed_conns()
    carries = [p[1] if p else b"" for p in pending]
    carries[3] = b"hell"
    got, _ = run_streams(torch, eng, conns, srv, en, AR.keys_for(random.Random(3), 96), pending=pending,
                         carries=carries, silent={3: AR.NO_CARRY})
    assert got["conn"][3] == dict(AR.ZERO, first_answer=got["conn"][3]["first_answer"], status=AR.NO_CARRY)
    assert got["reply"][3] == AR.RZERO


@pytest.mark.parametrize("bad", ["data", "ping"])
def test_bad_payload_range(torch, eng, bad):
    """wire_len cut short of the last connection's last payload, a data frame's or a PING's:
    BAD_RANGE and nothing for it — not even the answers of the frames before — the others as
    before"""
    last = AR.binary(b"defgh") if bad == "data" else AR.ping(b"defgh")
    conns = [[AR.ping(b"a"), AR.binary(b"bc", 0)], [AR.ping(b"p"), AR.text(b"abc"), AR.close(b""), last]]
    wire = sum(len(AR.raw(c)) for c in conns)
    got, _ = run_streams(torch, eng, conns, wire_len=wire - 1, silent={1: AR.BAD_RANGE}, max_frames=8)
    assert got["conn"][1] == dict(AR.ZERO, first_answer=1, status=AR.BAD_RANGE, closed=1)
    assert got["reply"][1] == dict(AR.RZERO, status=2, closed=1)
    assert got["out"] == b"\x8a\x01a" and got["open"] == b"bc"


def test_failed_decode_results(torch, eng):
    """ERR_CAPACITY (max_frames too small: every connection): nothing is considered, no CLOSE
    counts as delivered, a carry passes through"""
    conns, srv, en, pending = _mixed_conns()
    keys = AR.keys_for(random.Random(4), 96)
    got, res = run_streams(torch, eng, conns, srv, en, keys, pending=pending, max_frames=10, ref=False)
    assert {r.first_status for r, c in zip(res, conns) if c} == {-10}
    assert got["summary"] == {"out_bytes": 0, "open_bytes": 16, "n_answers": 0, "n_replies": 0, "n_closed_conns": 0,
                              "status": AR.OK}
    assert got["open"] == b"hello" + b"kept" + b"so far "


# ---- scan blocks -------------------------------------------------------------------------------

@pytest.mark.parametrize("S", [1, SCAN_BLOCK - 1, SCAN_BLOCK, SCAN_BLOCK + 1, 2 * SCAN_BLOCK + 1])
def test_connection_counts(torch, eng, S):
    """S connections of 0-3 frames: the per-connection scans and the finish over 1, 2 and 3
    blocks of connections; every third connection a client, every seventh closed"""
    rng = random.Random(S)
    conns = []
    for s in range(S):
        fr = [AR.ping(bytes([s & 0xFF]) * (s % 5)), AR.text(bytes([s & 0xFF]) * (s % 11), s % 4 != 0), AR.ping(b"z")]
        if s % 7 == 0:
            fr.insert(1, AR.close(b"\x03\xe8"))
        conns.append(fr[:s % 4] if s % 5 else fr)
    srv = [0 if s % 3 == 0 else 1 for s in range(S)]
    got, _ = run_streams(torch, eng, conns, srv, None, AR.keys_for(rng, 4 * S), ref=(S <= SCAN_BLOCK + 1))
    assert got["summary"]["n_closed_conns"] == sum(1 for s in range(S) if s % 7 == 0 and (s % 5 == 0 or s % 4 >= 2))


@pytest.mark.parametrize("n", [SCAN_BLOCK - 1, SCAN_BLOCK, SCAN_BLOCK + 1, 2 * SCAN_BLOCK + 1])
@pytest.mark.parametrize("mode", ["pings", "data", "mix"])
def test_descriptor_ranges_at_the_scan_blocks(torch, eng, n, mode):
    """n descriptors exactly (max_frames = n) over three connections, the middle one straddling
    the block boundaries: a batch of only PINGs (== control_replies_streams), of only data (==
    echo_messages_streams), and a mix with replies on the first and last descriptor"""
    def frame(i):
        if mode == "pings" or (mode == "mix" and (i % 3 == 0 or i == n - 1)):
            return AR.ping(bytes([i & 0xFF]) * (i % 9))
        if mode == "data":
            return AR.binary(bytes([i & 0xFF]) * (i % 7))
        # the mix: PING, first fragment, last fragment, ... (the last descriptor is a PING)
        return AR.binary(bytes([i & 0xFF]) * (1 + i % 7), 0) if i % 3 == 1 else AR.cont(bytes([i & 0xFF]) * (i % 5))
    cuts = [0, 99, (n - 7) // 3 * 3, n]  # (multiples of 3: no message is cut between connections)
    conns = [[frame(i) for i in range(cuts[k], cuts[k + 1])] for k in range(3)]
    got, res = run_streams(torch, eng, conns, max_frames=n, ref=(n == SCAN_BLOCK + 1),
                           identity={"pings": "replies", "data": "echo", "mix": None}[mode])
    assert sum(r.n_delivered for r in res) == n
    if mode != "mix":
        assert got["summary"]["n_answers"] == n and got["summary"]["n_replies"] == (n if mode == "pings" else 0)


@pytest.mark.parametrize("client", [0, 1])
@pytest.mark.parametrize("kind", ["replies", "echo"])
def test_identity_with_the_existing_calls(torch, eng, client, kind):
    """no data frame in the batch: d_out and d_out_off are control_replies_streams'; no control
    frame: echo_messages_streams' — flags, CLOSEs, clients and carries included"""
    rng = random.Random(50 + client)
    conns, pending = [], []
    for s in range(40):
        if kind == "replies":
            fr = [rng.choice([AR.ping(rng.randbytes(rng.choice([0, 1, 17, 125]))), AR.close(b"\x03\xe8" + rng.randbytes(3)),
                              AR.Fr(10, 1, b"pong")]) for _ in range(rng.randint(0, 9))]
            pending.append(None)
        else:
            rows = [(rng.choice([1, 2]), rng.randbytes(rng.choice([0, 1, 125, 126, 3000]))) for _ in range(rng.randint(0, 5))]
            fr = ER.FR.fragment_randomly(rng, rows, p_ping=0)
            pend = (1, rng.randbytes(33)) if s % 4 == 0 else None
            pending.append(pend)
            if pend:
                fr = [AR.cont(b"end")] + fr
        conns.append(fr)
    for flags in ((0, 2) if kind == "replies" else (0, 1)):
        run_streams(torch, eng, conns, [1 - client] * 40, None, AR.keys_for(rng, 400), flags, pending=pending, identity=kind)


# ---- the emit tile -----------------------------------------------------------------------------

@pytest.mark.parametrize("client", [0, 1])
def test_pongs_at_the_tile_edge(torch, eng, client):
    """connection k's echo ends d bytes before a 64 KiB edge of d_out, d = 0 .. 15, and a PONG of
    12 (18) bytes follows: the PONG straddles the edge, a tile starts inside its header, inside its
    key, at its first payload byte and right after it"""
    hdr = 8 if client else 4
    conns, at, starts = [], 0, []
    for d in range(16):
        edge = (at // TILE + 1) * TILE
        if edge - d - at < 1000:
            edge += TILE
        n = edge - d - at - hdr  # the echo's payload
        assert 126 <= n <= 65535
        conns.append([AR.binary(_payload(n, d)), AR.ping(b"0123456789")])
        starts.append(edge - d)
        at = edge - d + (16 if client else 12)
    got, _ = run_streams(torch, eng, conns, [1 - client] * 16, None, AR.keys_for(random.Random(7), 64))
    assert [got["out_off"][2 * k + 1] for k in range(16)] == starts
    if not client:
        assert all(got["out"][s:s + 12] == b"\x8a\x0a0123456789" for s in starts)


@pytest.mark.parametrize("client", [0, 1])
def test_large_echo_followed_by_a_pong(torch, eng, client):
    """an echo of 64 KiB + 1 bytes (whole tiles from one source), then a PONG, then the same
    message in two fragments with a PING between them"""
    p = _payload(TILE + 1, 9)
    conns = [[AR.binary(p), AR.ping(b"after"), AR.text(p[:70], 0), AR.ping(b"inside"), AR.cont(p[70:]), AR.close(b"\x03\xe8")]]
    got, _ = run_streams(torch, eng, conns, [1 - client], None, AR.keys_for(random.Random(8), 8))
    assert got["conn"][0]["n_answers"] == 5 and got["conn"][0]["n_replies"] == 3


def test_client_batch_keys_by_merged_slot(torch, eng):
    """every frame of a client batch is masked with the key of its slot in the merged run"""
    rng = random.Random(61)
    conns = []
    for _ in range(30):
        rows = [(rng.choice([1, 2]), rng.randbytes(rng.choice([0, 3, 16, 200]))) for _ in range(rng.randint(1, 4))]
        fr = ER.FR.fragment_randomly(rng, rows, p_ping=0.6)
        fr.insert(rng.randrange(len(fr) + 1), AR.ping(rng.randbytes(20)))
        conns.append(fr)
    keys = AR.keys_for(rng, 400)
    got, _ = run_streams(torch, eng, conns, [0] * 30, None, keys)
    n = got["summary"]["n_answers"]
    assert n > 60 and got["summary"]["n_replies"] >= 30
    for j in range(n):
        f = got["out"][got["out_off"][j]:got["out_off"][j + 1]]
        h = 2 if f[1] & 0x7F < 126 else 4
        assert f[1] & 0x80 and f[h:h + 4] == AR.key_bytes(keys[j]), j


# ---- a three-call session ------------------------------------------------------------------------

def test_three_call_session(torch, eng):
    """every connection's frames cut into three calls at random frame boundaries — fragments and
    PINGs fall on both sides of a cut — each call's (d_open, d_open_off, open_bytes) the next
    call's (d_carry, d_carry_off, carry_len) as they lie, and a connection disabled once a call
    has seen its CLOSE.  The answers of the three calls together are the transcript's of the whole
    session fed in one go"""
    rng = random.Random(71)
    S = 20
    sess = []
    for s in range(S):
        rows = [(rng.choice([1, 2]), rng.randbytes(rng.choice([1, 5, 130, 700]))) for _ in range(rng.randint(2, 6))]
        fr = ER.FR.fragment_randomly(rng, rows, p_ping=0.7)
        for _ in range(3):
            fr.insert(rng.randrange(len(fr) + 1), AR.ping(rng.randbytes(rng.choice([0, 9]))))
        if s % 4 == 0:
            fr.insert(rng.randrange(len(fr) + 1), AR.close(b"\x03\xe8"))
        a, b = sorted(rng.randrange(len(fr) + 1) for _ in range(2))
        sess.append((fr, [fr[:a], fr[a:b], fr[b:]]))
    want = AR.expected_batch([fr for fr, _ in sess])
    answers = [[] for _ in range(S)]
    carry = carry_off = None
    carry_len, pend, enable = 0, [None] * S, [1] * S
    for call in range(3):
        parts = [AR.raw(p[call]) for _, p in sess]
        wire, st, _ = _streams(parts, None, None, pend)
        dw, dst = _dev(torch, wire), _dev(torch, st, 0)
        mf = wire.size // 2 + 1
        desc, res = eng.decode_streams(dw, dst, S, mf, wire_len=wire.size)
        o = Out(torch, S, mf, wire.size + 14 * mf + 4096, wire.size + 4096)
        eng.answer_messages_streams(dw, desc, mf, dst, res, S, mf, o.out_cap, enable=_dev(torch, np.array(enable, np.uint8), 0),
                                    carry=carry, carry_len=carry_len, carry_off=carry_off, wire_len=wire.size, **o.kw())
        torch.cuda.synchronize()
        got = o.read(eng)
        results = eng.read_stream_results(res, S)
        for s, c in enumerate(got["conn"]):
            assert c["status"] == AR.OK
            answers[s] += [got["out"][got["out_off"][j]:got["out_off"][j + 1]]
                           for j in range(c["first_answer"], c["first_answer"] + c["n_answers"])]
            if enable[s]:
                assert c["open_len"] == results[s].pending_bytes
            pend[s] = (c["open_opcode"], b"\0" * c["open_len"]) if enable[s] else None
            enable[s] = int(enable[s] and not c["closed"])
        carry, carry_off, carry_len = o.open, o.ooff, got["summary"]["open_bytes"]
    for s, c in enumerate(want["conn"]):
        assert b"".join(answers[s]) == want["out"][want["out_off"][c["first_answer"]]:][:c["out_len"]], s
        assert len(answers[s]) == c["n_answers"]


# ---- the in-place form -------------------------------------------------------------------------

@pytest.mark.parametrize("compact", [False, True])
@pytest.mark.parametrize("client", [0, 1])
def test_inplace_form(torch, eng, compact, client):
    """after decode_inplace with the wire; after decode_compact the data payloads lie in the
    arena and the control payloads in the wire, so only a batch without control payloads can pass
    the arena: there the PINGs are empty"""
    import uvhttp_amd as U
    rng = random.Random(40 + client)
    rows = [(rng.choice([1, 2]), rng.randbytes(rng.choice([0, 1, 7, 100, 300, 5000]))) for _ in range(60)]
    frames = ER.FR.fragment_randomly(rng, rows, p_ping=0)
    for _ in range(40):
        frames.insert(rng.randrange(len(frames) + 1), AR.ping(b"" if compact else rng.randbytes(rng.choice([0, 4, 125]))))
    frames += [AR.text(b"left open", 0), AR.ping(b""), AR.close(b"")]
    raw = AR.raw(frames)
    n = len(frames)
    wire = np.frombuffer(raw, np.uint8).copy()
    offs = np.cumsum([0] + [len(f.bytes) for f in frames[:-1]]).astype(np.uint64)
    dw = _dev(torch, wire)
    kw = dict(offsets=torch.from_numpy(offs.view(np.int64)).to("cuda"), wire_len=wire.size, max_frame_size=AR.MF,
              max_message_size=AR.MM, is_server=1 - client)
    keys = AR.keys_for(rng, n)
    o = Out(torch, 1, n, wire.size + 14 * n, wire.size)
    if compact:
        arena = torch.zeros(wire.size + 64, dtype=torch.uint8, device="cuda")
        desc, _, summ = eng.decode_compact(dw, n, arena, **kw)
        src, src_len = arena, wire.size
    else:
        desc, summ = eng.decode_inplace(dw, n, **kw)
        src, src_len = dw, wire.size
    eng.answer_messages_inplace(src, desc, n, summ, n, wire.size + 14 * n, is_server=1 - client,
                                mask_keys=_dev(torch, keys, 0), wire_len=src_len, **o.kw())
    torch.cuda.synchronize()
    got = o.read(eng)
    bs = eng.read_summary(summ)
    assert bs["n_delivered"] == n
    host = AR.host_batch(U, src[:src_len].cpu().numpy(), eng.read_desc(desc, n), [0], [n], [1 - client], None, keys,
                         max_answers=n)
    assert got == host
    assert host == AR.expected_batch([raw], [1 - client], None, keys, max_answers=n)
    assert got["open"] == b"left open" and got["conn"][0]["open_len"] == bs["pending_bytes"]
    assert got["summary"]["n_answers"] == 60 + 42 and got["summary"]["n_replies"] == 42 and got["conn"][0]["closed"] == 1


# ---- capacity ----------------------------------------------------------------------------------

def test_capacity_one_short(torch, eng):
    conns, srv, en, pending = _mixed_conns()
    keys = AR.keys_for(random.Random(8), 96)
    full, _ = run_streams(torch, eng, conns, srv, en, keys, pending=pending)
    n, nbytes, nopen = (full["summary"][k] for k in ("n_answers", "out_bytes", "open_bytes"))
    assert nopen > 0
    for kw in (dict(max_answers=n - 1, out_cap=nbytes, open_cap=nopen), dict(max_answers=n, out_cap=nbytes - 1, open_cap=nopen),
               dict(max_answers=n, out_cap=nbytes, open_cap=nopen - 1)):
        got, _ = run_streams(torch, eng, conns, srv, en, keys, pending=pending, ref=False, **kw)
        assert got["summary"] == dict(full["summary"], status=AR.ERR_CAPACITY)
        assert got["out"] == b"" and got["open"] == b"" and set(got["out_off"]) == {0} and set(got["open_off"]) == {0}
        assert {c["status"] for c in got["conn"]} == {AR.ERR_CAPACITY} and {q["status"] for q in got["reply"]} == {1}
        assert [q["closed"] for q in got["reply"]] == [c["closed"] for c in full["conn"]]
    # a second call with the reported sizes succeeds; without d_open, open_cap is not tested
    got, _ = run_streams(torch, eng, conns, srv, en, keys, pending=pending, ref=False, max_answers=n, out_cap=nbytes,
                         open_cap=nopen)
    assert got["out"] == full["out"] and got["open"] == full["open"] and got["conn"] == full["conn"]
    got, _ = run_streams(torch, eng, conns, srv, en, keys, pending=pending, ref=False, max_answers=n, out_cap=nbytes,
                         open_cap=0, with_open=False)
    assert got["out"] == full["out"] and got["open_off"] == full["open_off"]


# ---- a captured graph --------------------------------------------------------------------------

def test_graph_replay(torch, eng):
    """decode_streams + answer_messages_streams captured on a side stream after one uncaptured
    call of the shape, replayed over two batches of the same layout: the answers follow the bytes"""
    rng = random.Random(9)

    def conns_of(second_fin, op):
        return [[AR.text(rng.randbytes(20)), AR.binary(rng.randbytes(300), 0), AR.Fr(op, 1, b"12345"),
                 AR.cont(rng.randbytes(9), second_fin), AR.ping(rng.randbytes(5))] for _ in range(8)]
    a, b = conns_of(1, 9), conns_of(0, 10)
    (w0, st, _), (w1, st1, _) = _streams([AR.raw(c) for c in a]), _streams([AR.raw(c) for c in b])
    assert w0.size == w1.size and (st == st1).all()
    S, mf, cap = 8, 48, 4096
    dw, dst = _dev(torch, w0), _dev(torch, st, 0)
    desc = torch.zeros(mf * 32, dtype=torch.uint8, device="cuda")
    res = torch.zeros(S * 64, dtype=torch.uint8, device="cuda")
    o = Out(torch, S, mf, cap, cap)

    def both(stream=None):
        eng.decode_streams(dw, dst, S, mf, desc=desc, results=res, wire_len=w0.size, stream=stream)
        eng.answer_messages_streams(dw, desc, mf, dst, res, S, mf, cap, wire_len=w0.size, stream=stream, **o.kw())

    both()
    torch.cuda.synchronize()
    cs = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=cs):
        both(cs)
    for w, conns in ((w0, a), (w1, b), (w0, a)):
        dw[: w.size] = torch.from_numpy(w).to("cuda")
        o.buf.fill_(FILL)
        o.obuf.fill_(FILL)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        got = o.read(eng)
        assert got == AR.expected_batch([AR.raw(c) for c in conns], max_answers=mf)
        assert got["summary"]["n_answers"] == (32 if conns is a else 16)
        assert got["summary"]["n_replies"] == (16 if conns is a else 8)


# ---- the emit in several pieces -----------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 3])
def test_grid_pieces(torch, monkeypatch, n):
    """the main cases with the emit's tiles going out in launches of n workgroups
    (UVHTTP_WS_GRID_PIECE, the experiment build), against the references and, byte for byte,
    against an unsplit engine"""
    split = _engine(monkeypatch, {"UVHTTP_WS_GRID_PIECE": n})
    whole = _engine(monkeypatch, {})
    try:
        conns, srv, en, pending = _mixed_conns()
        keys = AR.keys_for(random.Random(3), 96)
        split.grid_pieces()
        got, _ = run_streams(torch, split, conns, srv, en, keys, pending=pending, gap=3, ref_eng=whole)
        passes, pieces, tiles = split.grid_pieces()
        assert tiles >= 5 and pieces >= -(-tiles // n) and pieces > passes
        p = _payload(65537, 1)
        big = [[AR.binary(p[:1], 0), AR.ping(b"mid"), AR.cont(p[1:]), AR.ping(b"after"), AR.text(_payload(40000, 2), 0)],
               [AR.text(_payload(65531, 3)), AR.ping(b"0123456789")]]
        got, _ = run_streams(torch, split, big, [0, 1], None, keys, ref_eng=whole)
        assert got["summary"]["out_bytes"] > 2 * TILE and got["summary"]["open_bytes"] == 40000
    finally:
        whole.close()
        split.close()


# ---- a seeded fuzz -----------------------------------------------------------------------------

@pytest.mark.parametrize("seed", range(2))
def test_fuzz_small_batches(torch, eng, seed):
    """30 batches per seed of at most 64 connections and 2 000 frames: random messages cut into
    fragments, PINGs, PONGs and CLOSEs anywhere, a failing frame part-way, carried-in messages,
    servers and clients, enable bits, every flag combination, sometimes a capacity too small:
    device == host twin"""
    rng = random.Random(7300 + seed)
    seen = 0
    for _ in range(30):
        conns, srv, pending = [], [], []
        budget = 2000
        for _ in range(rng.randint(1, 64)):
            rows = [(rng.choice([1, 2]), rng.randbytes(rng.choice([0, 1, 5, 15, 16, 17, 125, 126, 300, 2000])))
                    for _ in range(rng.randint(0, 5))]
            fr = ER.FR.fragment_randomly(rng, rows, p_ping=0.5)
            pend = None
            if rng.random() < 0.3:
                pend = (rng.choice([1, 2]), rng.randbytes(rng.choice([1, 3, 16, 200])))
                pre = [AR.cont(rng.randbytes(rng.choice([0, 2, 40])), 0) for _ in range(rng.randint(0, 2))]
                fr = pre + [AR.cont(rng.randbytes(rng.choice([0, 7])))] + fr if rng.random() < 0.7 else pre
            for _ in range(rng.randint(0, 4)):
                fr.insert(rng.randrange(len(fr) + 1),
                          rng.choice([AR.ping(rng.randbytes(rng.choice([0, 1, 15, 16, 17, 125]))), AR.Fr(10, 1, b"pong")]))
            for _ in range(rng.choice([0, 0, 0, 1, 2])):
                fr.insert(rng.randrange(len(fr) + 1), AR.close(rng.choice([b"", b"\x03", b"\x03\xe8", b"\x03\xe8why"])))
            if rng.random() < 0.15 and fr:
                fr.insert(rng.randrange(len(fr) + 1), AR.Fr(2, 1, b"bad", rsv=True))
            fr = fr[:budget]
            budget -= len(fr)
            conns.append(AR.raw(fr))
            srv.append(rng.choice([1, 1, 0]))
            pending.append(pend)
        keys = AR.keys_for(rng, 800) if rng.random() < 0.8 else None
        enable = [rng.choice([1, 1, 1, 0]) for _ in conns] if rng.random() < 0.5 else None
        kw = {}
        if rng.random() < 0.2:
            kw = dict(max_answers=rng.randint(0, 60), out_cap=rng.randint(0, 20000), open_cap=rng.randint(0, 300))
        got, _ = run_streams(torch, eng, conns, srv, enable, keys, rng.choice([0, 1, 2, 3]), pending=pending,
                             gap=rng.choice([0, 1, 5]), ref=False, with_open=rng.random() < 0.9, **kw)
        seen += got["summary"]["n_answers"]
    assert seen > 1000


# ---- arguments ---------------------------------------------------------------------------------

def test_arguments(torch, eng):
    import uvhttp_amd as U
    wire, st, _ = _streams([AR.raw([AR.text(b"ok"), AR.ping(b"p")])])
    dw, dst = _dev(torch, wire), _dev(torch, st, 0)
    desc, res = eng.decode_streams(dw, dst, 1, 4, wire_len=wire.size)
    summ = torch.zeros(64, dtype=torch.uint8, device="cuda")
    o = Out(torch, 1, 4, 64, 64)
    torch.cuda.synchronize()

    class Null:
        def data_ptr(self):
            return None

    base = dict(wire=dw, desc=desc, streams_dev=dst, results=res, batch_summary=summ, mask_keys=None, carry=None,
                carry_off=None, **o.kw())
    del base["open_cap"]

    def streams(max_frames=4, max_answers=4, run_stride=8, n_streams=1, flags=0, **kw):
        a = dict(base, **kw)
        eng.answer_messages_streams(a["wire"], a["desc"], max_frames, a["streams_dev"], a["results"], n_streams,
                                    max_answers, 64, mask_keys=a["mask_keys"], flags=flags, carry=a["carry"],
                                    carry_off=a["carry_off"], out=a["out"], out_off=a["out_off"], runs=a["runs"],
                                    run_stride=run_stride, open=a["open"], open_cap=64, open_off=a["open_off"],
                                    conn=a["conn"], summary=a["summary"], reply_conn=a["reply_conn"], wire_len=wire.size)

    def inplace(max_answers=4, run_stride=8, flags=0, **kw):
        a = dict(base, **kw)
        eng.answer_messages_inplace(a["wire"], a["desc"], 1, a["batch_summary"], max_answers, 64,
                                    mask_keys=a["mask_keys"], flags=flags, out=a["out"], out_off=a["out_off"],
                                    runs=a["runs"], run_stride=run_stride, open=a["open"], open_cap=64,
                                    open_off=a["open_off"], conn=a["conn"], summary=a["summary"],
                                    reply_conn=a["reply_conn"], wire_len=wire.size)

    streams()
    inplace()
    streams(flags=3, reply_conn=None)
    for call, names in ((streams, ["wire", "desc", "streams_dev", "results", "out", "out_off", "open_off", "conn", "summary"]),
                        (inplace, ["wire", "desc", "batch_summary", "out", "out_off", "open_off", "conn", "summary"])):
        for name in names:
            with pytest.raises(U.GpuError, match="rc=-1"):
                call(**{name: Null()})
            view = base[name].view(torch.uint8) if name in ("out_off", "open_off") else base[name]
            with pytest.raises(U.GpuError, match="rc=-1"):
                call(**{name: view[1:]})
        for bad in (dict(mask_keys=dw[1:]), dict(runs=dw[2:]), dict(runs=o.runs, run_stride=4), dict(open=o.obuf[1:]),
                    dict(runs=o.runs, run_stride=10), dict(max_answers=(1 << 28) + 1), dict(reply_conn=o.reply[1:]),
                    dict(flags=4), dict(flags=0x80000001)):
            with pytest.raises(U.GpuError, match="rc=-1"):
                call(**bad)
    for bad in (dict(carry=dw[1:]), dict(carry_off=o.ooff.view(torch.uint8)[1:]), dict(max_frames=(1 << 28) + 1),
                dict(n_streams=(1 << 31) + 1)):
        with pytest.raises(U.GpuError, match="rc=-1"):
            streams(**bad)
    torch.cuda.synchronize()
