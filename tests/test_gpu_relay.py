"""uvhttp_ws_gpu_relay_messages_streams after decode_streams / decode_reads: device == the host
twin uvhttp_ws_relay_messages, byte for byte, in d_out, d_out_off, d_rooms, the receivers' runs,
d_open, d_open_off, the per-connection results and the summary, with guard bytes around each —
and == the room lists process_data's on_message makes (tests/_relay_ref.py) — for the CPU cases as
one batch, the identity room map against the device echo, the scan-block and radix-digit edges,
a room crossing an emit tile, a large message, two calls chained through d_open -> d_carry,
changing shapes on one engine, the no-sync chain into uvhttp_tls_gpu_seal_frames with the fan-out
opened per receiver, a captured graph, every chunked pass in several pieces and a seeded fuzz."""
import ctypes as C
import random

import numpy as np
import pytest

import _echo_ref as ER
import _oracle as O
import _relay_ref as RR
import _tls_send_ref as TS
from test_gpu_epoch_wrap import _engine

pytestmark = pytest.mark.gpu
SCAN_BLOCK = 256   # connections per workgroup of the scans and of a radix pass (ws_echo_gpu.hip: kBlock)
TILE = 65536       # output bytes per workgroup of the emit (kTile)
GUARD, FILL = 64, 0xA5
FAILED = (-9, -10, -11)


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


def _dev(torch, a, pad=64):
    a = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    d = torch.zeros(max(16, a.size + pad), dtype=torch.uint8, device="cuda")
    if a.size:
        d[: a.size] = torch.from_numpy(a.copy()).to("cuda")
    return d


def _streams(conns, is_server=None, reads=None, pending=None, gap=0):
    wire, st = ER.streams_of(conns, is_server, pending, gap)
    read_end = []
    for s in range(len(conns)):
        if reads is not None and reads[s] is not None:
            st[s]["first_read"], st[s]["n_reads"] = len(read_end), len(reads[s])
            read_end += list(np.cumsum([len(r) for r in reads[s]]))
    return wire, st, read_end


class Out:
    """guarded device outputs of one relay call, and their host copies"""

    def __init__(self, torch, S, n_rooms, n_recv, max_out, out_cap, open_cap, with_open=True):
        t = torch
        self.S, self.R, self.K, self.max_out, self.out_cap, self.open_cap = S, n_rooms, n_recv, max_out, out_cap, open_cap
        self.buf = t.full((GUARD + out_cap + GUARD,), FILL, dtype=t.uint8, device="cuda")
        self.out = self.buf[GUARD:GUARD + out_cap] if out_cap else self.buf[GUARD:GUARD + 1]
        self.obuf = t.full((GUARD + open_cap + GUARD,), FILL, dtype=t.uint8, device="cuda")
        self.open = (self.obuf[GUARD:GUARD + open_cap] if open_cap else self.obuf[GUARD:GUARD + 1]) if with_open else None
        self.off = t.full((max_out + 2,), -7, dtype=t.int64, device="cuda")
        self.ooff = t.full((S + 2,), -7, dtype=t.int64, device="cuda")
        self.rooms = t.full((32 * n_rooms + 32,), FILL, dtype=t.uint8, device="cuda")
        self.sends = t.full((2 * n_recv + 2,), 0x5A5A5A5A, dtype=t.int32, device="cuda")
        self.conn = t.full((32 * S + 32,), FILL, dtype=t.uint8, device="cuda")
        self.summ = t.full((32,), FILL, dtype=t.uint8, device="cuda")

    def kw(self):
        return dict(out=self.out, out_off=self.off, rooms=self.rooms, sends=self.sends, open=self.open,
                    open_cap=self.open_cap, open_off=self.ooff, conn=self.conn, summary=self.summ)

    def read(self, eng):
        summ = eng.read_relay_summary(self.summ)
        ok = summ["status"] == RR.OK
        buf, obuf = self.buf.cpu().numpy(), self.obuf.cpu().numpy()
        n = summ["out_bytes"] if ok else 0
        m = summ["open_bytes"] if ok and self.open is not None else 0
        assert (buf[:GUARD] == FILL).all() and (buf[GUARD + n:] == FILL).all(), "d_out written outside the frames"
        assert (obuf[:GUARD] == FILL).all() and (obuf[GUARD + m:] == FILL).all(), "d_open written outside the messages"
        off, ooff = self.off.cpu().numpy(), self.ooff.cpu().numpy()
        assert off[-1] == -7 and ooff[-1] == -7, "an offset table written past its end"
        sends = self.sends.cpu().numpy().view(np.uint32)
        assert (sends[2 * self.K:] == 0x5A5A5A5A).all()
        assert (self.conn.cpu().numpy()[32 * self.S:] == FILL).all()
        assert (self.rooms.cpu().numpy()[32 * self.R:] == FILL).all()
        return {"out": buf[GUARD:GUARD + n].tobytes(), "out_off": [int(x) for x in off[:-1]],
                "open": obuf[GUARD:GUARD + m].tobytes(), "open_off": [int(x) for x in ooff[:-1]],
                "conn": eng.read_echo_conns(self.conn, self.S), "rooms": eng.read_relay_rooms(self.rooms, self.R),
                "sends": [(int(sends[2 * k]), int(sends[2 * k + 1])) for k in range(self.K)], "summary": summ}


def run_relay(torch, eng, conns, room, n_rooms, recv_room=(), is_server=None, enable=None, flags=0, reads=None,
              pending=None, carries=None, gap=0, max_frames=None, max_out=None, out_cap=None, open_cap=None,
              with_open=True, ref=True, silent=None, ref_eng=None):
    """decode_streams (decode_reads with `reads`) then relay_messages_streams, no host sync between;
    everything the call writes against the host twin over the device's own decode, and (ref)
    against the on_message reference -> (got, stream results)"""
    import uvhttp_amd as U
    conns = [ER.raw(c) for c in conns]
    S, K = len(conns), len(recv_room)
    wire, st, read_end = _streams(conns, is_server, reads, pending, gap)
    dw, dst = _dev(torch, wire), _dev(torch, st, 0)
    re_dev = torch.tensor(read_end or [0], dtype=torch.int64, device="cuda") if reads is not None else None
    if max_frames is None:
        max_frames = len(wire) // 2 + 1
    carry, coff = ER.carry_tables(pending, S)
    if carries is not None:
        carry, coff = ER.carry_tables([(0, c) for c in carries], S)
    has_carry = pending is not None or carries is not None
    max_out = max_frames if max_out is None else max_out
    out_cap = 10 * max_out + len(wire) + len(carry) if out_cap is None else out_cap
    open_cap = len(wire) + len(carry) if open_cap is None else open_cap
    d_en = _dev(torch, np.array(enable, np.uint8), 0) if enable is not None else None
    d_room = _dev(torch, np.array(room, np.uint32), 0)
    d_recv = _dev(torch, np.array(recv_room, np.uint32), 0) if K else None
    d_carry = _dev(torch, np.frombuffer(carry, np.uint8)) if has_carry else None
    d_coff = torch.tensor(coff, dtype=torch.int64, device="cuda") if has_carry else None
    o = Out(torch, S, n_rooms, K, max_out, out_cap, open_cap, with_open)
    desc, res = eng.decode_streams(dw, dst, S, max_frames, wire_len=wire.size, read_end=re_dev, n_reads=len(read_end))

    def call(e, oo):
        kw = oo.kw()
        if not K:
            kw["sends"] = None
        e.relay_messages_streams(dw, desc, max_frames, dst, res, S, d_room, n_rooms, max_out, out_cap, enable=d_en,
                                 flags=flags, carry=d_carry, carry_len=len(carry), carry_off=d_coff, recv_room=d_recv,
                                 n_receivers=K, wire_len=wire.size, **kw)
        torch.cuda.synchronize()
        return oo.read(e)

    got = call(eng, o)
    results = eng.read_stream_results(res, S)
    hw, hd = dw[: wire.size].cpu().numpy(), eng.read_desc(desc, max_frames)
    host = U.relay_messages(hw, hd, max_frames, st, res[: 64 * S], room, n_rooms, enable, flags,
                            carry if has_carry else None, coff if has_carry else None, recv_room,
                            out_cap=max(out_cap, 10 * max_frames + len(wire) + len(carry)),
                            max_frames_out=max(max_out, max_frames), open_cap=max(open_cap, len(wire) + len(carry)))
    host["out_off"] = host["out_off"][:max_out + 1] if host["summary"]["n_frames"] <= max_out else host["out_off"]
    assert got == RR.want(host, max_out, out_cap, open_cap, with_open)
    if got["summary"]["status"] == RR.OK:
        for s, c in enumerate(got["conn"]):  # the open message is the decoder's
            if c["status"] == RR.OK and (enable is None or enable[s]) and results[s].first_status not in FAILED:
                assert c["open_len"] == results[s].pending_bytes, s
    if ref:
        want = RR.expected(conns, room, n_rooms, recv_room, is_server, enable, flags, reads, pending, silent or {}, max_out)
        assert host == want
    if ref_eng is not None:  # the same call on an unsplit engine: byte for byte
        assert call(ref_eng, Out(torch, S, n_rooms, K, max_out, out_cap, open_cap, with_open)) == got
    return got, results


# ---- the CPU cases as one batch ------------------------------------------------------------------

@pytest.mark.parametrize("flags", [0, RR.SERVER_SEND])
def test_mixed_rooms(torch, eng, flags):
    m = RR.mixed_case()
    got, res = run_relay(torch, eng, flags=flags, gap=3, **m)
    assert [r["n_frames"] for r in got["rooms"]] == ([5, 3, 1, 0, 5, 1] if flags else [5, 3, 1, 0, 6, 1])
    assert got["conn"][9]["status"] == RR.BAD_ROOM and got["summary"]["n_bad_rooms"] == 1
    assert got["summary"]["n_bad_receivers"] == 2 and got["sends"][0] == got["sends"][7] == (0, 5)
    assert got["conn"][14]["open_len"] == 4 and got["conn"][13]["open_len"] == 204


def test_statuses_and_their_precedence(torch, eng):
    T = ER.text
    conns = [[T(b"zero")], [ER.cont(b" world")], [ER.cont(b"x")], [T(b"three")], [T(b"four")], [T(b"ok")]]
    pending = [None, (1, b"hello"), (1, b"abc"), None, None, None]
    carries = [b"", b"hell", b"abc", b"", b"", b""]
    room = [0, 7, 1, 7, 0, 1]
    got, _ = run_relay(torch, eng, conns, room, 2, [0, 1, 2], enable=[1, 1, 1, 1, 0, 1], pending=pending,
                       carries=carries, silent={1: RR.NO_CARRY})
    assert [c["status"] for c in got["conn"]] == [RR.OK, RR.NO_CARRY, RR.OK, RR.BAD_ROOM, RR.OK, RR.OK]
    assert got["out"] == b"\x81\x04zero\x81\x04abcx\x81\x02ok" and got["sends"] == [(0, 1), (1, 2), (0, 0)]


def test_bad_payload_range_ranks_after_bad_room(torch, eng):
    """wire_len cut short of the last payload of two senders: the one in a room says BAD_RANGE, the
    one in none BAD_ROOM"""
    import uvhttp_amd as U
    conns = [ER.raw(c) for c in ([ER.text(b"a"), ER.binary(b"bc", 0)], [ER.text(b"first"), ER.text(b"second")],
                                 [ER.text(b"third"), ER.text(b"fourth")])]
    for room, want in (([0, 1, 1], [RR.OK, RR.OK, RR.BAD_RANGE]), ([0, 1, 5], [RR.OK, RR.OK, RR.BAD_ROOM])):
        wire, st, _ = _streams(conns)
        dw, dst = _dev(torch, wire), _dev(torch, st, 0)
        desc, res = eng.decode_streams(dw, dst, 3, 8, wire_len=wire.size)
        short = wire.size - 2
        o = Out(torch, 3, 2, 2, 8, 256, 64)
        eng.relay_messages_streams(dw, desc, 8, dst, res, 3, _dev(torch, np.array(room, np.uint32), 0), 2, 8, 256,
                                   recv_room=_dev(torch, np.array([1, 0], np.uint32), 0), n_receivers=2, wire_len=short,
                                   **o.kw())
        torch.cuda.synchronize()
        got = o.read(eng)
        host = U.relay_messages(dw[: wire.size].cpu().numpy(), eng.read_desc(desc, 8), 8, st, res[:192], room, 2,
                                recv_room=[1, 0], wire_len=short, out_cap=256, max_frames_out=8, open_cap=64)
        assert got == host and [c["status"] for c in got["conn"]] == want
        assert got["out"] == b"\x81\x01a\x81\x05first\x81\x06second" and got["open"] == b"bc"


# ---- the identity room map against the device echo ------------------------------------------------

@pytest.mark.parametrize("flags", [0, RR.SERVER_SEND])
def test_identity_rooms_equal_the_device_echo(torch, eng, flags):
    m = RR.mixed_case()
    conns = [ER.raw(c) for c in m["conns"]]
    S = len(conns)
    wire, st, _ = _streams(conns, None, None, m["pending"])
    dw, dst = _dev(torch, wire), _dev(torch, st, 0)
    mf = wire.size // 2 + 1
    cap = wire.size + 14 * mf + 300
    carry, coff = ER.carry_tables(m["pending"], S)
    d_carry, d_coff = _dev(torch, np.frombuffer(carry, np.uint8)), torch.tensor(coff, dtype=torch.int64, device="cuda")
    desc, res = eng.decode_streams(dw, dst, S, mf, wire_len=wire.size)
    d_open = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    runs = torch.zeros(2 * S, dtype=torch.int32, device="cuda")
    e_out, e_off, e_ooff, e_conn, e_sum = eng.echo_messages_streams(
        dw, desc, mf, dst, res, S, mf, cap, flags=flags, carry=d_carry, carry_len=len(carry), carry_off=d_coff,
        runs=runs, open=d_open, open_cap=cap, wire_len=wire.size)
    o = Out(torch, S, S, S, mf, cap, cap)
    ident = _dev(torch, np.arange(S, dtype=np.uint32), 0)
    eng.relay_messages_streams(dw, desc, mf, dst, res, S, ident, S, mf, cap, flags=flags, carry=d_carry,
                               carry_len=len(carry), carry_off=d_coff, recv_room=ident, n_receivers=S,
                               wire_len=wire.size, **o.kw())
    torch.cuda.synchronize()
    got, es = o.read(eng), eng.read_echo_summary(e_sum)
    assert es["n_echoes"] > 10 and es["open_bytes"] > 0
    assert got["summary"] == {"out_bytes": es["out_bytes"], "open_bytes": es["open_bytes"], "n_frames": es["n_echoes"],
                              "status": RR.OK, "n_bad_rooms": 0, "n_bad_receivers": 0}
    assert got["out"] == e_out[: es["out_bytes"]].cpu().numpy().tobytes()
    assert got["out_off"] == [int(x) for x in e_off.cpu().numpy()]
    assert got["open"] == d_open[: es["open_bytes"]].cpu().numpy().tobytes()
    assert got["open_off"] == [int(x) for x in e_ooff.cpu().numpy()]
    assert got["conn"] == eng.read_echo_conns(e_conn, S)
    assert got["sends"] == [tuple(int(x) for x in runs.cpu().numpy().view(np.uint32)[2 * s:2 * s + 2]) for s in range(S)]


# ---- scan-block and radix-digit edges -------------------------------------------------------------

@pytest.mark.parametrize("rooms", ["one", "two", "257", "n", "high"])
@pytest.mark.parametrize("S", [SCAN_BLOCK - 1, SCAN_BLOCK, SCAN_BLOCK + 1, 2 * SCAN_BLOCK + 1])
def test_connection_blocks_and_radix_digits(torch, eng, S, rooms):
    """S connections over 1, 2, 257 and S rooms (one and two radix passes, room ids scattered and
    descending), and over rooms that differ only above bit 8; a connection sends 0, 1 or 2
    messages, one in every block fragments its own"""
    n_rooms = {"one": 1, "two": 2, "257": 257, "n": S, "high": 1024}[rooms]
    room = {"one": [0] * S, "two": [(s * 5 + 1) % 2 for s in range(S)], "257": [(s * 101) % 257 for s in range(S)],
            "n": [S - 1 - s for s in range(S)], "high": [((s * 3) % 4) << 8 for s in range(S)]}[rooms]

    def sender(s):
        if s % 7 == 3:
            return []
        if s % SCAN_BLOCK == 9:
            return [ER.binary(b"fr", 0), ER.ping(b""), ER.cont(b"ag%d" % s)]
        return [ER.text(b"%d" % s)] + ([ER.binary(bytes([s & 0xFF]) * (s % 11))] if s % 3 == 0 else [])
    recv = [0, n_rooms - 1, n_rooms // 2, 256 % n_rooms, n_rooms]
    got, _ = run_relay(torch, eng, [sender(s) for s in range(S)], room, n_rooms, recv, ref=(S == SCAN_BLOCK + 1))
    assert got["summary"]["n_frames"] == sum(0 if s % 7 == 3 else 1 if s % SCAN_BLOCK == 9 or s % 3 else 2 for s in range(S))
    assert sum(r["n_frames"] for r in got["rooms"]) == got["summary"]["n_frames"]
    if rooms == "high":
        assert [r for r, x in enumerate(got["rooms"]) if x["n_frames"]] == [0, 256, 512, 768]


# ---- tiles ----------------------------------------------------------------------------------------

def test_room_crossing_a_tile_with_scattered_senders(torch, eng):
    """three rooms of four senders each, interleaved, 20 000 bytes a sender: every room's frames
    cross a 64 KiB tile, and the records of one tile come from descriptors far apart"""
    conns = [[ER.binary(RR.payload(20000 + s, s), 0), ER.cont(RR.payload(100, s + 1))] if s % 2 else
             [ER.text(RR.payload(20100 + s, s))] for s in range(12)]
    got, _ = run_relay(torch, eng, conns, [s % 3 for s in range(12)], 3, [0, 1, 2])
    assert all(r["out_len"] > TILE and r["n_frames"] == 4 for r in got["rooms"])
    assert got["rooms"][1]["out_off"] // TILE != (got["rooms"][1]["out_off"] + got["rooms"][1]["out_len"]) // TILE


def test_large_message(torch, eng):
    """a 70 000-byte message (a 10-byte header, whole tiles from one source) between short ones of
    the same room, one fragment and three"""
    p = RR.payload(70000, 5)
    conns = [[ER.text(b"lead")], [ER.binary(p)], [ER.text(b"mid")], [ER.text(p[:1], 0), ER.cont(p[1:69999], 0), ER.cont(p[69999:])],
             [ER.text(b"tail")]]
    got, _ = run_relay(torch, eng, conns, [1, 0, 0, 1, 0], 2, [0, 1])
    assert got["rooms"][0]["out_len"] == 10 + 70000 + 5 + 6 and got["rooms"][1]["n_frames"] == 2
    lo = got["out_off"][3] + 6
    assert got["out"][lo:lo + 10] == b"\x81\x7f" + (70000).to_bytes(8, "big") and got["out"][lo + 10:lo + 70010] == p


# ---- two calls chained through d_open -> d_carry --------------------------------------------------

def test_chained_calls_at_every_frame_boundary(torch, eng):
    """a 3-message, 7-fragment sender cut at every frame boundary (sender 2k of call 1 gets frames
    [0, k), of call 2 the rest), beside a sender of the same room that completes messages in both
    calls; call 1's (d_open, d_open_off, open_bytes) are call 2's (d_carry, d_carry_off, carry_len)
    as they lie, though the rooms differ between the calls.  Both calls together give the room the
    messages of one call over the whole wire"""
    frames = [ER.text(b"first ", 0), ER.cont(b"message", 0), ER.cont(b" done"), ER.binary(RR.payload(130, 1), 0),
              ER.cont(RR.payload(70, 2)), ER.text(b"x", 0), ER.cont(b"yz")]
    cuts = list(range(1, 7))
    S = 2 * len(cuts)
    other1 = [ER.text(b"other one"), ER.binary(b"other", 0)]
    other2 = [ER.cont(b" two"), ER.text(b"other three")]
    whole, _ = run_relay(torch, eng, [frames], [0], 1)
    msgs = RR.room_lists(whole)[0]
    o_whole, _ = run_relay(torch, eng, [other1 + other2], [0], 1)
    o_msgs = RR.room_lists(o_whole)[0]

    room1 = [k // 2 for k in range(S)]                 # call 1: the pair (2k, 2k + 1) shares room k
    room2 = [len(cuts) - 1 - k // 2 for k in range(S)]  # call 2: the rooms reversed
    c1 = [c for k in cuts for c in (frames[:k], other1)]
    c2 = [c for k in cuts for c in (frames[k:], other2)]
    w1, st1, _ = _streams([ER.raw(c) for c in c1])
    dw1, dst1 = _dev(torch, w1), _dev(torch, st1, 0)
    desc1, res1 = eng.decode_streams(dw1, dst1, S, 64, wire_len=w1.size)
    o1 = Out(torch, S, len(cuts), 0, 64, 4096, 4096)
    eng.relay_messages_streams(dw1, desc1, 64, dst1, res1, S, _dev(torch, np.array(room1, np.uint32), 0), len(cuts), 64,
                               4096, wire_len=w1.size, **dict(o1.kw(), sends=None))
    torch.cuda.synchronize()
    got1 = o1.read(eng)
    r1 = eng.read_stream_results(res1, S)
    pend2 = [(c["open_opcode"], b"\0" * r.pending_bytes) for c, r in zip(got1["conn"], r1)]
    w2, st2, _ = _streams([ER.raw(c) for c in c2], None, None, pend2)
    dw2, dst2 = _dev(torch, w2), _dev(torch, st2, 0)
    desc2, res2 = eng.decode_streams(dw2, dst2, S, 64, wire_len=w2.size)
    o2 = Out(torch, S, len(cuts), 0, 64, 4096, 4096)
    eng.relay_messages_streams(dw2, desc2, 64, dst2, res2, S, _dev(torch, np.array(room2, np.uint32), 0), len(cuts), 64,
                               4096, carry=o1.open, carry_len=got1["summary"]["open_bytes"], carry_off=o1.ooff,
                               wire_len=w2.size, **dict(o2.kw(), sends=None))
    torch.cuda.synchronize()
    got2 = o2.read(eng)
    assert all(c["status"] == RR.OK for c in got2["conn"]) and got2["open"] == b""
    for s in range(S):
        both = []
        for g in (got1, got2):
            c = g["conn"][s]
            both += [g["out"][g["out_off"][j]:g["out_off"][j + 1]] for j in range(c["first_echo"], c["first_echo"] + c["n_echoes"])]
        assert both == (o_msgs if s % 2 else msgs), s
    for k in range(len(cuts)):  # a room's run is its two senders' frames, the lower index first
        a, b = got2["conn"][S - 2 - 2 * k], got2["conn"][S - 1 - 2 * k]
        assert got2["rooms"][k]["first_frame"] == a["first_echo"] and b["first_echo"] == a["first_echo"] + a["n_echoes"]
        assert got2["rooms"][k]["n_frames"] == a["n_echoes"] + b["n_echoes"]


# ---- one engine, changing shapes ------------------------------------------------------------------

def test_changing_rooms_and_shapes_on_one_engine(torch):
    import uvhttp_amd as U
    e = U.GpuEngine(0)
    try:
        rng = random.Random(5)
        for S, n_rooms in ((3, 1), (300, 300), (40, 70000), (2, 0), (600, 3), (1, 200000), (300, 2)):
            conns = [[ER.text(b"%d/%d" % (s, n_rooms))] * (s % 3) for s in range(S)]
            room = [rng.randrange(n_rooms + 1) if s % 5 == 0 else rng.randrange(max(1, n_rooms)) for s in range(S)]
            recv = [rng.randrange(n_rooms + 1) for _ in range(S // 2 + 1)]
            got, _ = run_relay(torch, e, conns, room, n_rooms, recv, ref=False)
            assert got["summary"]["n_frames"] == sum(s % 3 for s in range(S) if room[s] < n_rooms)
    finally:
        e.close()


# ---- the no-sync chain ----------------------------------------------------------------------------

def test_chain_records_in_sealed_fan_out(torch):
    """seal_records (the clients' messages) -> open_records -> ws_streams -> decode_reads ->
    relay_messages_streams -> seal_frames with n_sends = the receivers and a pre-filled sends
    table: no host read before the end.  24 connections in 4 rooms, every one a receiver with a
    key of its own: the oracle opens every receiver's records into its room's frame list"""
    import uvhttp_amd as U
    t = torch
    rng = random.Random(79)
    S, R = 24, 4
    room = [(s * 7 + s // 5) % R for s in range(S)]
    kinds = [TS.KEY_KINDS[rng.randrange(6)] for _ in range(S)]
    keys = np.concatenate([TS.make_key(rng, k) for k in kinds] + [TS.make_key(rng, k) for k in kinds])
    plains, recs_rows, tls_st, reads = [], [], np.zeros(S, O.TLS_STREAM_DT), []
    src_pos, out_pos = 0, 0
    for c in range(S):
        rows = [(rng.choice([1, 2]), rng.randbytes(rng.choice([0, 1, 20, 200, 3000]))) for _ in range(rng.randint(0, 4))]
        plain = ER.raw(ER.FR.fragment_randomly(rng, rows))
        seq0, begin, pos, j, rd = rng.randrange(1 << 40), out_pos, 0, 0, []
        while pos < len(plain):
            n = min(len(plain) - pos, rng.choice([1, 7, 40, 500, 16384]))
            recs_rows.append((src_pos + pos, out_pos, seq0 + j, n, c, 23, 0))
            rd.append(plain[pos:pos + n])
            out_pos += n + TS.overhead(keys[c])
            pos += n
            j += 1
        tls_st[c] = (begin, out_pos - begin, seq0, c, 0)
        plains.append(plain)
        reads.append(rd or None)
        src_pos += len(plain)
    seal = np.array(recs_rows, O.TLS_SEAL_DT)
    dev = lambda a: t.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to("cuda")  # noqa: E731
    eng_t, eng_w = U.TlsEngine(0), U.GpuEngine(0)
    d_keys, d_src = dev(keys), dev(np.frombuffer(b"".join(plains), np.uint8))
    cipher = t.zeros(out_pos + 64, dtype=t.uint8, device="cuda")
    max_records = len(seal) + 1
    plain_cap = max(16, out_pos)
    plain_out = t.zeros(plain_cap + 64, dtype=t.uint8, device="cuda")
    ws = []
    for c in range(S):
        s = U.Stream()
        conn = U.WsConnection(1, ER.MF, ER.MM)
        U.lib().uvhttp_ws_stream_init(conn.ptr, 0, 0, C.byref(s))
        ws.append(bytes(s))
    ws_dev = dev(np.frombuffer(b"".join(ws), np.uint8))
    read_end = t.zeros(max_records, dtype=t.int64, device="cuda")
    max_frames = max_out = 1024
    out_cap = src_pos + 10 * max_out
    sends = np.zeros(S, TS.TLS_SEND_DT)
    seq_s = [rng.randrange(1 << 40) for _ in range(S)]
    for c in range(S):
        sends[c] = (seq_s[c], 0xDEAD, 0xBEEF, S + c, 23, 0, 0)  # first_frame / n_frames: the call's
    d_sends = dev(sends)
    fan = max(room.count(r) for r in range(R))  # the largest room's members
    max_out_records = fan * (max_out + out_cap // 16384 + 1)
    sealed = t.zeros(fan * out_cap + max_out_records * 64, dtype=t.uint8, device="cuda")
    d_room = dev(np.array(room, np.uint32))

    eng_t.seal_records(d_src, dev(seal), len(seal), d_keys, len(keys), cipher[:out_pos])
    tls_dev = dev(tls_st)
    recs, res = eng_t.open_records(cipher, d_keys, len(keys), tls_dev, S, max_records, plain_out[:plain_cap],
                                   wire_len=out_pos)
    eng_t.ws_streams(res, recs, S, tls_dev, plain_out, ws_dev, read_end)
    desc, wres = eng_w.decode_streams(plain_out, ws_dev, S, max_frames, wire_len=plain_cap, read_end=read_end,
                                      n_reads=max_records)
    out, off, _, rconn, rrooms, rsum = eng_w.relay_messages_streams(
        plain_out, desc, max_frames, ws_dev, wres, S, d_room, R, max_out, out_cap, recv_room=d_room, n_receivers=S,
        sends=d_sends[8:], send_stride=32, wire_len=plain_cap)
    _, sres, ssum = eng_t.seal_frames(out, off, max_out, d_sends, S, d_keys, len(keys), max_out_records, sealed,
                                      frames_len=out_cap)
    t.cuda.synchronize()  # the first host read

    want = RR.expected(plains, room, R, room, reads=reads, max_frames_out=max_out)
    lists = RR.room_lists(want)
    assert eng_w.read_relay_summary(rsum) == want["summary"] and want["summary"]["n_frames"] > 20
    assert eng_w.read_echo_conns(rconn, S) == want["conn"] and eng_w.read_relay_rooms(rrooms, R) == want["rooms"]
    sr = sres.cpu().numpy()[:S * 48].view(TS.TLS_SEND_RESULT_DT)
    assert (sr["status"] == 0).all()
    host_sealed = sealed.cpu().numpy()
    open_st = np.zeros(S, O.TLS_STREAM_DT)
    for c in range(S):
        open_st[c] = (int(sr[c]["out_off"]), int(sr[c]["out_len"]), seq_s[c], S + c, 0)
    total = int(ssum.cpu().numpy().view(TS.TLS_SEND_SUMMARY_DT)[0]["out_bytes"])
    o_recs, o_res, o_out = O.tls_open_batch(host_sealed[:max(1, total)], keys, open_st, out_cap=total + 16)
    for c in range(S):
        r = o_res[c]
        got = b"".join(o_out[rec["out_off"]:rec["out_off"] + rec["content_len"]].tobytes()
                       for rec in o_recs[r["first_record"]:r["first_record"] + r["n_delivered"]])
        assert got == b"".join(lists[room[c]]), c
    eng_w.close()
    eng_t.close()


# ---- a captured graph -----------------------------------------------------------------------------

def test_graph_replay(torch, eng):
    """decode_streams + relay_messages_streams captured on a side stream after one uncaptured call
    of the shape, replayed over two wires of the same layout: the rooms follow the bytes"""
    rng = random.Random(9)

    def conns_of(second_fin):
        return [[ER.text(rng.randbytes(20)), ER.binary(rng.randbytes(300), 0), ER.cont(rng.randbytes(9), second_fin),
                 ER.ping(b"12345")] for _ in range(8)]
    a, b = conns_of(1), conns_of(0)
    (w0, st, _), (w1, st1, _) = _streams([ER.raw(c) for c in a]), _streams([ER.raw(c) for c in b])
    assert w0.size == w1.size and (st == st1).all()
    S, R, mf, cap = 8, 300, 40, 4096
    room = [299, 0, 257, 0, 1, 299, 256, 0]
    recv = [0, 299, 5, 300]
    dw, dst = _dev(torch, w0), _dev(torch, st, 0)
    d_room, d_recv = _dev(torch, np.array(room, np.uint32), 0), _dev(torch, np.array(recv, np.uint32), 0)
    desc = torch.zeros(mf * 32, dtype=torch.uint8, device="cuda")
    res = torch.zeros(S * 64, dtype=torch.uint8, device="cuda")
    o = Out(torch, S, R, len(recv), mf, cap, cap)

    def both(stream=None):
        eng.decode_streams(dw, dst, S, mf, desc=desc, results=res, wire_len=w0.size, stream=stream)
        eng.relay_messages_streams(dw, desc, mf, dst, res, S, d_room, R, mf, cap, recv_room=d_recv, n_receivers=len(recv),
                                   wire_len=w0.size, stream=stream, **o.kw())

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
        assert got == RR.expected([ER.raw(c) for c in conns], room, R, recv, max_frames_out=mf)
        assert got["summary"]["n_frames"] == (16 if conns is a else 8)
        assert got["sends"][0] == (0, 6 if conns is a else 3) and got["summary"]["n_bad_receivers"] == 1


# ---- every chunked pass in several pieces ---------------------------------------------------------

@pytest.mark.parametrize("n", [1, 3])
def test_grid_pieces(torch, monkeypatch, n):
    """the ordering passes, the room and receiver passes and the emit going out in launches of n
    workgroups (UVHTTP_WS_GRID_PIECE, the experiment build), against the references and, byte for
    byte, against an unsplit engine"""
    split = _engine(monkeypatch, {"UVHTTP_WS_GRID_PIECE": n})
    whole = _engine(monkeypatch, {})
    try:
        m = RR.mixed_case()
        split.grid_pieces()
        run_relay(torch, split, gap=3, ref_eng=whole, **m)
        passes, pieces, tiles = split.grid_pieces()
        assert tiles >= 5 and pieces >= -(-tiles // n) and pieces > passes
        S = 4 * SCAN_BLOCK + 5  # five workgroups in every connection pass, two radix passes, 1300 rooms
        conns = [[ER.text(b"%d" % s)] * (s % 3) for s in range(S)]
        split.grid_pieces()
        got, _ = run_relay(torch, split, conns, [(s * 577) % 1300 for s in range(S)], 1300,
                           [(k * 31) % 1301 for k in range(700)], ref=False, ref_eng=whole)
        passes, pieces, tiles = split.grid_pieces()
        assert passes >= 13 and pieces >= passes + 10 * (-(-5 // n) - 1)
        assert got["summary"]["n_frames"] == sum(s % 3 for s in range(S))
    finally:
        whole.close()
        split.close()


# ---- a seeded fuzz --------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", range(4))
def test_fuzz_small_batches(torch, eng, seed):
    """50 batches per seed of at most 64 connections and 2 000 frames: random messages cut into
    fragments with PINGs between, a CLOSE or a failing frame part-way, carried-in messages, enable
    bits, random rooms (some out of range) and receivers, both flags, sometimes a capacity too
    small: device == host twin"""
    rng = random.Random(7300 + seed)
    seen = 0
    for _ in range(50):
        conns, srv, pending = [], [], []
        budget = 2000
        for _ in range(rng.randint(1, 64)):
            rows = [(rng.choice([1, 2]), rng.randbytes(rng.choice([0, 1, 5, 15, 16, 17, 125, 126, 300, 2000])))
                    for _ in range(rng.randint(0, 5))]
            fr = ER.FR.fragment_randomly(rng, rows)
            pend = None
            if rng.random() < 0.3:
                pend = (rng.choice([1, 2]), rng.randbytes(rng.choice([1, 3, 16, 200])))
                pre = [ER.cont(rng.randbytes(rng.choice([0, 2, 40])), 0) for _ in range(rng.randint(0, 2))]
                fr = pre + [ER.cont(rng.randbytes(rng.choice([0, 7])))] + fr if rng.random() < 0.7 else pre
            if rng.random() < 0.2 and fr:
                fr.insert(rng.randrange(len(fr) + 1), ER.close(b"\x03\xe8"))
            if rng.random() < 0.15 and fr:
                fr.insert(rng.randrange(len(fr) + 1), ER.Fr(2, 1, b"bad", rsv=True))
            if rng.random() < 0.3:
                fr = fr[:max(0, len(fr) - 1)]
            fr = fr[:budget]
            budget -= len(fr)
            conns.append(ER.raw(fr))
            srv.append(rng.choice([1, 1, 0]))
            pending.append(pend)
        n_rooms = rng.choice([0, 1, 2, 5, 64, 255, 256, 257, 70000])
        room = [rng.randrange(n_rooms + 1) if rng.random() < 0.95 else rng.getrandbits(32) for _ in conns]
        recv = [rng.randrange(n_rooms + 2) for _ in range(rng.randint(0, 80))]
        enable = [rng.choice([1, 1, 1, 0]) for _ in conns] if rng.random() < 0.5 else None
        kw = {}
        if rng.random() < 0.2:
            kw = dict(max_out=rng.randint(0, 40), out_cap=rng.randint(0, 20000), open_cap=rng.randint(0, 300))
        got, _ = run_relay(torch, eng, conns, room, n_rooms, recv, srv, enable, rng.choice([0, RR.SERVER_SEND]),
                           pending=pending, gap=rng.choice([0, 1, 5]), ref=False, with_open=rng.random() < 0.9, **kw)
        seen += got["summary"]["n_frames"]
    assert seen > 1000


# ---- capacity -------------------------------------------------------------------------------------

def test_capacity_one_short(torch, eng):
    m = RR.mixed_case()
    full, _ = run_relay(torch, eng, **m)
    n, nbytes, nopen = (full["summary"][k] for k in ("n_frames", "out_bytes", "open_bytes"))
    assert nopen > 0
    for kw in (dict(max_out=n - 1, out_cap=nbytes, open_cap=nopen), dict(max_out=n, out_cap=nbytes - 1, open_cap=nopen),
               dict(max_out=n, out_cap=nbytes, open_cap=nopen - 1)):
        got, _ = run_relay(torch, eng, ref=False, **m, **kw)
        assert got["summary"] == dict(full["summary"], status=RR.ERR_CAPACITY)
        assert got["out"] == b"" and got["open"] == b"" and set(got["out_off"]) == {0} and set(got["open_off"]) == {0}
        assert {c["status"] for c in got["conn"]} == {RR.ERR_CAPACITY} and set(got["sends"]) == {(0, 0)}
        assert all(r == RR.ZERO_ROOM for r in got["rooms"])
    got, _ = run_relay(torch, eng, ref=False, max_out=n, out_cap=nbytes, open_cap=nopen, **m)
    assert got["out"] == full["out"] and got["open"] == full["open"] and got["conn"] == full["conn"]
    got, _ = run_relay(torch, eng, ref=False, max_out=n, out_cap=nbytes, open_cap=0, with_open=False, **m)
    assert got["out"] == full["out"] and got["open_off"] == full["open_off"] and got["rooms"] == full["rooms"]


# ---- arguments ------------------------------------------------------------------------------------

def test_arguments(torch, eng):
    import uvhttp_amd as U
    wire, st, _ = _streams([ER.raw([ER.text(b"ok")])])
    dw, dst = _dev(torch, wire), _dev(torch, st, 0)
    desc, res = eng.decode_streams(dw, dst, 1, 4, wire_len=wire.size)
    o = Out(torch, 1, 1, 1, 4, 64, 64)
    d_room = torch.zeros(4, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()

    class Null:
        def data_ptr(self):
            return None

    base = dict(wire=dw, desc=desc, streams_dev=dst, results=res, room=d_room, recv_room=d_room, carry=None,
                carry_off=None, **o.kw())
    del base["open_cap"]

    def call(max_frames=4, max_out=4, send_stride=8, n_streams=1, n_rooms=1, n_receivers=1, **kw):
        a = dict(base, **kw)
        eng.relay_messages_streams(a["wire"], a["desc"], max_frames, a["streams_dev"], a["results"], n_streams, a["room"],
                                   n_rooms, max_out, 64, carry=a["carry"], carry_off=a["carry_off"], out=a["out"],
                                   out_off=a["out_off"], rooms=a["rooms"], recv_room=a["recv_room"],
                                   n_receivers=n_receivers, sends=a["sends"], send_stride=send_stride, open=a["open"],
                                   open_cap=64, open_off=a["open_off"], conn=a["conn"], summary=a["summary"],
                                   wire_len=wire.size)

    call()
    call(recv_room=None, sends=None, n_receivers=0)
    for name in ["wire", "desc", "streams_dev", "results", "room", "out", "out_off", "rooms", "recv_room", "sends",
                 "open_off", "conn", "summary"]:
        with pytest.raises(U.GpuError, match="rc=-1"):
            call(**{name: Null()})
        view = base[name].view(torch.uint8) if name in ("out_off", "open_off", "room", "recv_room", "sends") else base[name]
        with pytest.raises(U.GpuError, match="rc=-1"):
            call(**{name: view[1:]})
    for bad in (dict(send_stride=4), dict(send_stride=10), dict(open=o.obuf[1:]), dict(max_out=(1 << 28) + 1),
                dict(carry=dw[1:]), dict(carry_off=o.ooff.view(torch.uint8)[1:]), dict(max_frames=(1 << 28) + 1),
                dict(n_streams=(1 << 31) + 1), dict(n_rooms=(1 << 28) + 1), dict(recv_room=None), dict(sends=None)):
        with pytest.raises(U.GpuError, match="rc=-1"):
            call(**bad)
    torch.cuda.synchronize()
    assert o.read(eng)["out"] == b"\x81\x02ok"
