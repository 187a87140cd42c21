"""uvhttp_ws_relay_messages (the host twin of the device relay of data messages to the members
of their rooms) against the room lists the product's process_data makes through a recording
on_message (tests/_relay_ref.py): rooms of 0, 1, 2 and 5 senders, interleaved and descending room
maps, the message lengths at the header steps, fragmented and carried-in messages, a message
completing after its sender's CLOSE, a failing frame, enable = 0, BAD_ROOM, NO_CARRY, BAD_RANGE
and their precedence, receivers in empty and invalid rooms, SERVER_SEND, the capacity failures,
the identity room map against uvhttp_ws_echo_messages, and a seeded mix."""
import random

import numpy as np
import pytest

import _echo_ref as ER
import _relay_ref as RR

LENGTHS = [0, 1, 125, 126, 65535, 65536]


@pytest.fixture(scope="module")
def U():
    import uvhttp_amd as U
    return U


def _decode(conns, is_server=None, pending=None):
    wire, st = ER.streams_of(conns, is_server, pending)
    w, desc, first, nd, out = ER.FR.oracle_decode(wire, st)
    return w, desc, st, first, nd, out


def _check(U, conns, room, n_rooms, recv_room=(), is_server=None, enable=None, flags=0, pending=None, silent=(),
           carries=None, wire_len=None):
    """host twin == room lists of the on_message reference, in every output"""
    w, desc, st, first, nd, out = _decode(conns, is_server, pending)
    want = RR.expected(conns, room, n_rooms, recv_room, is_server, enable, flags, None, pending, silent, len(desc))
    got = RR.host_batch(U, w, desc, len(desc), st, RR.results_of(first, nd), room, n_rooms, recv_room, enable, flags,
                        pending, carries, wire_len=wire_len)
    assert got == want
    for s, c in enumerate(got["conn"]):  # the open message is the decoder's pending message
        if c["status"] == RR.OK and (enable is None or enable[s]):
            assert c["open_len"] == int(out["frag_size"][s])
    return got


def test_mixed_rooms(U):
    m = RR.mixed_case()
    got = _check(U, **m)
    assert [r["n_frames"] for r in got["rooms"]] == [5, 3, 1, 0, 6, 1]
    assert got["rooms"][3] == dict(RR.ZERO_ROOM, first_frame=9, out_off=got["rooms"][4]["out_off"])
    assert got["conn"][9] == dict(RR.ZERO, first_echo=16, status=RR.BAD_ROOM)
    assert got["conn"][8] == dict(RR.ZERO, first_echo=got["conn"][13]["first_echo"])  # disabled, in room 4
    assert got["conn"][6]["n_echoes"] == 1 and got["conn"][7]["n_echoes"] == 1  # after CLOSE; a failing frame
    assert got["sends"][3] == (9, 0) and got["sends"][6] == (0, 0) and got["sends"][8] == (0, 0)
    assert got["sends"][0] == got["sends"][7] == (0, 5)
    assert got["summary"]["n_bad_rooms"] == 1 and got["summary"]["n_bad_receivers"] == 2
    # every frame is a server frame, the clients' (10 in room 0, 11 in room 5) included
    assert all(not f[1] & 0x80 for fr in RR.room_lists(got) for f in fr)
    assert RR.room_lists(got)[5] == [b"\x81\x7e\x01\x2c" + RR.payload(300, 3)]


@pytest.mark.parametrize("n", LENGTHS)
def test_lengths_in_two_rooms(U, n):
    p = RR.payload(n, 1)
    got = _check(U, [[ER.text(b"a")], [ER.binary(p)], [ER.text(b"b")]], [1, 0, 1], 2, [1, 0])
    hdr = 2 if n <= 125 else 4 if n <= 65535 else 10
    assert got["rooms"] == [dict(first_frame=0, n_frames=1, out_off=0, out_len=hdr + n),
                            dict(first_frame=1, n_frames=2, out_off=hdr + n, out_len=6)]
    assert got["out"][hdr:hdr + n] == p and got["out"][hdr + n:] == b"\x81\x01a\x81\x01b"
    assert got["sends"] == [(1, 2), (0, 1)]


@pytest.mark.parametrize("order", ["mod3", "descending", "one", "own"])
def test_room_maps(U, order):
    S = 11
    conns = [[ER.text(b"m%d" % s), ER.binary(b"x" * s, 0), ER.cont(b"y")] if s % 4 else [ER.text(b"solo%d" % s)]
             for s in range(S)]
    room = {"mod3": [s % 3 for s in range(S)], "descending": [S - 1 - s for s in range(S)], "one": [0] * S,
            "own": list(range(S))}[order]
    n_rooms = max(room) + 1
    got = _check(U, conns, room, n_rooms, list(range(n_rooms)))
    for r, fr in enumerate(RR.room_lists(got)):  # a room's list is its senders' messages in index order
        mine = [s for s in range(S) if room[s] == r]
        assert [f[2:] for f in fr if f[2:3] in (b"m", b"s")] == [(b"m%d" if s % 4 else b"solo%d") % s for s in mine]


def test_statuses_and_their_precedence(U):
    T = ER.text
    conns = [[T(b"zero")], [ER.cont(b" world")], [ER.cont(b"x")], [T(b"three")], [T(b"four")], [T(b"last"), T(b"gone")]]
    pending = [None, (1, b"hello"), (1, b"abc"), None, None, None]
    carries = [b"", b"hell", b"abc", b"", b"", b""]
    w, desc, st, first, nd, _ = _decode(conns, None, pending)
    short = w.size - 1  # the last payload of sender 5 lies outside the wire
    for room, st5 in (([0, 7, 1, 7, 0, 1], RR.BAD_RANGE), ([0, 7, 1, 7, 0, 7], RR.BAD_ROOM)):
        got = _check(U, conns, room, 2, [0, 1, 2], None, [1, 1, 1, 1, 0, 1], 0, pending, {1: RR.NO_CARRY, 5: RR.BAD_RANGE},
                     carries, wire_len=short)
        assert [c["status"] for c in got["conn"]] == [RR.OK, RR.NO_CARRY, RR.OK, RR.BAD_ROOM, RR.OK, st5]
        assert got["out"] == b"\x81\x04zero\x81\x04abcx" and got["summary"]["n_bad_rooms"] == (1 if st5 == RR.BAD_RANGE else 2)
        assert got["summary"]["n_bad_receivers"] == 1 and got["sends"] == [(0, 1), (1, 1), (0, 0)]


def test_carry_passes_through_and_open_is_per_sender(U):
    conns = [[ER.cont(b"more", 0), ER.ping(b"x")], [], [ER.ping(b"only")], [ER.cont(b"fin"), ER.text(b"again", 0)]]
    pending = [(1, b"so far "), (2, b"idle"), (1, b"kept"), (2, b"x")]
    got = _check(U, conns, [3, 2, 1, 0], 4, [0, 3], pending=pending)
    assert got["open"] == b"so far more" + b"idle" + b"kept" + b"again" and got["open_off"] == [0, 11, 15, 19, 24]
    assert [c["open_opcode"] for c in got["conn"]] == [1, 2, 1, 1]
    assert got["out"] == b"\x82\x04xfin" and got["sends"] == [(0, 1), (1, 0)]


def test_server_send_flag(U):
    conns = [[ER.binary(b"bin"), ER.text(b""), ER.binary(b"l", 0), ER.cont(b"ate"), ER.binary(b"")], [ER.binary(b"")]]
    got = _check(U, conns, [1, 0], 2, [0, 1], flags=RR.SERVER_SEND)
    assert got["out"] == b"\x81\x03bin\x81\x04late" and got["sends"] == [(0, 0), (0, 2)]
    assert _check(U, conns, [1, 0], 2)["summary"]["n_frames"] == 5


def test_capacity_one_short_then_the_reported_sizes(U):
    m = RR.mixed_case()
    w, desc, st, first, nd, _ = _decode(m["conns"], m["is_server"], m["pending"])
    args = (U, w, desc, len(desc), st, RR.results_of(first, nd), m["room"], m["n_rooms"], m["recv_room"], m["enable"], 0,
            m["pending"])
    full = RR.host_batch(*args)
    n, nbytes, nopen = (full["summary"][k] for k in ("n_frames", "out_bytes", "open_bytes"))
    assert n == 16 and nopen > 0
    for kw in (dict(max_frames_out=n - 1, out_cap=nbytes, open_cap=nopen),
               dict(max_frames_out=n, out_cap=nbytes - 1, open_cap=nopen),
               dict(max_frames_out=n, out_cap=nbytes, open_cap=nopen - 1)):
        got = RR.host_batch(*args, **kw)
        assert got == RR.capacity_failure(full, kw["max_frames_out"])
        assert got["summary"]["out_bytes"] == nbytes and got["summary"]["n_bad_rooms"] == 1
    got = RR.host_batch(*args, max_frames_out=n, out_cap=nbytes, open_cap=nopen)
    assert got == dict(full, out_off=full["out_off"][:n + 1])
    got = RR.host_batch(*args, max_frames_out=n, out_cap=nbytes, open_cap=0, want_open=False)  # open_cap not tested
    assert got["out"] == full["out"] and got["open_off"] == full["open_off"] and got["rooms"] == full["rooms"]


def _echo_identity(U, conns, pending=None, enable=None, flags=0):
    """d_room[s] = s and server connections: d_out, d_out_off and the open outputs are the echo's"""
    w, desc, st, first, nd, _ = _decode(conns, None, pending)
    S = len(conns)
    got = RR.host_batch(U, w, desc, len(desc), st, RR.results_of(first, nd), list(range(S)), S, list(range(S)), enable,
                        flags, pending)
    echo = ER.host_batch(U, w, desc, first, nd, None, enable, None, flags, pending, None, len(desc))
    for k in ("out", "out_off", "open", "open_off", "conn"):
        assert got[k] == echo[k], k
    assert got["sends"] == [(c["first_echo"], c["n_echoes"]) for c in echo["conn"]]
    assert [r["out_len"] for r in got["rooms"]] == [c["out_len"] for c in echo["conn"]]


def test_identity_rooms_equal_the_echo(U):
    m = RR.mixed_case()
    _echo_identity(U, m["conns"], m["pending"], m["enable"])
    _echo_identity(U, m["conns"], m["pending"], None, RR.SERVER_SEND)


def test_failed_results_and_max_frames(U):
    """a result with ERR_CAPACITY considers nothing and passes its carry through; frames at or past
    max_frames are skipped"""
    conns = [[ER.cont(b"tail")], [ER.text(b"one"), ER.text(b"two")], [ER.text(b"cut")]]
    pending = [(2, b"head"), None, None]
    w, desc, st, first, nd, _ = _decode(conns, None, pending)
    carry, coff = ER.carry_tables(pending, 3)
    res = RR.results_of(first, nd, [-10, 0, 0])
    got = U.relay_messages(w, desc, 2, st, res, [0, 0, 0], 1, carry=carry, carry_off=coff, recv_room=[0])
    assert got["out"] == b"\x81\x03one" and got["open"] == b"head" and got["conn"][0]["open_opcode"] == 2
    assert got["sends"] == [(0, 1)] and got["conn"][2] == dict(RR.ZERO, first_echo=1)


def test_arguments(U):
    import ctypes as C
    L = U.lib()
    off, ooff = (C.c_uint64 * 2)(), (C.c_uint64 * 2)()
    st, res = np.zeros(1, ER.O.STREAM_DT), RR.results_of([0], [0])
    room, rooms, sends = (C.c_uint32 * 1)(0), (U.RelayRoom * 1)(), (C.c_uint32 * 2)()
    conn, summ = (U.EchoConn * 1)(), U.RelaySummary()
    a = [None, 0, None, 0, st.ctypes.data, res.ctypes.data, 1, None, room, 1, 0, None, 0, None, None, 0, off, 1, rooms,
         room, 1, sends, 8, None, 0, ooff, conn, C.byref(summ)]
    assert L.uvhttp_ws_relay_messages(*a) == 0 and summ.n_frames == 0 and list(sends) == [0, 0]
    for k, v in ((4, None), (5, None), (8, None), (16, None), (18, None), (19, None), (21, None), (22, 4), (22, 10),
                 (25, None), (26, None), (27, None), (1, 9), (3, 1), (15, 9)):
        b = list(a)
        b[k] = v
        assert L.uvhttp_ws_relay_messages(*b) == -1, k
    b = list(a)
    b[19], b[20], b[21] = None, 0, None  # no receivers: no tables
    assert L.uvhttp_ws_relay_messages(*b) == 0


@pytest.mark.parametrize("seed", range(40))
def test_seeded_mix(U, seed):
    """random senders in random rooms: messages cut into 1-5 fragments with PINGs between,
    sometimes a CLOSE or a failing frame part-way, a carried-in message, servers and clients,
    enable bits, rooms out of range, both flags, random receivers"""
    rng = random.Random(9300 + seed)
    conns, srv, pending = [], [], []
    for _ in range(rng.randint(1, 12)):
        rows = [(rng.choice([1, 2]), rng.randbytes(rng.choice([0, 1, 5, 125, 126, 300, 2000])))
                for _ in range(rng.randint(0, 6))]
        fr = ER.FR.fragment_randomly(rng, rows)
        pend = None
        if rng.random() < 0.4:
            pend = (rng.choice([1, 2]), rng.randbytes(rng.choice([1, 3, 16, 200])))
            pre = [ER.cont(rng.randbytes(rng.choice([0, 2, 40])), 0) for _ in range(rng.randint(0, 2))]
            fr = pre + [ER.cont(rng.randbytes(rng.choice([0, 7])))] + fr if rng.random() < 0.7 else pre
        if rng.random() < 0.3 and fr:
            fr.insert(rng.randrange(len(fr) + 1), ER.close(b"\x03\xe8"))
        if rng.random() < 0.2 and fr:
            fr.insert(rng.randrange(len(fr) + 1), ER.Fr(2, 1, b"bad", rsv=True))
        if rng.random() < 0.3:
            fr = fr[:max(0, len(fr) - 1)]  # may leave a message open
        conns.append(fr)
        srv.append(rng.choice([1, 1, 0]))
        pending.append(pend)
    n_rooms = rng.choice([0, 1, 2, 3, 7])
    room = [rng.randrange(n_rooms + 1) if rng.random() < 0.9 else 0xFFFFFFFF for _ in conns]
    recv = [rng.randrange(n_rooms + 2) for _ in range(rng.randint(0, 9))]
    enable = [rng.choice([1, 1, 1, 0]) for _ in conns] if rng.random() < 0.5 else None
    _check(U, conns, room, n_rooms, recv, srv, enable, rng.choice([0, RR.SERVER_SEND]), pending)
