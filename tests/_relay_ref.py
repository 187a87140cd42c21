"""Reference relays for the relay tests (test_relay_host.py, test_gpu_relay.py):
uvhttp_ws_relay_messages and uvhttp_ws_gpu_relay_messages_streams against what the product's
uvhttp_ws_process_data hands a recording on_message, as tests/_echo_ref.py does for the echo.

A sender's bytes go through process_data; every on_message call made while the sender is OPEN
becomes the oracle's build_frame(payload, opcode, mask = 0, fin = 1) — under SERVER_SEND opcode
TEXT and nothing for an empty message, uvhttp_server_ws_broadcast's rules — and is appended to
its room's list.  A room's bytes are its list, senders in index order; a receiver's expected
frames are its room's list."""
import numpy as np

import _echo_ref as ER

SERVER_SEND = ER.SERVER_SEND
OK, ERR_CAPACITY, BAD_RANGE, NO_KEYS, NO_CARRY, BAD_ROOM = range(6)
ZERO = ER.ZERO
ZERO_ROOM = {"first_frame": 0, "n_frames": 0, "out_off": 0, "out_len": 0}
RESULT_DT = np.dtype([("first_frame", "<u4"), ("n_frames", "<u4"), ("n_delivered", "<u4"), ("status", "<i4"),
                      ("first_status", "<i4"), ("calls", "<u4"), ("consumed_bytes", "<u8"),
                      ("recv_buffer_size", "<u8"), ("pending_bytes", "<u8"), ("buffered_end", "<u8"),
                      ("reserved", "<u8")])
assert RESULT_DT.itemsize == 64


def results_of(first, nd, first_status=None):
    """a uvhttp_ws_stream_result_t table that names desc[first[s], first[s] + nd[s]) per connection"""
    res = np.zeros(max(1, len(first)), RESULT_DT)
    for s in range(len(first)):
        res[s]["first_frame"], res[s]["n_frames"], res[s]["n_delivered"] = first[s], nd[s], nd[s]
        if first_status is not None:
            res[s]["first_status"] = first_status[s]
    return res


def sender_rows(conns, room, n_rooms, is_server=None, enable=None, flags=0, reads=None, pending=None, silent=()):
    """[(frames, open bytes, status, open_opcode)] per sender from the on_message reference.
    `silent` = {s: status}: senders that get nothing for a reason process_data does not know
    (NO_CARRY, BAD_RANGE), or whose decode result failed (OK: the carry passes through)"""
    rows = []
    for s, frames in enumerate(conns):
        srv = 1 if is_server is None else int(is_server[s])
        en = 1 if enable is None else int(enable[s])
        pend = pending[s] if pending is not None else None
        rd = reads[s] if reads is not None and reads[s] is not None else [ER.raw(frames)]
        if not en:
            rows.append(([], b"", OK, 0))
        elif s in silent:
            status = silent[s] if silent[s] == NO_CARRY or room[s] < n_rooms else BAD_ROOM  # the precedence
            through = status == OK and pend and pend[1]
            rows.append(([], pend[1] if through else b"", status, pend[0] if through else 0))
        elif room[s] >= n_rooms:
            rows.append(([], b"", BAD_ROOM, 0))
        else:
            calls, still = ER.on_messages(rd, srv, pend)
            rows.append((ER.echo_frames(calls, 1, None, flags), still[1], OK, still[0]))
    return rows


def layout(rows, room, n_rooms, recv_room=(), max_frames_out=None):
    """the call's outputs from the senders' rows: every room's list in room order"""
    S = len(rows)
    out, off, conn, rooms = bytearray(), [], [None] * S, []

    def place(s):
        fr, ob, status, oop = rows[s]
        conn[s] = {"first_echo": len(off), "n_echoes": len(fr), "out_len": sum(map(len, fr)), "open_len": len(ob),
                   "status": status, "open_opcode": oop if ob else 0}
        for b in fr:
            off.append(len(out))
            out.extend(b)

    for r in range(n_rooms):
        first, at = len(off), len(out)
        for s in range(S):
            if room[s] == r:
                place(s)
        rooms.append({"first_frame": first, "n_frames": len(off) - first, "out_off": at, "out_len": len(out) - at})
    for s in range(S):
        if room[s] >= n_rooms:
            place(s)
    opn, ooff = bytearray(), []
    for s in range(S):
        ooff.append(len(opn))
        opn += rows[s][1]
    n = len(off)
    off += [len(out)] * ((n if max_frames_out is None else max_frames_out) + 1 - n)
    sends = [(rooms[r]["first_frame"], rooms[r]["n_frames"]) if r < n_rooms else (0, 0) for r in recv_room]
    bad_rooms = sum(1 for s in range(S) if rows[s][2] == BAD_ROOM)
    return {"out": bytes(out), "out_off": off, "open": bytes(opn), "open_off": ooff + [len(opn)], "conn": conn,
            "rooms": rooms, "sends": sends,
            "summary": {"out_bytes": len(out), "open_bytes": len(opn), "n_frames": n, "status": OK,
                        "n_bad_rooms": bad_rooms, "n_bad_receivers": sum(1 for r in recv_room if r >= n_rooms)}}


def expected(conns, room, n_rooms, recv_room=(), is_server=None, enable=None, flags=0, reads=None, pending=None,
             silent=(), max_frames_out=None):
    rows = sender_rows(conns, room, n_rooms, is_server, enable, flags, reads, pending, silent)
    return layout(rows, room, n_rooms, recv_room, max_frames_out)


def room_lists(exp):
    """[[frame bytes]] per room of an expected (or produced) batch"""
    out, off = exp["out"], exp["out_off"]
    return [[out[off[j]:off[j + 1]] for j in range(r["first_frame"], r["first_frame"] + r["n_frames"])]
            for r in exp["rooms"]]


def capacity_failure(exp, max_frames_out):
    """what a call whose max_frames_out, out_cap or open_cap is too small for `exp` must give"""
    return {"out": b"", "out_off": [0] * (max_frames_out + 1), "open": b"", "open_off": [0] * len(exp["open_off"]),
            "conn": [dict(ZERO, status=ERR_CAPACITY) for _ in exp["conn"]],
            "rooms": [dict(ZERO_ROOM) for _ in exp["rooms"]], "sends": [(0, 0) for _ in exp["sends"]],
            "summary": dict(exp["summary"], status=ERR_CAPACITY)}


def want(host, max_frames_out, out_cap, open_cap, with_open=True):
    s = host["summary"]
    if s["n_frames"] > max_frames_out or s["out_bytes"] > out_cap or (with_open and s["open_bytes"] > open_cap):
        return capacity_failure(host, max_frames_out)
    return host if with_open else dict(host, open=b"")


def host_batch(U, wire, desc, max_frames, st, res, room, n_rooms, recv_room=(), enable=None, flags=0, pending=None,
               carries=None, **kw):
    """the host twin over host copies of a decoded batch -> the same dict as expected()"""
    S = len(room)
    carry = off = None
    if pending is not None or carries is not None:
        carry, off = ER.carry_tables(pending if carries is None else [(0, c) for c in carries], S)
    return U.relay_messages(wire, desc, max_frames, st, res, room, n_rooms, enable, flags, carry, off, recv_room, **kw)


def payload(n, salt=0):
    return bytes((salt + 31 * i + (i >> 8)) & 0xFF for i in range(n))


def mixed_case():
    """sixteen senders in six rooms: rooms of 0, 1, 2 and 5 senders, interleaved; the message
    lengths at the header steps, fragmented and carried-in messages, a message completing after
    its sender's CLOSE, a failing frame, a disabled sender, a sender in no room, a client; and
    receivers in every room, in the empty one and in none"""
    P = ER.ping(b"\xff\xfe")
    T, B, K = ER.text, ER.binary, ER.cont
    conns = [
        [T(b""), B(b"a"), T(payload(125)), B(payload(126, 1))],
        [],
        [T(b"ab", 0), K(b"cd")],
        [B(b"abc", 0), K(b"", 0), K(b"defg")],
        [T(b"x" * 100, 0), P, K(b"y" * 30, 0), P, P, K(b"")],
        [T(b"", 0), T(b"fresh")],
        [T(b"before"), T(b"open", 0), ER.close(b"\x03\xe8"), K(b"ed"), T(b"after")],
        [T(b"ok"), B(b"part", 0), ER.Fr(0, 1, b"bad", rsv=True), T(b"never")],
        [T(b"quiet"), T(b"op", 0)],
        [T(b"nowhere"), B(b"lost", 0)],
        [T(b"abcde"), P, B(b"fr", 0), K(b"agment")],
        [T(payload(300, 3))],
        [K(b" world"), T(b"next", 0)],
        [K(b"more", 0), P],
        [],
        [B(payload(65535, 4)), T(payload(65536, 5))],
    ]
    S = len(conns)
    srv = [1] * S
    srv[10] = srv[11] = 0
    en = [1] * S
    en[8] = 0
    pending = [None] * S
    pending[12], pending[13], pending[14] = (1, b"hello"), (2, payload(200, 7)), (1, b"idle")
    #       0  1  2  3  4  5  6  7  8  9 10 11 12 13 14 15
    room = [4, 4, 0, 1, 4, 0, 2, 4, 4, 9, 0, 5, 0, 4, 0, 1]
    n_rooms = 6  # room 3 is empty, 2 and 5 have one sender, 1 has two, 0 five, 4 the rest
    recv_room = [0, 1, 2, 3, 4, 5, 6, 0, 0xFFFFFFFF, 3, 4, 1]
    return dict(conns=conns, is_server=srv, enable=en, pending=pending, room=room, n_rooms=n_rooms,
                recv_room=recv_room)
