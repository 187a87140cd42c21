"""Reference echoes for the echo tests (test_echo_host.py, test_gpu_echo.py):
uvhttp_ws_echo_messages and uvhttp_ws_gpu_echo_messages_streams / _inplace against what the
product's uvhttp_ws_process_data hands a recording on_message.

A connection's bytes go through process_data; every on_message call made while state == OPEN
becomes the oracle's build_frame(payload, opcode, mask = !is_server, fin = 1) — under
SERVER_SEND with the rules of uvhttp_server_ws_send: opcode TEXT, nothing for an empty message —
and the expected output is those frames back to back.  The message still open afterwards is what
the connection holds in fragmented_message.  A carried-in message is made by feeding the
connection a first fragment before the recording starts."""
import ctypes as C

import numpy as np

import _oracle as O
import _utf8_frames_ref as FR

SERVER_SEND = 0x1
OK, ERR_CAPACITY, BAD_RANGE, NO_KEYS, NO_CARRY = range(5)
MF, MM = FR.MF, FR.MM
Fr = FR.Fr
STATE_OPEN = 1
ZERO = {"first_echo": 0, "n_echoes": 0, "out_len": 0, "open_len": 0, "status": OK, "open_opcode": 0}


def text(payload=b"", fin=1):
    return Fr(1, fin, payload)


def binary(payload=b"", fin=1):
    return Fr(2, fin, payload)


def cont(payload=b"", fin=1):
    return Fr(0, fin, payload)


def ping(payload=b""):
    return Fr(9, 1, payload)


def close(payload=b""):
    return Fr(8, 1, payload)


def raw(c):
    return bytes(c) if isinstance(c, (bytes, bytearray)) else b"".join(f.bytes for f in c)


def key_bytes(k):
    return int(k).to_bytes(4, "little")


def keys_for(rng, n):
    return np.array([rng.getrandbits(32) for _ in range(max(1, n))], dtype=np.uint32)


def on_messages(reads, is_server=1, pending=None):
    """-> ([(opcode, payload)] of the on_message calls made while state == OPEN, (opcode, bytes)
    of the message still open afterwards or (0, b"")) for one connection fed `reads` (one
    process_data call each, until one fails), after a first fragment `pending` = (opcode, bytes)"""
    import uvhttp_amd as U
    conn = U.WsConnection(is_server, MF, MM)
    calls, armed = [], [False]

    def hook(c, ev):
        if armed[0] and c.struct.state == STATE_OPEN:
            calls.append((ev[1], ev[2]))

    conn.hook = hook
    conn.ptr.contents.state = STATE_OPEN  # as after the handshake (src/uvhttp_websocket.c:503)
    if pending and pending[1]:
        assert conn.process_data(Fr(pending[0], 0, pending[1]).bytes) == 0
    armed[0] = True
    for r in reads:
        if conn.process_data(bytes(r)) != 0:
            break
    s = conn.struct
    still = (0, b"")
    if s.fragmented_message and s.fragmented_size:
        still = (s.fragmented_opcode, C.string_at(s.fragmented_message, s.fragmented_size))
    conn.close()
    return calls, still


def echo_frames(calls, is_server, keys, flags=0):
    """the oracle's build_frame of every recorded call; echo j takes keys[j]"""
    out = []
    for op, payload in calls:
        if flags & SERVER_SEND:
            if not payload:
                continue
            op = 1
        rc, b = O.build_frame(payload, op, 0 if is_server else 1, 1,
                              b"\0\0\0\0" if is_server else key_bytes(keys[len(out)]))
        assert rc > 0
        out.append(b)
    return out


def _batch(rows, max_echoes):
    """[(frames, open bytes, status, open_opcode)] per connection -> the batch's outputs"""
    out, off, opn, ooff, res = bytearray(), [], bytearray(), [], []
    for fr, ob, status, oop in rows:
        res.append({"first_echo": len(off), "n_echoes": len(fr), "out_len": sum(map(len, fr)),
                    "open_len": len(ob), "status": status, "open_opcode": oop if ob else 0})
        for b in fr:
            off.append(len(out))
            out += b
        ooff.append(len(opn))
        opn += ob
    n = len(off)
    off += [len(out)] * ((n if max_echoes is None else max_echoes) + 1 - n)
    return {"out": bytes(out), "out_off": off, "open": bytes(opn), "open_off": ooff + [len(opn)], "conn": res,
            "summary": {"out_bytes": len(out), "open_bytes": len(opn), "n_echoes": n, "status": OK}}


def expected_batch(conns, is_server=None, enable=None, keys=None, flags=0, reads=None, pending=None,
                   silent=(), max_echoes=None):
    """the whole batch's expected outputs from the on_message reference: connection s = conns[s]
    ([Fr], or raw bytes), fed as reads[s] (list of byte strings) when given, with pending[s] =
    (opcode, bytes) carried in.  `silent` = {s: status}: connections that get nothing for a
    reason process_data does not know (BAD_RANGE, NO_CARRY), or whose decode result failed
    (status OK: the carry passes through)"""
    rows, n = [], 0
    for s, frames in enumerate(conns):
        srv = 1 if is_server is None else int(is_server[s])
        en = 1 if enable is None else int(enable[s])
        pend = pending[s] if pending is not None else None
        rd = reads[s] if reads is not None and reads[s] is not None else [raw(frames)]
        if s in silent:
            through = silent[s] == OK and en and pend and pend[1] and (srv or keys is not None)
            rows.append(([], pend[1] if through else b"", silent[s], pend[0] if through else 0))
        elif not en:
            rows.append(([], b"", OK, 0))
        elif not srv and keys is None:
            rows.append(([], b"", NO_KEYS, 0))
        else:
            calls, still = on_messages(rd, srv, pend)
            fr = echo_frames(calls, srv, None if keys is None else keys[n:], flags)
            rows.append((fr, still[1], OK, still[0]))
        n += len(rows[-1][0])
    return _batch(rows, max_echoes)


def capacity_failure(exp, max_echoes):
    """what a call whose max_echoes, out_cap or open_cap is too small for `exp` must give"""
    return {"out": b"", "out_off": [0] * (max_echoes + 1), "open": b"", "open_off": [0] * len(exp["open_off"]),
            "conn": [dict(ZERO, status=ERR_CAPACITY) for _ in exp["conn"]],
            "summary": dict(exp["summary"], status=ERR_CAPACITY)}


def host_batch(U, wire, desc, first, nd, is_server=None, enable=None, keys=None, flags=0, pending=None,
               carries=None, max_echoes=None, wire_len=None):
    """the host twin over every connection of a decoded batch, put together as the device lays
    the batch out -> the same dict as expected_batch.  pending[s] = (opcode, n bytes) as the
    stream table says, carries[s] = the bytes handed in (None: pending's own)"""
    rows, n = [], 0
    for s in range(len(first)):
        srv = 1 if is_server is None else int(is_server[s])
        en = 1 if enable is None else int(enable[s])
        pop, pby = pending[s] if pending is not None and pending[s] else (0, b"")
        carry = pby if carries is None else carries[s]
        k = None if keys is None else [int(x) for x in keys[n:n + nd[s]]] + [0] * (nd[s] + 1)
        b, o, opn, r = U.echo_messages(wire, desc, first[s], nd[s], srv, en, k, flags, pop, len(pby), carry,
                                       wire_len=wire_len)
        assert r["status"] != ERR_CAPACITY and len(b) == r["out_len"] and len(opn) == r["open_len"]
        assert o[:r["n_echoes"] + 1] == o[:r["n_echoes"]] + [len(b)] and r["first_echo"] == 0
        fr = [b[o[j]:o[j + 1]] for j in range(r["n_echoes"])]
        rows.append((fr, opn, r["status"], r["open_opcode"]))
        n += len(fr)
    return _batch(rows, max_echoes)


def streams_of(conns, is_server=None, pending=None, gap=0):
    """FR.streams_of over raw bytes or [Fr], with a per-connection is_server; pending[s] =
    (opcode, bytes) -> the table's pending_opcode / pending_bytes"""
    wire, st = bytearray(), np.zeros(len(conns), O.STREAM_DT)
    for s, c in enumerate(conns):
        b = raw(c)
        pop, pby = (pending[s] if pending else None) or (0, b"")
        st[s] = (len(wire), len(b), 65536, len(pby), pop if pby else 0, MF, MM,
                 1 if is_server is None else int(is_server[s]), 0, 0, 0)
        wire += b + b"\xff" * gap
    return np.frombuffer(bytes(wire) or b"\0", np.uint8).copy(), st


def carry_tables(pending, n):
    """the carry buffer and its n + 1 offsets of pending[s] = (opcode, bytes) or None"""
    buf, off = bytearray(), [0]
    for s in range(n):
        buf += (pending[s][1] if pending and pending[s] else b"")
        off.append(len(buf))
    return bytes(buf), off
