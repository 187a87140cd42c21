"""Reference answers for the answer tests (test_answer_host.py, test_gpu_answer.py,
test_gpu_answer_chain.py): uvhttp_ws_answer_messages and uvhttp_ws_gpu_answer_messages_streams /
_inplace against the transcript of one connection.

A connection's reads go through the product's uvhttp_ws_process_data with BOTH recorders active:
the on_message hook of _echo_ref.on_messages (a call counts while state == OPEN) and the control
sink of _deliver.control_sink (PONGs and CLOSE echoes).  Both append to ONE list, so the list is
in call order: the order the reference sends in.  Every entry becomes the oracle's
build_frame(payload, opcode, mask = !is_server, fin = 1) with key keys[j] for list position j.
on_close drops user_data unless REPLY_AFTER_CLOSE is set, as the reference server's frees the
wrapper.  Nothing here looks at the code under test."""
import ctypes as C

import _deliver as D
import _echo_ref as ER
import _oracle as O

SERVER_SEND, REPLY_AFTER_CLOSE = 0x1, 0x2
OK, ERR_CAPACITY, BAD_RANGE, NO_KEYS, NO_CARRY = range(5)
REPLY_STATUS = {OK: 0, ERR_CAPACITY: 1, BAD_RANGE: 2, NO_KEYS: 3, NO_CARRY: 0}
MF, MM = ER.MF, ER.MM
Fr = ER.Fr
text, binary, cont, ping, close, raw = ER.text, ER.binary, ER.cont, ER.ping, ER.close, ER.raw
key_bytes, keys_for, streams_of, carry_tables = ER.key_bytes, ER.keys_for, ER.streams_of, ER.carry_tables
ZERO = {"first_answer": 0, "n_answers": 0, "out_len": 0, "open_len": 0, "status": OK, "open_opcode": 0,
        "closed": 0, "n_replies": 0}
RZERO = {"first_reply": 0, "n_replies": 0, "out_len": 0, "status": 0, "closed": 0}


def transcript(reads, is_server=1, flags=0, pending=None, enable=1):
    """-> ([(opcode, payload)] in call order: a data opcode for an on_message call made while
    state == OPEN, 0xA for a PONG, 0x8 for a CLOSE echo; (opcode, bytes) of the message still open
    afterwards or (0, b""); whether on_close fired) for one connection fed `reads` (one
    process_data call each, until one fails) after a first fragment `pending` = (opcode, bytes)"""
    import uvhttp_amd as U
    conn = U.WsConnection(is_server, MF, MM, callbacks=False, user_data=bool(enable))
    armed, closed = [False], []
    with D.control_sink() as sink:
        def on_message(c, data, n, opcode):
            if armed[0] and conn.struct.state == ER.STATE_OPEN:
                sink.append(("echo", opcode, C.string_at(data, n) if n else b""))
            return 0

        def on_close(c, code, reason):
            closed.append(code)
            if not (flags & REPLY_AFTER_CLOSE):
                conn.ptr.contents.user_data = None  # the reference server's on_close frees the wrapper
            return 0

        cbs = (U.ON_MESSAGE(on_message), U.ON_CLOSE(on_close), U.ON_ERROR(lambda *a: 0))
        U.lib().uvhttp_ws_set_callbacks(conn.ptr, *cbs)
        conn.ptr.contents.state = ER.STATE_OPEN  # as after the handshake
        if pending and pending[1]:
            assert conn.process_data(Fr(pending[0], 0, pending[1]).bytes) == 0
        armed[0] = True
        for r in reads:
            if conn.process_data(bytes(r)) != 0:
                break
        events = [(e[1], e[2]) if e[0] == "echo" else (0xA if e[0] == "pong" else 0x8, e[1]) for e in sink]
    s = conn.struct
    still = (0, b"")
    if s.fragmented_message and s.fragmented_size:
        still = (s.fragmented_opcode, C.string_at(s.fragmented_message, s.fragmented_size))
    conn.close()
    return events, still, bool(closed)


def answer_frames(events, is_server, keys, flags=0):
    """the oracle's build_frame of every transcript entry -> [(frame, is_reply)]; list position j
    takes keys[j]"""
    out = []
    for op, payload in events:
        reply = op >= 8
        if not reply and (flags & SERVER_SEND):
            if not payload:
                continue
            op = 1
        rc, b = O.build_frame(payload, op, 0 if is_server else 1, 1,
                              b"\0\0\0\0" if is_server else key_bytes(keys[len(out)]))
        assert rc > 0
        out.append((b, reply))
    return out


def _batch(rows, max_answers):
    """[(frames [(bytes, is_reply)], open bytes, status, open_opcode, closed)] per connection ->
    the batch's outputs"""
    out, off, opn, ooff, res, rep = bytearray(), [], bytearray(), [], [], []
    for fr, ob, status, oop, closed in rows:
        nr = sum(1 for _, r in fr if r)
        res.append({"first_answer": len(off), "n_answers": len(fr), "out_len": sum(len(b) for b, _ in fr),
                    "open_len": len(ob), "status": status, "open_opcode": oop if ob else 0,
                    "closed": int(closed), "n_replies": nr})
        rep.append({"first_reply": 0, "n_replies": nr, "out_len": sum(len(b) for b, r in fr if r),
                    "status": REPLY_STATUS[status], "closed": int(closed)})
        for b, _ in fr:
            off.append(len(out))
            out += b
        ooff.append(len(opn))
        opn += ob
    n = len(off)
    off += [len(out)] * ((n if max_answers is None else max_answers) + 1 - n)
    return {"out": bytes(out), "out_off": off, "open": bytes(opn), "open_off": ooff + [len(opn)], "conn": res,
            "reply": rep,
            "summary": {"out_bytes": len(out), "open_bytes": len(opn), "n_answers": n,
                        "n_replies": sum(r["n_replies"] for r in res),
                        "n_closed_conns": sum(r["closed"] for r in res), "status": OK}}


def expected_batch(conns, is_server=None, enable=None, keys=None, flags=0, reads=None, pending=None,
                   silent=(), max_answers=None):
    """the whole batch's expected outputs from the transcript: connection s = conns[s] ([Fr], or
    raw bytes), fed as reads[s] (list of byte strings) when given, with pending[s] = (opcode,
    bytes) carried in.  `silent` = {s: status}: connections that get nothing for a reason
    process_data does not know (BAD_RANGE, NO_CARRY), or whose decode result failed (status OK:
    the carry passes through, nothing counts as delivered)"""
    rows, n = [], 0
    for s, frames in enumerate(conns):
        srv = 1 if is_server is None else int(is_server[s])
        en = 1 if enable is None else int(enable[s])
        pend = pending[s] if pending is not None else None
        rd = reads[s] if reads is not None and reads[s] is not None else [raw(frames)]
        if s in silent and silent[s] == OK:
            through = en and pend and pend[1] and (srv or keys is not None)
            status = OK if (not en or srv or keys is not None) else NO_KEYS
            rows.append(([], pend[1] if through else b"", status, pend[0] if through else 0, False))
            continue
        events, still, closed = transcript(rd, srv, flags, pend)
        if s in silent:
            rows.append(([], b"", silent[s], 0, closed))
        elif not en:
            rows.append(([], b"", OK, 0, closed))
        elif not srv and keys is None:
            rows.append(([], b"", NO_KEYS, 0, closed))
        else:
            fr = answer_frames(events, srv, None if keys is None else keys[n:], flags)
            rows.append((fr, still[1], OK, still[0], closed))
        n += len(rows[-1][0])
    return _batch(rows, max_answers)


def capacity_failure(exp, max_answers):
    """what a call whose max_answers, out_cap or open_cap is too small for `exp` must give"""
    return {"out": b"", "out_off": [0] * (max_answers + 1), "open": b"", "open_off": [0] * len(exp["open_off"]),
            "conn": [dict(ZERO, status=ERR_CAPACITY) for _ in exp["conn"]],
            "reply": [dict(RZERO, status=1, closed=c["closed"]) for c in exp["conn"]],
            "summary": dict(exp["summary"], status=ERR_CAPACITY)}


def host_batch(U, wire, desc, first, nd, is_server=None, enable=None, keys=None, flags=0, pending=None,
               carries=None, max_answers=None, wire_len=None):
    """the host twin over every connection of a decoded batch, put together as the device lays
    the batch out -> the same dict as expected_batch.  pending[s] = (opcode, bytes) as the stream
    table says, carries[s] = the bytes handed in (None: pending's own)"""
    rows, n, reps = [], 0, []
    for s in range(len(first)):
        srv = 1 if is_server is None else int(is_server[s])
        en = 1 if enable is None else int(enable[s])
        pop, pby = pending[s] if pending is not None and pending[s] else (0, b"")
        carry = pby if carries is None else carries[s]
        k = None if keys is None else [int(x) for x in keys[n:n + nd[s]]] + [0] * (nd[s] + 1)
        b, o, opn, r, q = U.answer_messages(wire, desc, first[s], nd[s], srv, en, k, flags, pop, len(pby), carry,
                                            wire_len=wire_len)
        assert r["status"] != ERR_CAPACITY and len(b) == r["out_len"] and len(opn) == r["open_len"]
        assert o[:r["n_answers"] + 1] == o[:r["n_answers"]] + [len(b)] and r["first_answer"] == 0
        fr = [b[o[j]:o[j + 1]] for j in range(r["n_answers"])]
        fr = [(x, (x[0] & 0x0F) >= 8) for x in fr]
        rows.append((fr, opn, r["status"], r["open_opcode"], r["closed"]))
        assert r["n_replies"] == sum(1 for _, rp in fr if rp)
        reps.append(q)
        n += len(fr)
    got = _batch(rows, max_answers)
    assert got["reply"] == reps  # the twin's own reply table is the one derived from its frames
    return got
