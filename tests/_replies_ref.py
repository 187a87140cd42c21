"""Reference replies for the control-reply tests (test_control_replies_host.py,
test_gpu_control_replies.py): uvhttp_ws_control_replies and uvhttp_ws_gpu_control_replies_streams /
_inplace against what the existing host path hands the control sink.

A connection's bytes go through the product's uvhttp_ws_process_data with the recording control
hooks of tests/_deliver.py; every sink call (opcode, payload) becomes the oracle's
build_frame(payload, opcode, mask = !is_server, fin = 1), and the expected output is those frames
back to back.  Without REPLY_AFTER_CLOSE the connection's on_close drops user_data, as the
reference server's frees the wrapper (so nothing after the first CLOSE is answered); with it,
on_close leaves user_data alone.  Frames are built with _oracle.build_frame; which frames are
delivered, and their descriptors, come from _oracle.decode_streams (_utf8_frames_ref)."""
import numpy as np

import _deliver as D
import _oracle as O
import _utf8_frames_ref as FR

AFTER_CLOSE = 0x1
OK, ERR_CAPACITY, BAD_RANGE, NO_KEYS = range(4)
MF, MM = FR.MF, FR.MM
Fr = FR.Fr


def ping(payload=b"", key=b"\x11\x22\x33\x44"):
    return Fr(9, 1, payload, key)


def pong(payload=b""):
    return Fr(10, 1, payload)


def close(payload=b""):
    return Fr(8, 1, payload)


def data(payload=b"data", op=2, fin=1):
    return Fr(op, fin, payload)


def key_bytes(k):
    """a reply slot's 32-bit key as the four key bytes on the wire (k0 = the low byte)"""
    return int(k).to_bytes(4, "little")


def sink_calls(reads, is_server=1, enable=1, flags=0):
    """the control sink's calls [(opcode, payload)] and whether on_close fired, for one fresh
    connection fed `reads` (one process_data call each, until one fails)"""
    import uvhttp_amd as U
    conn = U.WsConnection(is_server, MF, MM, user_data=bool(enable))
    closed = []

    def on_close(c, code, reason):
        closed.append(code)
        if not (flags & AFTER_CLOSE):
            conn.ptr.contents.user_data = None  # the reference server's on_close frees the wrapper
        return 0

    cbs = (U.ON_MESSAGE(lambda *a: 0), U.ON_CLOSE(on_close), U.ON_ERROR(lambda *a: 0))
    U.lib().uvhttp_ws_set_callbacks(conn.ptr, *cbs)
    with D.control_sink() as sink:
        for r in reads:
            if conn.process_data(bytes(r)) != 0:
                break
        calls = [(0xA if k == "pong" else 0x8, p) for k, p in sink]
    return calls, bool(closed)


def reply_frames(calls, is_server, keys):
    """the oracle's build_frame of every sink call; reply j takes keys[j]"""
    out = []
    for j, (op, payload) in enumerate(calls):
        rc, b = O.build_frame(payload, op, 0 if is_server else 1, 1,
                              b"\0\0\0\0" if is_server else key_bytes(keys[j]))
        assert rc > 0
        out.append(b)
    return out


def streams_of(conns, is_server=None, **kw):
    """FR.streams_of with a per-connection is_server"""
    wire, st = FR.streams_of(conns, **kw)
    if is_server is not None:
        st["is_server"] = is_server
    return wire, st


def expected_batch(conns, is_server=None, enable=None, keys=None, flags=0, reads=None, silent=(),
                   max_replies=None):
    """the whole batch's expected outputs from the sink reference: connection s = conns[s]
    ([Fr], or raw bytes), fed as reads[s] (list of byte strings) when given.  `silent` = {s:
    status} connections that get no replies for a reason the sink path does not know (BAD_RANGE,
    a failed decode result: status OK).  -> dict(out, out_off, conn, summary); out_off has
    max_replies + 1 entries when max_replies is given, else n_replies + 1"""
    out, off, res = bytearray(), [], []
    n_closed = 0
    for s, frames in enumerate(conns):
        srv = 1 if is_server is None else int(is_server[s])
        en = 1 if enable is None else int(enable[s])
        raw = frames if isinstance(frames, (bytes, bytearray)) else b"".join(f.bytes for f in frames)
        rd = reads[s] if reads is not None and reads[s] is not None else [raw]
        status = OK
        if s in silent:
            calls, closed = [], sink_calls(rd, srv, 0, flags)[1] if silent[s] == BAD_RANGE else False
            status = silent[s]
        elif en and not srv and keys is None:
            calls, closed = [], sink_calls(rd, srv, 0, flags)[1]
            status = NO_KEYS
        else:
            calls, closed = sink_calls(rd, srv, en, flags)
        fr = reply_frames(calls, srv, None if keys is None else keys[len(off):])
        res.append({"first_reply": len(off), "n_replies": len(fr), "out_len": sum(map(len, fr)),
                    "status": status, "closed": int(closed)})
        n_closed += int(closed)
        for b in fr:
            off.append(len(out))
            out += b
    n = len(off)
    off += [len(out)] * ((n if max_replies is None else max_replies) + 1 - n)
    return {"out": bytes(out), "out_off": off, "conn": res,
            "summary": {"out_bytes": len(out), "n_replies": n, "n_closed_conns": n_closed, "status": OK}}


def capacity_failure(exp, max_replies):
    """what a call whose max_replies or out_cap is too small for `exp` must give"""
    return {"out": b"", "out_off": [0] * (max_replies + 1),
            "conn": [{"first_reply": 0, "n_replies": 0, "out_len": 0, "status": ERR_CAPACITY,
                      "closed": c["closed"]} for c in exp["conn"]],
            "summary": dict(exp["summary"], status=ERR_CAPACITY)}


def host_batch(U, wire, desc, first, nd, is_server=None, enable=None, keys=None, flags=0,
               max_replies=None, wire_len=None):
    """the host twin over every connection of a decoded batch, put together as the device lays
    the batch out -> the same dict as expected_batch"""
    out, off, res = bytearray(), [], []
    for s in range(len(first)):
        srv = 1 if is_server is None else int(is_server[s])
        en = 1 if enable is None else int(enable[s])
        k = None if keys is None else [int(x) for x in keys[len(off):len(off) + nd[s]]] + [0] * nd[s]
        b, o, r = U.control_replies(wire, desc, first[s], nd[s], srv, en, k, flags, wire_len=wire_len)
        assert r["status"] != ERR_CAPACITY and len(b) == r["out_len"]
        assert o[:r["n_replies"] + 1] == o[:r["n_replies"]] + [len(b)] and r["first_reply"] == 0
        r["first_reply"] = len(off)
        off += [len(out) + x for x in o[:r["n_replies"]]]
        out += b
        res.append(r)
    n = len(off)
    off += [len(out)] * ((n if max_replies is None else max_replies) + 1 - n)
    return {"out": bytes(out), "out_off": off, "conn": res,
            "summary": {"out_bytes": len(out), "n_replies": n,
                        "n_closed_conns": sum(r["closed"] for r in res), "status": OK}}


def keys_for(rng, n):
    return np.array([rng.getrandbits(32) for _ in range(max(1, n))], dtype=np.uint32)
