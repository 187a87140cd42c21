"""Reference of the server's own CLOSE frames (uvhttp_ws_close_frames,
uvhttp_ws_gpu_close_frames_streams; include/uvhttp_ws_amd.h): a Python restatement of the rule,
its frames built by the oracle's build_frame(code || reason, opcode 8, mask = !is_server, fin 1),
which is what uvhttp_ws_close(NULL, conn, 1002, "protocol error") hands to the reference's
uvhttp_ws_build_frame.  Also the numpy layouts of the tables the pass reads and writes, and the
shared case list of the host and GPU tests."""
import random

import numpy as np

import _oracle as O
from _relay_ref import RESULT_DT

STREAM_DT = O.STREAM_DT
VERDICT_DT = np.dtype([("first_invalid", "<u4"), ("n_text_frames", "<u4"), ("pend", "u1", 3), ("n", "u1"),
                       ("status", "u1"), ("reserved", "u1", 3)])
REPLY_CONN_DT = np.dtype([("first_reply", "<u4"), ("n_replies", "<u4"), ("out_len", "<u4"), ("status", "u1"),
                          ("closed", "u1"), ("reserved", "u1", 2)])
CLOSE_CONN_DT = np.dtype([("code", "<u4"), ("out_len", "<u4"), ("status", "u1"), ("reserved", "u1", 7)])
CLOSE_SUMMARY_DT = np.dtype([("out_bytes", "<u8"), ("n_closes", "<u4"), ("n_1002", "<u4"), ("n_1007", "<u4"),
                             ("status", "<i4"), ("reserved", "<u4", 2)])
assert VERDICT_DT.itemsize == 16 and REPLY_CONN_DT.itemsize == 16
assert CLOSE_CONN_DT.itemsize == 16 and CLOSE_SUMMARY_DT.itemsize == 32

OK, ERR_CAPACITY, NO_KEYS = 0, 1, 3
UTF8_VALID, UTF8_INVALID, UTF8_NOT_TEXT, UTF8_PREFIX, UTF8_BAD_RANGE = range(5)
ERR_LAYOUT, ERR_CAPACITY_FRAME, ERR_DEVICE = -9, -10, -11
# every UVHTTP_WS_FRAME_* a result's first_status can hold, and what it gives on its own
FRAME_STATUS_CODE = {0: 0, 1: 0, 2: 0, -1: 1002, -2: 1002, -3: 1002, -4: 1002, -5: 1002, -6: 1002, -7: 1002,
                     -8: 1002, ERR_LAYOUT: 0, ERR_CAPACITY_FRAME: 0, ERR_DEVICE: 0}
REASON_1002 = b"protocol error"


def close_frame(code, is_server, key=0):
    payload = code.to_bytes(2, "big") + (REASON_1002 if code == 1002 else b"")
    rc, b = O.build_frame(payload, 8, 0 if is_server else 1, 1, int(key).to_bytes(4, "little"))
    assert rc == len(b)
    return b


def tables(n):
    """zeroed (streams, results, verdict, reply_conn, enable, keys) for n server connections"""
    st = np.zeros(max(1, n), STREAM_DT)
    st["is_server"] = 1
    return (st, np.zeros(max(1, n), RESULT_DT), np.zeros(max(1, n), VERDICT_DT),
            np.zeros(max(1, n), REPLY_CONN_DT), np.ones(max(1, n), np.uint8), np.zeros(max(1, n), np.uint32))


def close_frames_ref(streams, results, n, verdict=None, reply_conn=None, enable=None, keys=None,
                     out_cap=None, clear_runs=()):
    """-> dict(out=bytes, out_off=[n + 1], runs=[(first, n)], conn=[dict], summary=dict); the
    arrays of clear_runs (uint32 [n, >= 2]) are changed in place as the pass changes them"""
    frames, conn, codes = [], [], []
    for s in range(n):
        code, status = 0, OK
        fs = int(results[s]["first_status"])
        if (enable is None or enable[s]) and fs not in (ERR_LAYOUT, ERR_CAPACITY_FRAME, ERR_DEVICE) and \
                not (reply_conn is not None and reply_conn[s]["closed"]):
            if verdict is not None and verdict[s]["status"] == UTF8_INVALID:
                code = 1007
            elif fs < 0:
                code = 1002
            if code and not streams[s]["is_server"] and keys is None:
                code, status = 0, NO_KEYS
        codes.append(code)
        frames.append(close_frame(code, int(streams[s]["is_server"]),
                                  0 if keys is None else keys[s]) if code else b"")
        conn.append({"code": code, "out_len": len(frames[-1]), "status": status})
    total = sum(len(f) for f in frames)
    summary = {"out_bytes": total, "n_closes": sum(1 for c in codes if c), "n_1002": codes.count(1002),
               "n_1007": codes.count(1007), "status": OK}
    if out_cap is not None and total > out_cap:
        summary["status"] = ERR_CAPACITY
        return {"out": b"", "out_off": [0] * (n + 1), "runs": [(0, 0)] * n, "summary": summary,
                "conn": [{"code": 0, "out_len": 0, "status": ERR_CAPACITY}] * n}
    off, runs, at, j = [], [], 0, 0
    for s in range(n):
        runs.append((j, 1 if codes[s] else 0))
        if codes[s]:
            off.append(at)
            at += len(frames[s])
            j += 1
            if codes[s] == 1007:
                for t in clear_runs:
                    t[s][1] = 0
    off += [at] * (n + 1 - len(off))
    return {"out": b"".join(frames), "out_off": off, "runs": runs, "conn": conn, "summary": summary}


def rule_cases():
    """One batch that holds every rule once: (streams, results, verdict, reply_conn, enable, keys,
    want codes).  Every frame status alone, every verdict status over a good and over a failed
    decode, closed, not enabled, and all of it again for client streams."""
    rows = []  # (is_server, first_status, verdict, closed, enable, want)
    for srv in (1, 0):
        for fs, code in FRAME_STATUS_CODE.items():
            rows.append((srv, fs, UTF8_VALID, 0, 1, code))
        for v in (UTF8_VALID, UTF8_INVALID, UTF8_NOT_TEXT, UTF8_PREFIX, UTF8_BAD_RANGE):
            rows.append((srv, 0, v, 0, 1, 1007 if v == UTF8_INVALID else 0))
            rows.append((srv, -7, v, 0, 1, 1007 if v == UTF8_INVALID else 1002))  # 1007 wins over 1002
        for fs in (ERR_LAYOUT, ERR_CAPACITY_FRAME, ERR_DEVICE):
            rows.append((srv, fs, UTF8_INVALID, 0, 1, 0))   # the call failed, not the peer
        rows.append((srv, -2, UTF8_VALID, 1, 1, 0))         # the CLOSE echo already closes it
        rows.append((srv, 0, UTF8_INVALID, 1, 1, 0))
        rows.append((srv, -2, UTF8_VALID, 0, 0, 0))         # not enabled
        rows.append((srv, 0, UTF8_INVALID, 0, 0, 0))
    n = len(rows)
    st, res, ver, rep, en, keys = tables(n)
    rng = random.Random(0xC105E)
    for s, (srv, fs, v, closed, e, _) in enumerate(rows):
        st[s]["is_server"], res[s]["first_status"], ver[s]["status"] = srv, fs, v
        rep[s]["closed"], en[s], keys[s] = closed, e, rng.getrandbits(32)
        ver[s]["first_invalid"] = 0xFFFFFFFF if v != UTF8_INVALID else s
    return st, res, ver, rep, en, keys, [r[5] for r in rows]


def mixed_case(seed, n=None):
    """a seeded mix of every input -> (streams, results, verdict, reply_conn, enable, keys)"""
    rng = random.Random(seed)
    n = rng.randint(1, 40) if n is None else n
    st, res, ver, rep, en, keys = tables(n)
    for s in range(n):
        st[s]["is_server"] = rng.random() < 0.6
        res[s]["first_status"] = rng.choice(list(FRAME_STATUS_CODE)) if rng.random() < 0.5 else 0
        ver[s]["status"] = rng.choice([0, 0, 1, 1, 2, 3, 4])
        rep[s]["closed"] = rng.random() < 0.15
        en[s] = rng.random() < 0.85
        keys[s] = rng.getrandbits(32)
    return st, res, ver, rep, en, keys
