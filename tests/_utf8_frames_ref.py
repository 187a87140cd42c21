"""Reference verdicts for the frame-level UTF-8 validation tests (test_utf8_frames_host.py,
test_gpu_utf8_frames.py): uvhttp_ws_utf8_judge_frames and uvhttp_ws_gpu_validate_utf8_streams /
_inplace against a walk over a connection's delivered frames in Python.

The walk follows the decoder's message membership (opcode 1 / 2 starts a message, a
CONTINUATION joins the open one or the carried-in one, FIN ends it, control frames contribute
nothing) and judges the accumulated bytes of a TEXT message with CPython's strict decoder:
_utf8_ref.prefix_verdict after every frame, complete_verdict at FIN.  Frames are built with
_oracle.build_frame; which frames are delivered comes from _oracle.decode_streams."""
import numpy as np

import _oracle as O
import _utf8_ref as R

NONE = 0xFFFFFFFF
CHECK_CLOSE = 0x1
MF, MM = 1 << 24, 1 << 26
DESC_DT = np.dtype([("payload_off", "<u8"), ("payload_len", "<u8"), ("masking_key", "<u4"),
                    ("message", "<u4"), ("opcode", "u1"), ("flags", "u1"),
                    ("header_size", "u1"), ("status", "i1"), ("wire_len", "<u4")])
assert DESC_DT.itemsize == 32


class Fr:
    """one frame: what it is and its wire bytes (masked; rsv: RSV1 set, so it fails)"""

    def __init__(self, op, fin, payload=b"", key=b"\x11\x22\x33\x44", rsv=False):
        self.op, self.fin, self.payload = op, int(bool(fin)), bytes(payload)
        rc, b = O.build_frame(self.payload, op, 1, self.fin, key)
        assert rc > 0
        self.bytes = bytes([b[0] | 0x40]) + b[1:] if rsv else b


PING = lambda: Fr(9, 1, b"\xff\xfe\x80")  # noqa: E731  (a control payload that is not UTF-8)


def fragments(payload, cuts, op=1, between=()):
    """`payload` as one message cut at the byte positions `cuts` (ascending; equal neighbours
    give empty fragments); `between` = frames put after every fragment but the last"""
    edges = [0] + list(cuts) + [len(payload)]
    out = []
    for k in range(len(edges) - 1):
        last = k == len(edges) - 2
        out.append(Fr(op if k == 0 else 0, last, payload[edges[k]:edges[k + 1]]))
        if not last:
            out += list(between)
    return out


def judge(frames, first_frame=0, open_opcode=0, pend=b"", flags=0, bad_range=()):
    """the verdict of one connection's delivered `frames` ([Fr]); bad_range = indices (relative)
    whose payload range lies outside the wire"""
    op = open_opcode if open_opcode in (1, 2) else 0
    acc = bytearray(pend) if op == 1 else bytearray()
    status, first, ntext = R.VALID, NONE, 0
    for i, f in enumerate(frames):
        if f.op >= 8:
            if f.op == 8 and (flags & CHECK_CLOSE) and len(f.payload) > 2 and status == R.VALID:
                if i in bad_range:
                    status = R.BAD_RANGE
                elif R.complete_verdict(f.payload[2:])[0] == R.INVALID:
                    status = R.INVALID
                if status != R.VALID:
                    first = first_frame + i
            continue
        if f.op in (1, 2):
            op, acc = f.op, bytearray()
        if op == 1:
            ntext += 1
            if status == R.VALID:
                if i in bad_range:
                    status = R.BAD_RANGE
                else:
                    acc += f.payload
                    v, tail = R.complete_verdict(acc) if f.fin else R.prefix_verdict(acc)
                    if v == R.INVALID:
                        status = R.INVALID
                    elif not f.fin:  # the valid part is settled: keep the open sequence only
                        acc = acc[len(acc) - tail:]
                if status != R.VALID:
                    first = first_frame + i
        if f.fin:
            op, acc = 0, bytearray()
    state = (b"", 0)
    if status == R.VALID and op == 1:
        status = R.PREFIX
        state = (bytes(acc), len(acc))
    return {"first_invalid": first, "n_text_frames": ntext, "state": state, "status": status}


def summary(verdicts):
    bad = [s for s, v in enumerate(verdicts) if v["status"] in (R.INVALID, R.BAD_RANGE)]
    return {"n_text_frames": sum(v["n_text_frames"] for v in verdicts), "n_invalid_conns": len(bad),
            "first_invalid_conn": bad[0] if bad else NONE,
            "n_open_conns": sum(1 for v in verdicts if v["status"] == R.PREFIX)}


def streams_of(conns, pending=None, gap=0, lead=0):
    """wire and stream table of `conns` ([[Fr]]) back to back (`gap` bytes of FF between, `lead`
    before the first); pending[s] = (opcode, bytes) of a message open from earlier calls"""
    wire, st = bytearray(b"\xff" * lead), np.zeros(len(conns), O.STREAM_DT)
    for s, frames in enumerate(conns):
        b = b"".join(f.bytes for f in frames)
        pop, pby = (pending[s] if pending else None) or (0, 0)
        st[s] = (len(wire), len(b), 65536, pby, pop, MF, MM, 1, 0, 0, 0)
        wire += b + b"\xff" * gap
    return np.frombuffer(bytes(wire), np.uint8).copy(), st


def oracle_decode(wire, st, read_end=None):
    """the oracle's stream decode -> (decoded wire, desc[DESC_DT] of the delivered frames in
    connection order, first_frame per connection, n_delivered per connection, outcomes)"""
    w = wire.copy()
    cap = w.size // 2 + 1
    out, frames, total = O.decode_streams(w, st, read_end=read_end, max_frames=cap)
    assert total <= cap
    desc = np.zeros(max(1, total), DESC_DT)
    for name, src in (("payload_off", "payload_off"), ("payload_len", "payload_len"), ("masking_key", "key"),
                      ("opcode", "opcode"), ("flags", "flags"), ("header_size", "header_size"),
                      ("wire_len", "wire_len")):
        desc[name][:total] = frames[src]
    nd = [int(x) for x in out["n_frames"]]
    first = [int(x) for x in np.cumsum([0] + nd[:-1])]
    return w, desc[:total], first, nd, out


def delivered(conns, nd):
    return [frames[:n] for frames, n in zip(conns, nd)]


def fragment_randomly(rng, rows, p_ping=0.3):
    """[(opcode, payload)] -> [Fr]: every message cut into 1-5 fragments at random positions
    (the first never empty, as the reference does not open a message on an empty first
    fragment), PINGs sprinkled in"""
    out = []
    for op, b in rows:
        n = rng.randint(1, 5)
        cuts = sorted(rng.randint(1, len(b)) for _ in range(n - 1)) if len(b) >= 1 else []
        for f in fragments(b, cuts, op):
            out.append(f)
            if not f.fin and rng.random() < p_ping:
                out.append(PING())
    return out
