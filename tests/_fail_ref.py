"""Reference of the fail points (uvhttp_ws_fail_points, uvhttp_ws_gpu_fail_points_streams;
include/uvhttp_ws_amd.h): the rule in plain Python over numpy copies of the tables, the numpy
layouts of the two new structs, and the shared case builders of the host and GPU tests:

  rule_cases()    real frames through the oracle's stream decode and the UTF-8 reference verdicts
                  (tests/_utf8_frames_ref.py): every reason, every boundary close code, every place
                  a violation can stand relative to the CLOSE, each with what the rule must give
  synth_batch()   tables written directly (the pass reads descriptors, results, verdicts and two
                  wire bytes, nothing else), for shapes: many connections, long connections
"""
import random

import numpy as np

import _close_ref as CR
import _echo_ref as ER
import _utf8_frames_ref as FR
import _utf8_ref as R
from _relay_ref import RESULT_DT

NONE = 0xFFFFFFFF
CHECK_CLOSE = 0x1
OK, BAD_RANGE = 0, 2
R_NONE, R_DECODE, R_UTF8, R_CLOSE_LEN, R_CLOSE_CODE = range(5)
ERR_UTF8, ERR_CLOSE = -12, -13
CALL_FAILED = (-9, -10, -11)
DESC_DT, VERDICT_DT = FR.DESC_DT, CR.VERDICT_DT
FAIL_DT = np.dtype([("frame", "<u4"), ("n_dropped", "<u4"), ("code", "<u2"), ("reason", "u1"), ("status", "u1"),
                    ("reserved", "<u4")])
SUMMARY_DT = np.dtype([("n_dropped", "<u8"), ("n_decode", "<u4"), ("n_utf8", "<u4"), ("n_close_len", "<u4"),
                       ("n_close_code", "<u4"), ("n_bad_range", "<u4"), ("first_failed", "<u4")])
assert FAIL_DT.itemsize == 16 and SUMMARY_DT.itemsize == 32
BOUNDARY_CODES = [999, 1000, 1003, 1004, 1006, 1007, 1014, 1015, 1016, 2999, 3000, 4999, 5000, 65535]


def code_valid(c):
    """RFC 6455 §7.4.1-2 plus the IANA-registered 1012-1014"""
    return 1000 <= c <= 1003 or 1007 <= c <= 1014 or 3000 <= c <= 4999


def fail_points_ref(wire, desc, max_frames, results, n, verdict=None, enable=None, flags=0, wire_len=None):
    """-> (results_out[RESULT_DT], verdict_out[VERDICT_DT] or None, fail[FAIL_DT], summary[SUMMARY_DT])"""
    wire_len = len(wire) if wire_len is None else wire_len
    res = np.array(results[:max(1, n)], RESULT_DT, copy=True)
    ver = None if verdict is None else np.array(verdict[:max(1, n)], VERDICT_DT, copy=True)
    fail = np.zeros(max(1, n), FAIL_DT)
    summ = np.zeros(1, SUMMARY_DT)
    summ["first_failed"] = NONE
    fail["frame"][:n] = NONE
    for s in range(n):
        fs = int(results[s]["first_status"])
        if (enable is not None and not enable[s]) or fs in CALL_FAILED:
            continue
        ff, nd_all = int(results[s]["first_frame"]), int(results[s]["n_delivered"])
        nd = 0 if ff >= max_frames else min(nd_all, max_frames - ff)
        c = next((f for f in range(ff, ff + nd) if desc[f]["opcode"] == 8 and desc[f]["status"] == 0), None)
        cut, reason = None, R_NONE
        if (flags & CHECK_CLOSE) and c is not None:
            ln, off = int(desc[c]["payload_len"]), int(desc[c]["payload_off"])
            if ln == 1:
                cut, reason = c, R_CLOSE_LEN
            elif ln >= 2:
                if off + ln > wire_len:
                    fail[s]["status"] = BAD_RANGE
                    summ["n_bad_range"] += 1
                    continue
                if not code_valid(int(wire[off]) << 8 | int(wire[off + 1])):
                    cut, reason = c, R_CLOSE_CODE
        close_cut = cut is not None
        u = NONE if verdict is None else int(verdict[s]["first_invalid"])
        if verdict is not None and verdict[s]["status"] == CR.UTF8_INVALID and ff <= u < ff + nd and \
                (c is None or u <= c) and (cut is None or u < cut):   # the earlier frame; 1002 on the same one
            cut, reason = u, R_UTF8
        if cut is not None:
            fail[s] = (cut, ff + nd - cut, 1007 if reason == R_UTF8 else 1002, reason, OK, 0)
            res[s]["n_delivered"] = cut - ff
            res[s]["n_frames"] = cut - ff + 1
            res[s]["status"] = -1
            res[s]["first_status"] = ERR_UTF8 if reason == R_UTF8 else ERR_CLOSE
        elif fs < 0:
            reason = R_DECODE
            fail[s] = ((ff + nd_all) & 0xFFFFFFFF, 0, 1002, reason, OK, 0)
        if verdict is not None and u != NONE and c is not None and (u > c or (close_cut and u == c)):
            ver[s]["status"], ver[s]["first_invalid"], ver[s]["pend"], ver[s]["n"] = CR.UTF8_VALID, NONE, 0, 0
        summ["n_dropped"] += int(fail[s]["n_dropped"])
        key = {R_DECODE: "n_decode", R_UTF8: "n_utf8", R_CLOSE_LEN: "n_close_len", R_CLOSE_CODE: "n_close_code"}
        if reason != R_NONE:
            summ[key[reason]] += 1
            if summ["first_failed"][0] == NONE:
                summ["first_failed"] = s
    return res, ver, fail, summ


def as_bytes(a):
    return None if a is None else np.ascontiguousarray(a).view(np.uint8).reshape(-1).tobytes()


def ref_bytes(ref, n):
    """the reference's four outputs as the bytes a call must write for n connections"""
    res, ver, fail, summ = ref
    return (as_bytes(res[:n]), None if ver is None else as_bytes(ver[:n]), as_bytes(fail[:n]), as_bytes(summ))


# ---- real frames ----------------------------------------------------------------------------
def code(c, reason=b""):
    return int(c).to_bytes(2, "big") + reason


BAD = b"\xff\xfe bad"


def rule_rows():
    """[(name, frames, pending (opcode, bytes) or None, tweak, want)]: want = (reason, the cut's
    frame relative to the connection's first or None, code, status) under CHECK_CLOSE with a
    verdict; tweak = "off" (not enabled), a call-failure status, "range" (the first CLOSE's payload
    moved outside the wire) or None"""
    T, B, K, P, CL = ER.text, ER.binary, ER.cont, ER.ping, ER.close
    rsv = lambda: ER.Fr(1, 1, b"rsv", rsv=True)  # noqa: E731
    rows = [("clean", [T(b"hello"), P(b"x"), B(b"\xff\xfe")], None, None, (R_NONE, None, 0, OK)),
            ("empty", [], None, None, (R_NONE, None, 0, OK))]
    for c in BOUNDARY_CODES:
        want = (R_NONE, None, 0, OK) if code_valid(c) else (R_CLOSE_CODE, 1, 1002, OK)
        rows.append((f"code {c}", [T(b"a"), CL(code(c)), T(b"after")], None, None, want))
    rows += [
        ("close 0 bytes", [T(b"a"), CL(b""), P(b"p")], None, None, (R_NONE, None, 0, OK)),
        ("close 1 byte", [T(b"x"), P(b"p"), CL(b"\x03"), P(b"late")], None, None, (R_CLOSE_LEN, 2, 1002, OK)),
        ("close 125 bytes", [CL(code(1000, b"r" * 123))], None, None, (R_NONE, None, 0, OK)),
        ("close 125 bytes, bad code", [B(b"b"), CL(code(1005, b"r" * 123))], None, None, (R_CLOSE_CODE, 1, 1002, OK)),
        ("utf8 before the close", [T(b"ok"), T(BAD), P(b"late"), CL(code(1000)), T(b"later")], None, None,
         (R_UTF8, 1, 1007, OK)),
        ("utf8 at the close", [T(b"ok"), CL(code(1000, b"\xff\xfe"))], None, None, (R_UTF8, 1, 1007, OK)),
        ("utf8 after the close", [T(b"ok"), CL(code(1000)), T(BAD)], None, None, (R_NONE, None, 0, OK)),
        ("both on one frame", [T(b"ok"), CL(code(1005, b"\xff"))], None, None, (R_CLOSE_CODE, 1, 1002, OK)),
        ("bad close before invalid text", [CL(b"\x03"), T(BAD)], None, None, (R_CLOSE_LEN, 0, 1002, OK)),
        ("carried-in message", [K(b"\x28 more"), T(b"next")], (1, b"caf\xc3"), None, (R_UTF8, 0, 1007, OK)),
        ("carried-in message, fine", [K(b"\xa9 ok"), T(b"next")], (1, b"caf\xc3"), None, (R_NONE, None, 0, OK)),
        ("cut at the last frame", [T(b"a"), B(b"b"), T(BAD)], None, None, (R_UTF8, 2, 1007, OK)),
        ("second fragment", [T(b"one ", 0), P(b"mid"), K(b"\xff", 0), P(b"late"), K(b"end")], None, None,
         (R_UTF8, 2, 1007, OK)),
        ("decode failure", [T(b"a"), rsv(), T(b"never")], None, None, (R_DECODE, None, 1002, OK)),
        ("decode failure after invalid text", [T(BAD), B(b"ok"), rsv()], None, None, (R_UTF8, 0, 1007, OK)),
        ("decode failure after a bad close", [P(b"p"), CL(b"\x00"), rsv()], None, None, (R_CLOSE_LEN, 1, 1002, OK)),
        ("only the first close", [CL(code(1000)), CL(b"\x03")], None, None, (R_NONE, None, 0, OK)),
        ("not enabled", [T(BAD), CL(b"\x03")], None, "off", (R_NONE, None, 0, OK)),
        ("close outside the wire", [T(b"a"), CL(code(1000))], None, "range", (R_NONE, None, 0, BAD_RANGE)),
        ("invalid text, close outside the wire", [T(BAD), CL(code(1005))], None, "range", (R_NONE, None, 0, BAD_RANGE)),
    ]
    for fs in CALL_FAILED:
        rows.append((f"call failed {fs}", [T(BAD), CL(b"\x03")], None, fs, (R_NONE, None, 0, OK)))
    return rows


class Batch:
    """one decoded batch: what the passes read (wire, desc, st, res, ver, en), what made it (conns,
    pending) and, for rule_cases, what the rule must give (want)"""

    def __init__(self, conns, pending=None, tweaks=None, wants=None):
        n = len(conns)
        self.conns, self.pending, self.n, self.wants = conns, pending or [None] * n, n, wants
        wire, self.st = ER.streams_of(conns, pending=self.pending)
        self.wire, self.desc, self.first, self.nd, out = FR.oracle_decode(wire, self.st)
        self.desc = self.desc.copy()
        self.res = np.zeros(max(1, n), RESULT_DT)
        self.ver = np.zeros(max(1, n), VERDICT_DT)
        self.en = np.ones(max(1, n), np.uint8)
        for s in range(n):
            failed = int(out[s]["rc"]) != 0
            self.res[s] = (self.first[s], self.nd[s] + failed, self.nd[s], int(out[s]["rc"]), int(out[s]["reason"]),
                           int(out[s]["calls"]), int(out[s]["consumed"]), int(out[s]["recv_size"]),
                           int(out[s]["frag_size"]), int(out[s]["recv_pos"]), 0)
            pend = self.pending[s]
            tail = R.prefix_verdict(pend[1])[1] if pend and pend[0] == 1 else 0
            v = FR.judge(conns[s][:self.nd[s]], self.first[s], pend[0] if pend else 0,
                         pend[1][len(pend[1]) - tail:] if tail else b"", CHECK_CLOSE)
            self.ver[s]["first_invalid"], self.ver[s]["n_text_frames"] = v["first_invalid"], v["n_text_frames"]
            self.ver[s]["status"], self.ver[s]["n"] = v["status"], v["state"][1]
            self.ver[s]["pend"][:v["state"][1]] = list(v["state"][0])
            tw = tweaks[s] if tweaks else None
            if tw == "off":
                self.en[s] = 0
            elif tw == "range":
                c = next(f for f in range(self.first[s], self.first[s] + self.nd[s]) if self.desc[f]["opcode"] == 8)
                self.desc[c]["payload_off"] = len(self.wire) - 1
            elif tw is not None:
                self.res[s]["first_status"], self.res[s]["status"] = tw, -1
        self.max_frames = len(self.desc)

    def tables(self):
        return self.wire, self.desc, self.max_frames, self.res, self.n


def rule_cases():
    rows = rule_rows()
    return Batch([r[1] for r in rows], [r[2] for r in rows], [r[3] for r in rows], [r[4] for r in rows]), [r[0] for r in rows]


def clean_batch():
    """no violation anywhere: nothing may change"""
    T, B, K, P, CL = ER.text, ER.binary, ER.cont, ER.ping, ER.close
    conns = [[T(b"hello"), P(b"x"), B(b"\xff\xfe")], [], [T(b"a", 0), K(b"b")], [T(b"bye"), CL(code(1000, b"done")), T(b"x")],
             [CL(b"")], [K(b"\xa9")], [T(b"open \xe2\x82", 0)], [CL(code(4999))], [B(BAD), CL(code(3000))]]
    pending = [None] * len(conns)
    pending[5] = (1, b"caf\xc3")
    return Batch(conns, pending)


# ---- tables written directly ------------------------------------------------------------------
def spec(n, close=None, utf8=None, fs=0, enable=1, bad_range=False):
    """one connection of n delivered frames: close = [(frame, payload_len, code)] CLOSE frames,
    utf8 = the frame its verdict blames, fs = its decode's first_status"""
    return dict(n=n, close=close or [], utf8=utf8, fs=fs, enable=enable, bad_range=bad_range)


def synth_batch(specs, rng=None, gap=0):
    """-> (wire, desc, max_frames, results, n, verdict, enable) of the connections `specs`"""
    rng = rng or random.Random(1)
    n = len(specs)
    total = sum(sp["n"] + gap for sp in specs)
    desc = np.zeros(max(1, total), DESC_DT)
    desc["opcode"] = np.array([1, 2, 0, 9, 10, 0, 1], np.uint8)[np.arange(max(1, total)) % 7]
    desc["payload_len"] = np.arange(max(1, total)) % 50
    res, ver, en = np.zeros(max(1, n), RESULT_DT), np.zeros(max(1, n), VERDICT_DT), np.ones(max(1, n), np.uint8)
    wire, at = bytearray(b"\xee" * 5), 0
    for s, sp in enumerate(specs):
        res[s] = (at, sp["n"] + (sp["fs"] < 0), sp["n"], -1 if sp["fs"] < 0 else 0, sp["fs"], 1 + s % 3,
                  rng.getrandbits(40), 65536, rng.getrandbits(8), rng.getrandbits(40), 0)
        for i, (f, ln, c) in enumerate(sp["close"]):
            desc[at + f]["opcode"], desc[at + f]["payload_len"] = 8, ln
            desc[at + f]["payload_off"] = (1 << 40) if sp["bad_range"] and i == 0 else len(wire)
            wire += (code(c) + b"r" * 123)[:ln]
        ver[s]["first_invalid"], ver[s]["n_text_frames"] = NONE, rng.getrandbits(6)
        if sp["utf8"] is not None:
            ver[s]["first_invalid"], ver[s]["status"] = at + sp["utf8"], CR.UTF8_INVALID
        elif rng.random() < 0.2:
            ver[s]["status"], ver[s]["n"], ver[s]["pend"][0] = CR.UTF8_PREFIX, 1, 0xC3
        en[s] = sp["enable"]
        at += sp["n"]
        for g in range(gap):   # descriptors of nobody: a bad CLOSE that must not count
            desc[at + g]["opcode"], desc[at + g]["payload_len"] = 8, 1
        at += gap
    return np.frombuffer(bytes(wire), np.uint8).copy(), desc, total, res, n, ver, en


def every_reason(n=3):
    """specs that hold every reason, status and not-judged kind once; n = frames per connection"""
    m = n - 1
    return [spec(n), spec(n, utf8=m), spec(n, close=[(m, 1, 0)]), spec(n, close=[(0, 2, 1005)]),
            spec(n, close=[(0, 2, 1000)], utf8=m), spec(n, fs=-2), spec(n, utf8=0, fs=-7), spec(n, utf8=0, enable=0),
            spec(n, close=[(0, 1, 0)], fs=-10), spec(n, close=[(m, 125, 1000)], bad_range=True), spec(0),
            spec(n, close=[(0, 125, 65535)], utf8=0)]


def seeded_specs(seed):
    rng = random.Random(seed)
    specs = every_reason(rng.randint(1, 6))
    for _ in range(rng.randint(0, 60)):
        n = rng.choice([0, 1, 1, 2, 3, 5, 9, 40])
        close = sorted({rng.randrange(n) for _ in range(rng.randint(0, 2))}) if n else []
        close = [(f, rng.choice([0, 1, 2, 2, 2, 7, 125]), rng.choice(BOUNDARY_CODES + [1000, 1001, 1008, 3500]))
                 for f in close]
        specs.append(spec(n, close, rng.randrange(n) if n and rng.random() < 0.3 else None,
                          rng.choice([0, 0, 0, 0, -1, -3, -8, -9, -10, -11]), rng.random() < 0.9,
                          rng.random() < 0.1))
    rng.shuffle(specs)
    return specs, rng
