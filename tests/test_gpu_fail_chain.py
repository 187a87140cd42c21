"""The per-batch chain of a TLS echo or room server on the device (tests/test_gpu_parts_chain.py)
with the fail points between the judging and the sends: seal_records (the clients' messages) ->
open_records -> ws_streams -> decode_reads -> validate_utf8_streams -> fail_points ->
control_replies -> echo (or relay) -> close_frames -> seal_parts.  24 connections with keys of
their own in rooms of 1, 3, 8, 6 and 6; the first three rooms hold one sender of invalid UTF-8 each,
the fourth the other scripted connections, the fifth nobody who fails.

The oracle opens every connection's records.  A failed connection's plaintext is exactly [its
echoes before the cut][its replies before the cut][the close fail[s].code names]; a bad CLOSE is
not echoed; a PING after the cut gets no PONG; no receiver gets a byte of an offender's message;
connections that did not fail send what the chain without the pass sends.  And the gap this
closes: without the pass the offender's bytes do reach its room."""
import ctypes as C
import random

import numpy as np
import pytest

import _close_ref as CR
import _echo_ref as ER
import _fail_ref as F
import _oracle as O
import _relay_ref as RL
import _replies_ref as RR
import _tls_send_ref as TS
from test_gpu_echo import _parse_unmasked

pytestmark = pytest.mark.gpu

S = 24
ROOM = [0] + [1] * 3 + [2] * 8 + [3] * 6 + [4] * 6
R = 5
ALONE, OF_THREE, OF_EIGHT, BAD_CODE, SHORT_CLOSE, PING, PEER_CLOSE, PROTOCOL_ERROR, INVALID_THEN_ERROR = 0, 2, 7, 12, 13, 14, 15, 16, 17
# what the rule gives the scripted connections: (reason, the cut's frame in the connection, code)
WANT = {ALONE: (F.R_UTF8, 1, 1007), OF_THREE: (F.R_UTF8, 1, 1007), OF_EIGHT: (F.R_UTF8, 2, 1007),
        BAD_CODE: (F.R_CLOSE_CODE, 1, 1002), SHORT_CLOSE: (F.R_CLOSE_LEN, 1, 1002),
        PROTOCOL_ERROR: (F.R_DECODE, None, 1002), INVALID_THEN_ERROR: (F.R_UTF8, 0, 1007)}
MARKS = {ALONE: b"evil zero", OF_THREE: b"evil two", OF_EIGHT: b"evil seven"}


@pytest.fixture(scope="module")
def torch():
    import torch as t
    if not t.cuda.is_available():
        pytest.skip("no GPU")
    return t


def _frames(rng, c):
    T, B, K, P, CL = ER.text, ER.binary, ER.cont, ER.ping, ER.close
    rsv = ER.Fr(1, 1, b"rsv", rsv=True)
    if c == ALONE:
        return [T(b"fine"), T(b"\xff\xfe " + MARKS[c]), T(b"later " + MARKS[c])]
    if c == OF_THREE:
        return [T(b"ok two"), T(b"\xc0\x80 " + MARKS[c]), P(b"after the cut"), T(b"again " + MARKS[c])]
    if c == OF_EIGHT:
        return [P(b"early"), T(b"seven ", 0), K(b"\xff " + MARKS[c], 0), K(b" end"), T(b"more " + MARKS[c])]
    if c == BAD_CODE:
        return [T(b"hi twelve"), CL(F.code(1005, b"x")), T(b"post")]
    if c == SHORT_CLOSE:
        return [P(b"p13"), CL(b"\x03"), P(b"late")]
    if c == PING:
        return [P(b"are you there"), T(b"hello"), P()]
    if c == PEER_CLOSE:
        return [T(b"bye"), CL(F.code(1000, b"done")), T(b"unheard")]
    if c == PROTOCOL_ERROR:
        return [T(b"before"), B(rng.randbytes(300)), rsv, T(b"after")]
    if c == INVALID_THEN_ERROR:
        return [T(b"\xc0\x80"), B(b"ok"), rsv]
    ascii_ = lambda n: bytes(rng.choice(b"abcdefghij klmnop") for _ in range(n))  # noqa: E731
    rows = [(2, rng.randbytes(rng.choice([0, 1, 20, 200, 3000]))) if rng.random() < 0.5 else
            (1, ascii_(rng.choice([0, 1, 20, 200]))) for _ in range(rng.randint(0, 4))]
    return ER.FR.fragment_randomly(rng, rows)


def _chain(torch, relay, with_pass):
    """one batch through the whole chain -> (frames per connection, the reads they came in, the
    opened plaintext per connection, the fail entries or None)"""
    import uvhttp_amd as U
    t = torch
    rng = random.Random(417)
    kinds = [TS.KEY_KINDS[rng.randrange(6)] for _ in range(S)]
    keys = np.concatenate([TS.make_key(rng, k) for k in kinds] + [TS.make_key(rng, k) for k in kinds])
    conns, plains, recs_rows, tls_st, reads = [], [], [], np.zeros(S, O.TLS_STREAM_DT), []
    src_pos, out_pos = 0, 0
    for c in range(S):
        conns.append(_frames(rng, c))
        plain = ER.raw(conns[c])
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
    max_frames = max_echoes = max_replies = 512
    echo_cap = (src_pos + 14 * max_echoes + 15) // 16 * 16
    reply_cap, close_cap = 131 * 64, 32 * S
    arena = t.full((echo_cap + reply_cap + close_cap,), 0xEE, dtype=t.uint8, device="cuda")
    sends = np.zeros(S, TS.TLS_SEND_DT)
    seq_s = [rng.randrange(1 << 40) for _ in range(S)]
    for c in range(S):
        sends[c] = (seq_s[c], 0xDEAD, 0xBEEF, S + c, 23, 0, 0)
    d_sends = dev(sends)
    runs_e = t.zeros(2 * S, dtype=t.int32, device="cuda")
    runs_r = t.zeros(2 * S, dtype=t.int32, device="cuda")
    runs_c = t.zeros(2 * S, dtype=t.int32, device="cuda")
    fan = max(ROOM.count(r) for r in range(R)) if relay else 1
    max_out_records = fan * (max_echoes + echo_cap // 16384 + 1) + max_replies + S
    sealed = t.zeros(fan * echo_cap + reply_cap + close_cap + max_out_records * 64, dtype=t.uint8, device="cuda")
    d_room = dev(np.array(ROOM, np.uint32))

    eng_t.seal_records(d_src, dev(seal), len(seal), d_keys, len(keys), cipher[:out_pos])
    tls_dev = dev(tls_st)
    recs, res = eng_t.open_records(cipher, d_keys, len(keys), tls_dev, S, max_records, plain_out[:plain_cap],
                                   wire_len=out_pos)
    eng_t.ws_streams(res, recs, S, tls_dev, plain_out, ws_dev, read_end)
    desc, wres = eng_w.decode_streams(plain_out, ws_dev, S, max_frames, wire_len=plain_cap, read_end=read_end,
                                      n_reads=max_records)
    verdict, _ = eng_w.validate_utf8_streams(plain_out, desc, max_frames, ws_dev, wres, S, flags=U.UTF8_CHECK_CLOSE,
                                             wire_len=plain_cap)
    fail = None
    if with_pass:   # the one new call: the send passes below take its tables, nothing else changes
        wres, verdict, fail, _ = eng_w.fail_points_streams(plain_out, desc, max_frames, wres, S, verdict,
                                                           flags=U.FAIL_CHECK_CLOSE, wire_len=plain_cap)
    _, r_off, r_conn, _ = eng_w.control_replies_streams(
        plain_out, desc, max_frames, ws_dev, wres, S, max_replies, reply_cap, out=arena[echo_cap:echo_cap + reply_cap],
        runs=runs_r, wire_len=plain_cap)
    if relay:
        _, e_off, _, _, _, _ = eng_w.relay_messages_streams(
            plain_out, desc, max_frames, ws_dev, wres, S, d_room, R, max_echoes, echo_cap, out=arena[:echo_cap],
            recv_room=d_room, n_receivers=S, sends=d_sends[8:], send_stride=32, wire_len=plain_cap)
        first_runs, first_stride = d_sends[8:], 32
    else:
        _, e_off, _, _, _ = eng_w.echo_messages_streams(
            plain_out, desc, max_frames, ws_dev, wres, S, max_echoes, echo_cap, out=arena[:echo_cap], runs=runs_e,
            wire_len=plain_cap)
        first_runs, first_stride = runs_e, 8
    _, c_off, c_conn, _ = eng_w.close_frames_streams(
        ws_dev, wres, S, close_cap, verdict=verdict, reply_conn=r_conn, out=arena[echo_cap + reply_cap:], runs=runs_c)
    parts = [(0, echo_cap, e_off, first_runs, first_stride, max_echoes),
             (echo_cap, reply_cap, r_off, runs_r, 8, max_replies),
             (echo_cap + reply_cap, close_cap, c_off, runs_c, 8, S)]
    _, sres, ssum = eng_t.seal_parts(arena, parts, d_sends, S, d_keys, len(keys), max_out_records, sealed)
    t.cuda.synchronize()  # the first host read

    sr = sres.cpu().numpy()[:S * 48].view(TS.TLS_SEND_RESULT_DT)
    assert (sr["status"] == 0).all()
    host_sealed = sealed.cpu().numpy()
    open_st = np.zeros(S, O.TLS_STREAM_DT)
    for c in range(S):
        open_st[c] = (int(sr[c]["out_off"]), int(sr[c]["out_len"]), seq_s[c], S + c, 0)
    total = int(ssum.cpu().numpy().view(TS.TLS_SEND_SUMMARY_DT)[0]["out_bytes"])
    o_recs, o_res, o_out = O.tls_open_batch(host_sealed[:max(1, total)], keys, open_st, out_cap=total + 16)
    got = []
    for c in range(S):
        r = o_res[c]
        assert int(r["n_delivered"]) == int(sr[c]["n_records"]) and int(r["status"]) == 0, c
        got.append(b"".join(o_out[rec["out_off"]:rec["out_off"] + rec["content_len"]].tobytes()
                            for rec in o_recs[r["first_record"]:r["first_record"] + r["n_delivered"]]))
    codes = [c["code"] for c in eng_w.read_close_conns(c_conn, S)]
    fails = None if fail is None else eng_w.read_fail_conns(fail, S)
    first = wres.cpu().numpy()[:S * 64].view(RL.RESULT_DT)["first_frame"].tolist()
    eng_w.close()
    eng_t.close()
    return conns, reads, got, fails, codes, first


@pytest.fixture(scope="module")
def runs(torch):
    """(relay, with the pass) -> the chain's outcome; every test below reads these four runs"""
    return {(relay, wp): _chain(torch, relay, wp) for relay in (False, True) for wp in (False, True)}


def _cut(conns, fails, first):
    """every connection's bytes ending just before its cut frame (whole when it has none)"""
    return [ER.raw(f[:fl["frame"] - first[c]]) if fl["reason"] >= F.R_UTF8 else ER.raw(f)
            for c, (f, fl) in enumerate(zip(conns, fails))]


@pytest.mark.parametrize("relay", [False, True])
def test_failed_connections_stop_at_the_violation(runs, relay):
    conns, reads, got, fails, codes, first = runs[relay, True]
    for c in range(S):
        reason, rel, code = WANT.get(c, (F.R_NONE, None, 0))
        assert (fails[c]["reason"], fails[c]["code"], fails[c]["status"]) == (reason, code, F.OK), c
        assert fails[c]["frame"] == (F.NONE if reason == F.R_NONE else first[c] + (2 if rel is None else rel)), c
    assert codes == [f["code"] for f in fails]           # close_frames sends what the fail entry names
    cut = _cut(conns, fails, first)
    rd = [None if fails[c]["reason"] >= F.R_UTF8 else reads[c] for c in range(S)]
    want_r = RR.expected_batch(cut, reads=rd)
    reply_bytes = []
    for w in want_r["conn"]:
        lo = want_r["out_off"][w["first_reply"]]
        reply_bytes.append(want_r["out"][lo:lo + w["out_len"]])
    if relay:
        lists = RL.room_lists(RL.expected(cut, ROOM, R, ROOM, reads=rd))
        echo_bytes = [b"".join(lists[ROOM[c]]) for c in range(S)]
    else:
        want_e = ER.expected_batch(cut, reads=rd)
        echo_bytes = []
        for w in want_e["conn"]:
            lo = want_e["out_off"][w["first_echo"]]
            echo_bytes.append(want_e["out"][lo:lo + w["out_len"]])
    for c in range(S):
        close = CR.close_frame(fails[c]["code"], 1) if fails[c]["code"] else b""
        assert got[c] == echo_bytes[c] + reply_bytes[c] + close, c
    # a bad CLOSE is not echoed: the one CLOSE frame those connections get is the server's 1002
    for c in (BAD_CODE, SHORT_CLOSE):
        closes = [p for op, p in _parse_unmasked(got[c]) if op == 8]
        assert closes == [F.code(1002, b"protocol error")], c
    # a PING after the cut gets no PONG, one before it does
    assert [p for op, p in _parse_unmasked(got[OF_THREE]) if op == 10] == []
    assert [p for op, p in _parse_unmasked(got[OF_EIGHT]) if op == 10] == [b"early"]
    assert [p for op, p in _parse_unmasked(got[SHORT_CLOSE]) if op == 10] == [b"p13"]
    # every TEXT frame anybody receives is UTF-8, and no byte of an offender's message or of its later ones
    for c in range(S):
        for op, p in _parse_unmasked(got[c]):
            if op == 1:
                p.decode("utf-8")
        for mark in MARKS.values():
            assert mark not in got[c], (c, mark)
    if relay:   # the rooms' good senders still reach everybody
        assert b"ok two" in got[1] and b"ok two" in got[3] and b"fine" in got[ALONE]


@pytest.mark.parametrize("relay", [False, True])
def test_connections_that_did_not_fail_send_the_same(runs, relay):
    _, _, got, fails, _, _ = runs[relay, True]
    _, _, before, none, codes, _ = runs[relay, False]
    assert none is None
    cut_rooms = {ROOM[c] for c in range(S) if fails[c]["reason"] >= F.R_UTF8}
    same = [c for c in range(S) if (ROOM[c] not in cut_rooms if relay else fails[c]["reason"] < F.R_UTF8)]
    assert len(same) >= (1 if relay else 17) and (relay or PROTOCOL_ERROR in same)
    for c in same:
        assert got[c] == before[c], c
    if not relay:
        assert all(got[c] != before[c] for c in range(S) if fails[c]["reason"] >= F.R_UTF8)


def test_without_the_pass_the_offender_reaches_its_room(runs):
    """the gap being closed (existing behaviour, unchanged): the same batch through the chain
    without the pass relays the invalid message to every member of the offender's room, who must
    then fail their own connections (RFC 6455 §8.1), and echoes a CLOSE with a code that must not
    be on the wire"""
    _, _, got, _, codes, _ = runs[True, False]
    for c in range(S):
        for off, mark in MARKS.items():
            assert (mark in got[c]) == (ROOM[c] == ROOM[off]), (c, off)
    assert codes[OF_THREE] == 1007 and b"\xc0\x80 " + MARKS[OF_THREE] in got[1]
    _, _, echo, _, codes, _ = runs[False, False]
    assert (8, F.code(1005, b"x")) in _parse_unmasked(echo[BAD_CODE]) and codes[BAD_CODE] == 0
