"""The whole per-batch chain of a TLS echo or room server on the device, closed by ONE seal:
seal_records (the clients' messages) -> open_records -> ws_streams -> decode_reads ->
validate_utf8_streams -> control_replies -> echo (or relay) -> close_frames -> seal_parts over
three parts of one send arena.  No host read before the end.  24 connections with keys of their
own, among them a protocol error, invalid UTF-8 (alone, and before a protocol error), a PING, a
peer CLOSE (alone, and before a protocol error) and a fragmented message.

The oracle opens every connection's records with consecutive sequence numbers from its write
sequence number; the plaintext is exactly [echo frames][replies][close]; a failed connection's
last frame is its CLOSE; with d_clear_runs a 1007 connection's send is the close alone."""
import ctypes as C
import random

import numpy as np
import pytest

import _close_ref as CR
import _echo_ref as ER
import _oracle as O
import _relay_ref as RL
import _replies_ref as RR
import _tls_send_ref as TS
from test_gpu_echo import _parse_unmasked

pytestmark = pytest.mark.gpu

S = 24
# the scripted connections: what the server closes them with (0: it does not)
PROTOCOL_ERROR, INVALID_UTF8, PING, PEER_CLOSE, FRAGMENTED, INVALID_THEN_ERROR, CLOSE_THEN_ERROR = 3, 5, 7, 9, 11, 13, 15
CODES = {PROTOCOL_ERROR: 1002, INVALID_UTF8: 1007, INVALID_THEN_ERROR: 1007}


@pytest.fixture(scope="module")
def torch():
    import torch as t
    if not t.cuda.is_available():
        pytest.skip("no GPU")
    return t


def _rsv(frame):
    b = bytearray(frame.bytes)
    b[0] |= 0x40
    return bytes(b)


def _conn_bytes(rng, c):
    ascii_ = lambda n: bytes(rng.choice(b"abcdefghij klmnop") for _ in range(n))  # noqa: E731
    if c == PROTOCOL_ERROR:
        return ER.raw([ER.text(b"before"), ER.binary(rng.randbytes(300))]) + _rsv(ER.text(b"rsv")) + ER.raw([ER.text(b"after")])
    if c == INVALID_UTF8:
        return ER.raw([ER.text(b"fine"), ER.text(b"\xff\xfe bad"), ER.text(b"later")])
    if c == PING:
        return ER.raw([ER.ping(b"are you there"), ER.text(b"hello"), ER.ping()])
    if c == PEER_CLOSE:
        return ER.raw([ER.text(b"bye"), ER.close(b"\x03\xe8done"), ER.text(b"unheard")])
    if c == FRAGMENTED:
        return ER.raw([ER.text(b"one ", 0), ER.ping(b"mid"), ER.cont(b"two ", 0), ER.cont(b"three"), ER.binary(rng.randbytes(20000))])
    if c == INVALID_THEN_ERROR:
        return ER.raw([ER.text(b"\xc0\x80"), ER.binary(b"ok")]) + _rsv(ER.binary(b"rsv"))
    if c == CLOSE_THEN_ERROR:
        return ER.raw([ER.close(b"\x03\xe9")]) + _rsv(ER.text(b"rsv"))
    rows = [(2, rng.randbytes(rng.choice([0, 1, 20, 200, 3000]))) if rng.random() < 0.5 else
            (1, ascii_(rng.choice([0, 1, 20, 200]))) for _ in range(rng.randint(0, 4))]
    return ER.raw(ER.FR.fragment_randomly(rng, rows))


@pytest.mark.parametrize("clear", [False, True])
@pytest.mark.parametrize("relay", [False, True])
def test_one_seal_per_batch(torch, relay, clear):
    import uvhttp_amd as U
    t = torch
    rng = random.Random(91)
    R = 4
    room = [(s * 7 + s // 5) % R for s in range(S)]
    kinds = [TS.KEY_KINDS[rng.randrange(6)] for _ in range(S)]
    keys = np.concatenate([TS.make_key(rng, k) for k in kinds] + [TS.make_key(rng, k) for k in kinds])
    plains, recs_rows, tls_st, reads = [], [], np.zeros(S, O.TLS_STREAM_DT), []
    src_pos, out_pos = 0, 0
    for c in range(S):
        plain = _conn_bytes(rng, c)
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
        sends[c] = (seq_s[c], 0xDEAD, 0xBEEF, S + c, 23, 0, 0)  # first_frame / n_frames: the relay's, or unused
    d_sends = dev(sends)
    runs_e = t.zeros(2 * S, dtype=t.int32, device="cuda")
    runs_r = t.zeros(2 * S, dtype=t.int32, device="cuda")
    runs_c = t.zeros(2 * S, dtype=t.int32, device="cuda")
    fan = max(room.count(r) for r in range(R)) if relay else 1
    max_out_records = fan * (max_echoes + echo_cap // 16384 + 1) + max_replies + S
    sealed = t.zeros(fan * echo_cap + reply_cap + close_cap + max_out_records * 64, dtype=t.uint8, device="cuda")
    d_room = dev(np.array(room, np.uint32))

    eng_t.seal_records(d_src, dev(seal), len(seal), d_keys, len(keys), cipher[:out_pos])
    tls_dev = dev(tls_st)
    recs, res = eng_t.open_records(cipher, d_keys, len(keys), tls_dev, S, max_records, plain_out[:plain_cap],
                                   wire_len=out_pos)
    eng_t.ws_streams(res, recs, S, tls_dev, plain_out, ws_dev, read_end)
    desc, wres = eng_w.decode_streams(plain_out, ws_dev, S, max_frames, wire_len=plain_cap, read_end=read_end,
                                      n_reads=max_records)
    verdict, _ = eng_w.validate_utf8_streams(plain_out, desc, max_frames, ws_dev, wres, S, wire_len=plain_cap)
    _, r_off, r_conn, r_sum = eng_w.control_replies_streams(
        plain_out, desc, max_frames, ws_dev, wres, S, max_replies, reply_cap, out=arena[echo_cap:echo_cap + reply_cap],
        runs=runs_r, wire_len=plain_cap)
    if relay:
        _, e_off, _, e_conn, _, e_sum = eng_w.relay_messages_streams(
            plain_out, desc, max_frames, ws_dev, wres, S, d_room, R, max_echoes, echo_cap, out=arena[:echo_cap],
            recv_room=d_room, n_receivers=S, sends=d_sends[8:], send_stride=32, wire_len=plain_cap)
        first_runs, first_stride = d_sends[8:], 32
    else:
        _, e_off, _, e_conn, e_sum = eng_w.echo_messages_streams(
            plain_out, desc, max_frames, ws_dev, wres, S, max_echoes, echo_cap, out=arena[:echo_cap], runs=runs_e,
            wire_len=plain_cap)
        first_runs, first_stride = runs_e, 8
    _, c_off, c_conn, c_sum = eng_w.close_frames_streams(
        ws_dev, wres, S, close_cap, verdict=verdict, reply_conn=r_conn, out=arena[echo_cap + reply_cap:], runs=runs_c,
        clear_runs=[first_runs, runs_r] if clear else [], clear_stride=[first_stride, 8] if clear else [])
    parts = [(0, echo_cap, e_off, first_runs, first_stride, max_echoes),
             (echo_cap, reply_cap, r_off, runs_r, 8, max_replies),
             (echo_cap + reply_cap, close_cap, c_off, runs_c, 8, S)]
    _, sres, ssum = eng_t.seal_parts(arena, parts, d_sends, S, d_keys, len(keys), max_out_records, sealed)
    t.cuda.synchronize()  # the first host read

    # the passes' own outputs, as their tests pin them
    want_r = RR.expected_batch(plains, reads=reads, max_replies=max_replies)
    assert eng_w.read_reply_summary(r_sum) == want_r["summary"] and want_r["summary"]["n_replies"] >= 5
    assert eng_w.read_reply_conns(r_conn, S) == want_r["conn"]
    if relay:
        want_e = RL.expected(plains, room, R, room, reads=reads, max_frames_out=max_echoes)
        assert eng_w.read_relay_summary(e_sum) == want_e["summary"]
        lists = RL.room_lists(want_e)
        echo_bytes = [b"".join(lists[room[c]]) for c in range(S)]
    else:
        want_e = ER.expected_batch(plains, reads=reads, max_echoes=max_echoes)
        assert eng_w.read_echo_summary(e_sum) == want_e["summary"] and want_e["summary"]["n_echoes"] > 20
        echo_bytes = []
        for w in want_e["conn"]:
            lo = want_e["out_off"][w["first_echo"]]
            echo_bytes.append(want_e["out"][lo:lo + w["out_len"]])
    reply_bytes = []
    for w in want_r["conn"]:
        lo = want_r["out_off"][w["first_reply"]]
        reply_bytes.append(want_r["out"][lo:lo + w["out_len"]])
    # the close pass: the rule over the tables it read, and the scripted outcome
    h_res = wres.cpu().numpy()[:S * 64].view(RL.RESULT_DT)
    h_ver = verdict.cpu().numpy()[:S * 16].view(CR.VERDICT_DT)
    h_rep = r_conn.cpu().numpy()[:S * 16].view(CR.REPLY_CONN_DT)
    h_st = ws_dev.cpu().numpy().view(CR.STREAM_DT)
    want_c = CR.close_frames_ref(h_st, h_res, S, h_ver, h_rep, out_cap=close_cap)
    assert eng_w.read_close_conns(c_conn, S) == want_c["conn"]
    assert eng_w.read_close_summary(c_sum) == want_c["summary"]
    assert {c: w["code"] for c, w in enumerate(want_c["conn"]) if w["code"]} == CODES
    assert h_rep[PEER_CLOSE]["closed"] and h_rep[CLOSE_THEN_ERROR]["closed"] and h_res[CLOSE_THEN_ERROR]["first_status"] < 0
    close_bytes = [CR.close_frame(w["code"], 1) if w["code"] else b"" for w in want_c["conn"]]

    sr = sres.cpu().numpy()[:S * 48].view(TS.TLS_SEND_RESULT_DT)
    assert (sr["status"] == 0).all()
    host_sealed = sealed.cpu().numpy()
    open_st = np.zeros(S, O.TLS_STREAM_DT)
    for c in range(S):
        open_st[c] = (int(sr[c]["out_off"]), int(sr[c]["out_len"]), seq_s[c], S + c, 0)
    sm = ssum.cpu().numpy().view(TS.TLS_SEND_SUMMARY_DT)[0]
    total = int(sm["out_bytes"])
    assert int(sm["n_failed"]) == 0 and total == int(sr["out_len"].sum())
    o_recs, o_res, o_out = O.tls_open_batch(host_sealed[:max(1, total)], keys, open_st, out_cap=total + 16)
    for c in range(S):
        r = o_res[c]
        # every record of the send opens under seq, seq + 1, ...: one numbered send
        assert int(r["n_delivered"]) == int(sr[c]["n_records"]) and int(r["status"]) == 0, c
        assert int(sr[c]["next_seq"]) == seq_s[c] + int(sr[c]["n_records"])
        got = b"".join(o_out[rec["out_off"]:rec["out_off"] + rec["content_len"]].tobytes()
                       for rec in o_recs[r["first_record"]:r["first_record"] + r["n_delivered"]])
        if clear and CODES.get(c) == 1007:
            want = close_bytes[c]
        else:
            want = echo_bytes[c] + reply_bytes[c] + close_bytes[c]
        assert got == want, c
        assert int(sr[c]["plain_len"]) == len(want)
        if c in CODES:  # a failed connection's last frame is its CLOSE
            op, payload = _parse_unmasked(got)[-1]
            assert op == 8 and int.from_bytes(payload[:2], "big") == CODES[c]
    # (the cleared runs held something: without d_clear_runs those sends carry the echoes too)
    assert echo_bytes[INVALID_UTF8] and echo_bytes[INVALID_THEN_ERROR]
    eng_w.close()
    eng_t.close()
