"""The per-batch chain of a TLS echo server on the device with the answers as one run:
seal_records (the clients' messages) -> open_records -> ws_streams -> decode_reads ->
validate_utf8_streams -> fail_points -> answer_messages (d_reply_conn for close_frames) ->
close_frames (d_clear_runs = the answers' runs) -> seal_parts over TWO parts (answers, closes),
and seal_parts_coalesced over the same tables at max_fragment 16384 and 64.  24 connections with
keys of their own: a protocol error, invalid UTF-8 in a frame and in a fragment, PINGs between
messages and between fragments, a peer CLOSE followed by more frames, a bad close code, a short
CLOSE.

The oracle opens every connection's records under consecutive sequence numbers.  The plaintext is
exactly [the transcript's frames up to the fail point][the server's close, if any]: what
uvhttp_ws_send_frame would have been handed, in order.  A connection failed for invalid UTF-8 has
its run cleared and sends the close alone.  A PONG precedes the echo of a message that completes
after its PING: the order no arrangement of echo_messages and control_replies can give."""
import ctypes as C
import random

import numpy as np
import pytest

import _answer_ref as AR
import _close_ref as CR
import _fail_ref as F
import _oracle as O
import _tls_send_ref as TS
from test_gpu_echo import _parse_unmasked

pytestmark = pytest.mark.gpu

S = 24
INVALID, PROTOCOL_ERROR, PINGS, PEER_CLOSE, BAD_CODE, SHORT_CLOSE, INVALID_FRAGMENT = range(7)
# what the rule gives the scripted connections: (reason, the cut's frame in the connection, code)
WANT = {INVALID: (F.R_UTF8, 2, 1007), PROTOCOL_ERROR: (F.R_DECODE, 5, 1002), BAD_CODE: (F.R_CLOSE_CODE, 2, 1002),
        SHORT_CLOSE: (F.R_CLOSE_LEN, 1, 1002), INVALID_FRAGMENT: (F.R_UTF8, 2, 1007)}
CUTS = (0, 64)  # max_fragment of the two coalesced calls (0 = 16384)


@pytest.fixture(scope="module")
def torch():
    import torch as t
    if not t.cuda.is_available():
        pytest.skip("no GPU")
    return t


def _frames(rng, c):
    T, B, K, P, CL = AR.text, AR.binary, AR.cont, AR.ping, AR.close
    rsv = AR.Fr(1, 1, b"rsv", rsv=True)
    if c == INVALID:
        return [T(b"fine"), P(b"before the cut"), T(b"\xff\xfe evil"), P(b"after the cut"), T(b"later")]
    if c == PROTOCOL_ERROR:
        return [P(b"a"), T(b"before"), B(rng.randbytes(300), 0), P(b"mid"), K(rng.randbytes(40)), rsv, T(b"after")]
    if c == PINGS:
        return [T(b"m1"), P(b"between"), T(b"frag", 0), P(b"inside"), K(b"ment", 0), P(), K(b"s"), P(b"tail"), B(b"m3")]
    if c == PEER_CLOSE:
        return [T(b"bye"), P(b"still here"), CL(F.code(1000, b"done")), P(b"late"), T(b"unheard")]
    if c == BAD_CODE:
        return [P(b"p"), T(b"hi four"), CL(F.code(1005, b"x")), T(b"post")]
    if c == SHORT_CLOSE:
        return [P(b"p5"), CL(b"\x03"), P(b"late")]
    if c == INVALID_FRAGMENT:
        return [P(b"early"), T(b"six ", 0), K(b"\xff evil", 0), P(b"never"), K(b" end"), T(b"more")]
    ascii_ = lambda n: bytes(rng.choice(b"abcdefghij klmnop") for _ in range(n))  # noqa: E731
    rows = [(2, rng.randbytes(rng.choice([0, 1, 20, 200, 3000]))) if rng.random() < 0.5 else
            (1, ascii_(rng.choice([0, 1, 20, 200]))) for _ in range(rng.randint(0, 4))]
    fr = [f if f.op != 9 else P(rng.randbytes(rng.choice([0, 5, 125]))) for f in AR.ER.FR.fragment_randomly(rng, rows, 0.6)]
    for _ in range(rng.randint(0, 2)):
        fr.insert(rng.randrange(len(fr) + 1), P(rng.randbytes(rng.choice([0, 9]))))
    return fr


def _open(keys, seq_s, sres, ssum, sealed):
    """the oracle's open of every connection's records -> (plaintext per connection, send results)"""
    sr = sres.cpu().numpy()[:S * 48].view(TS.TLS_SEND_RESULT_DT)
    assert (sr["status"] == 0).all()
    open_st = np.zeros(S, O.TLS_STREAM_DT)
    for c in range(S):
        open_st[c] = (int(sr[c]["out_off"]), int(sr[c]["out_len"]), seq_s[c], S + c, 0)
    total = int(ssum.cpu().numpy().view(TS.TLS_SEND_SUMMARY_DT)[0]["out_bytes"])
    o_recs, o_res, o_out = O.tls_open_batch(sealed.cpu().numpy()[:max(1, total)], keys, open_st, out_cap=total + 16)
    got = []
    for c in range(S):
        r = o_res[c]
        assert int(r["n_delivered"]) == int(sr[c]["n_records"]) and int(r["status"]) == 0, c
        got.append(b"".join(o_out[rec["out_off"]:rec["out_off"] + rec["content_len"]].tobytes()
                            for rec in o_recs[r["first_record"]:r["first_record"] + r["n_delivered"]]))
    return got, sr.copy()


@pytest.fixture(scope="module")
def chain(torch):
    """one batch through the whole chain -> dict of everything the tests read"""
    import uvhttp_amd as U
    t = torch
    rng = random.Random(419)
    kinds = [TS.KEY_KINDS[rng.randrange(6)] for _ in range(S)]
    keys = np.concatenate([TS.make_key(rng, k) for k in kinds] + [TS.make_key(rng, k) for k in kinds])
    conns, plains, recs_rows, tls_st, reads = [], [], [], np.zeros(S, O.TLS_STREAM_DT), []
    src_pos, out_pos = 0, 0
    for c in range(S):
        conns.append(_frames(rng, c))
        plain = AR.raw(conns[c])
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
        conn = U.WsConnection(1, AR.MF, AR.MM)
        U.lib().uvhttp_ws_stream_init(conn.ptr, 0, 0, C.byref(s))
        ws.append(bytes(s))
    ws_dev = dev(np.frombuffer(b"".join(ws), np.uint8))
    read_end = t.zeros(max_records, dtype=t.int64, device="cuda")
    max_frames = max_answers = 512
    ans_cap = (src_pos + 14 * max_answers + 15) // 16 * 16
    close_cap = 32 * S
    arena = t.full((ans_cap + close_cap,), 0xEE, dtype=t.uint8, device="cuda")
    sends = np.zeros(S, TS.TLS_SEND_DT)
    seq_s = [rng.randrange(1 << 40) for _ in range(S)]
    for c in range(S):
        sends[c] = (seq_s[c], 0xDEAD, 0xBEEF, S + c, 23, 0, 0)
    d_sends = dev(sends)
    runs_a = t.zeros(2 * S, dtype=t.int32, device="cuda")
    runs_c = t.zeros(2 * S, dtype=t.int32, device="cuda")
    reply_conn = t.zeros(16 * S, dtype=t.uint8, device="cuda")
    max_out_records = max_answers + ans_cap // 64 + 1 + 2 * S
    out_bytes = ans_cap + close_cap + max_out_records * 64

    eng_t.seal_records(d_src, dev(seal), len(seal), d_keys, len(keys), cipher[:out_pos])
    tls_dev = dev(tls_st)
    recs, res = eng_t.open_records(cipher, d_keys, len(keys), tls_dev, S, max_records, plain_out[:plain_cap],
                                   wire_len=out_pos)
    eng_t.ws_streams(res, recs, S, tls_dev, plain_out, ws_dev, read_end)
    desc, wres = eng_w.decode_streams(plain_out, ws_dev, S, max_frames, wire_len=plain_cap, read_end=read_end,
                                      n_reads=max_records)
    verdict, _ = eng_w.validate_utf8_streams(plain_out, desc, max_frames, ws_dev, wres, S, flags=U.UTF8_CHECK_CLOSE,
                                             wire_len=plain_cap)
    wres, verdict, fail, _ = eng_w.fail_points_streams(plain_out, desc, max_frames, wres, S, verdict,
                                                       flags=U.FAIL_CHECK_CLOSE, wire_len=plain_cap)
    _, a_off, _, a_conn, a_sum = eng_w.answer_messages_streams(
        plain_out, desc, max_frames, ws_dev, wres, S, max_answers, ans_cap, out=arena[:ans_cap], runs=runs_a,
        reply_conn=reply_conn, wire_len=plain_cap)
    _, c_off, c_conn, _ = eng_w.close_frames_streams(
        ws_dev, wres, S, close_cap, verdict=verdict, reply_conn=reply_conn, out=arena[ans_cap:], runs=runs_c,
        clear_runs=[runs_a], clear_stride=[8])
    parts = [(0, ans_cap, a_off, runs_a, 8, max_answers), (ans_cap, close_cap, c_off, runs_c, 8, S)]
    sealed = t.zeros(out_bytes, dtype=t.uint8, device="cuda")
    _, sres, ssum = eng_t.seal_parts(arena, parts, d_sends, S, d_keys, len(keys), max_out_records, sealed)
    packed = {}
    for mf in CUTS:   # the same arena, tables and sends: only the last call of the chain differs
        out = t.zeros(out_bytes, dtype=t.uint8, device="cuda")
        _, cres, csum = eng_t.seal_parts_coalesced(arena, parts, d_sends, S, d_keys, len(keys), max_out_records, out,
                                                   max_fragment=mf)
        packed[mf] = (out, cres, csum)
    t.cuda.synchronize()  # the first host read

    r = {"conns": conns, "reads": reads, "keys": keys,
         "per_frame": _open(keys, seq_s, sres, ssum, sealed),
         "coalesced": {mf: _open(keys, seq_s, cres, csum, out) for mf, (out, cres, csum) in packed.items()},
         "codes": [c["code"] for c in eng_w.read_close_conns(c_conn, S)],
         "fails": eng_w.read_fail_conns(fail, S),
         "answers": eng_w.read_answer_conns(a_conn, S), "summary": eng_w.read_answer_summary(a_sum),
         "replies": eng_w.read_reply_conns(reply_conn, S),
         "first": [x.first_frame for x in eng_w.read_stream_results(wres, S)]}
    eng_w.close()
    eng_t.close()
    return r


def _expected(chain):
    """per connection: [the transcript's frames up to the fail point][the server's close]; a
    connection failed for invalid UTF-8 sends the close alone"""
    conns, reads, fails, first = chain["conns"], chain["reads"], chain["fails"], chain["first"]
    cut = [AR.raw(f[:fl["frame"] - first[c]]) if fl["reason"] >= F.R_UTF8 else AR.raw(f)
           for c, (f, fl) in enumerate(zip(conns, fails))]
    rd = [None if fails[c]["reason"] >= F.R_UTF8 else reads[c] for c in range(S)]
    want = AR.expected_batch(cut, reads=rd)
    out = []
    for c, w in enumerate(want["conn"]):
        lo = want["out_off"][w["first_answer"]]
        run = want["out"][lo:lo + w["out_len"]]
        close = CR.close_frame(fails[c]["code"], 1) if fails[c]["code"] else b""
        out.append(close if fails[c]["code"] == 1007 else run + close)
    return out, want


def test_fail_points_and_closes_are_the_rule(chain):
    fails, first = chain["fails"], chain["first"]
    for c in range(S):
        reason, rel, code = WANT.get(c, (F.R_NONE, None, 0))
        assert (fails[c]["reason"], fails[c]["code"], fails[c]["status"]) == (reason, code, F.OK), c
        assert fails[c]["frame"] == (F.NONE if reason == F.R_NONE else first[c] + rel), c
    assert chain["codes"] == [f["code"] for f in fails]
    assert chain["replies"][PEER_CLOSE]["closed"] == 1 and chain["codes"][PEER_CLOSE] == 0


def test_answer_tables_are_the_transcripts(chain):
    """d_conn, d_reply_conn and the summary before close_frames clears a run: the transcript of
    every connection up to its fail point"""
    _, want = _expected(chain)
    assert chain["answers"] == want["conn"] and chain["replies"] == want["reply"]
    assert chain["summary"] == want["summary"] and want["summary"]["n_replies"] > 20


def test_plaintext_is_what_send_frame_was_handed(chain):
    want, _ = _expected(chain)
    got, _ = chain["per_frame"]
    for c in range(S):
        assert got[c] == want[c], c
    # a failed connection's last frame is its CLOSE; a cleared 1007 connection sends the close alone
    for c, (_, _, code) in WANT.items():
        frames = _parse_unmasked(got[c])
        assert frames[-1][0] == 8 and frames[-1][1][:2] == code.to_bytes(2, "big"), c
        assert (len(frames) == 1) == (code == 1007), c
    # a peer CLOSE is echoed where it stood, nothing after it is answered, and no server close follows
    assert _parse_unmasked(got[PEER_CLOSE]) == [(1, b"bye"), (10, b"still here"), (8, F.code(1000, b"done"))]
    # a bad CLOSE is not echoed, a short one neither; the PINGs before them are answered
    assert _parse_unmasked(got[BAD_CODE]) == [(10, b"p"), (1, b"hi four"), (8, F.code(1002, b"protocol error"))]
    assert _parse_unmasked(got[SHORT_CLOSE]) == [(10, b"p5"), (8, F.code(1002, b"protocol error"))]
    assert [op for op, _ in _parse_unmasked(got[PROTOCOL_ERROR])] == [10, 1, 10, 2, 8]


def test_a_pong_precedes_a_later_echo(chain):
    """the ordering no arrangement of echo_messages and control_replies can give: a connection's
    run is neither all echoes then all replies nor the other way round"""
    got, _ = chain["per_frame"]
    assert _parse_unmasked(got[PINGS]) == [(1, b"m1"), (10, b"between"), (10, b"inside"), (10, b""), (1, b"fragments"),
                                           (10, b"tail"), (2, b"m3")]
    mixed = 0
    for c in range(S):
        ops = [op >= 8 for op, _ in _parse_unmasked(got[c])]
        mixed += ops != sorted(ops) and ops != sorted(ops, reverse=True)
    assert mixed >= 3  # the three scripted ones (PINGS, PROTOCOL_ERROR, BAD_CODE) at the least


@pytest.mark.parametrize("mf", CUTS)
def test_both_cuttings_carry_the_same_plaintext(chain, mf):
    (want, sr), keys = chain["per_frame"], chain["keys"]
    got, cr = chain["coalesced"][mf]
    cut = mf or 16384
    for c in range(S):
        assert got[c] == want[c], c
        assert int(cr[c]["plain_len"]) == len(want[c]) == int(sr[c]["plain_len"]), c
        assert int(cr[c]["n_records"]) == (len(want[c]) + cut - 1) // cut, c
        assert int(cr[c]["out_len"]) == len(want[c]) + int(cr[c]["n_records"]) * TS.overhead(keys[S + c]), c
