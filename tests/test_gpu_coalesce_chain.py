"""The per-batch chain of a TLS echo or room server on the device with the fail points
(tests/test_gpu_fail_chain.py: seal_records (the clients' messages) -> open_records -> ws_streams ->
decode_reads -> validate_utf8_streams -> fail_points -> control_replies -> echo (or relay) ->
close_frames), closed once by seal_parts and, over the same arena and run tables, by
seal_parts_coalesced at max_fragment 16384 and 64.  24 connections with keys of their own.

For every connection the plaintext the oracle opens is the same under both cuttings, the coalesced
call has ceil(B / max_fragment) records where seal_parts has at least one per frame, and a failed
connection's stream still ends with the server's close frame."""
import ctypes as C
import random

import numpy as np
import pytest

import _close_ref as CR
import _echo_ref as ER
import _oracle as O
import _tls_send_ref as TS
from test_gpu_fail_chain import R, ROOM, S, WANT, _frames

pytestmark = pytest.mark.gpu

CUTS = (0, 64)  # max_fragment of the two coalesced calls (0 = 16384)


@pytest.fixture(scope="module")
def torch():
    import torch as t
    if not t.cuda.is_available():
        pytest.skip("no GPU")
    return t


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


def _chain(torch, relay):
    """one batch through the whole chain -> (seal_parts' plaintext and results, the coalesced calls'
    per max_fragment, the close codes)"""
    import uvhttp_amd as U
    t = torch
    rng = random.Random(417)
    kinds = [TS.KEY_KINDS[rng.randrange(6)] for _ in range(S)]
    keys = np.concatenate([TS.make_key(rng, k) for k in kinds] + [TS.make_key(rng, k) for k in kinds])
    plains, recs_rows, tls_st = [], [], np.zeros(S, O.TLS_STREAM_DT)
    src_pos, out_pos = 0, 0
    for c in range(S):
        plain = ER.raw(_frames(rng, c))
        seq0, begin, pos, j = rng.randrange(1 << 40), out_pos, 0, 0
        while pos < len(plain):
            n = min(len(plain) - pos, rng.choice([1, 7, 40, 500, 16384]))
            recs_rows.append((src_pos + pos, out_pos, seq0 + j, n, c, 23, 0))
            out_pos += n + TS.overhead(keys[c])
            pos += n
            j += 1
        tls_st[c] = (begin, out_pos - begin, seq0, c, 0)
        plains.append(plain)
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
    # records: per frame at most its ceil, coalesced at 64 bytes at most bytes / 64 + 1 per connection
    max_out_records = fan * (max_echoes + echo_cap // 64 + 1) + max_replies + reply_cap // 64 + 2 * S
    out_bytes = fan * echo_cap + reply_cap + close_cap + max_out_records * 64
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
    sealed = t.zeros(out_bytes, dtype=t.uint8, device="cuda")
    _, sres, ssum = eng_t.seal_parts(arena, parts, d_sends, S, d_keys, len(keys), max_out_records, sealed)
    packed = {}
    for mf in CUTS:   # the same arena, tables and sends: only the last call of the chain differs
        out = t.zeros(out_bytes, dtype=t.uint8, device="cuda")
        _, cres, csum = eng_t.seal_parts_coalesced(arena, parts, d_sends, S, d_keys, len(keys), max_out_records, out,
                                                   max_fragment=mf)
        packed[mf] = (out, cres, csum)
    t.cuda.synchronize()  # the first host read

    per_frame = _open(keys, seq_s, sres, ssum, sealed)
    coalesced = {mf: _open(keys, seq_s, cres, csum, out) for mf, (out, cres, csum) in packed.items()}
    codes = [c["code"] for c in eng_w.read_close_conns(c_conn, S)]
    fails = eng_w.read_fail_conns(fail, S)
    eng_w.close()
    eng_t.close()
    return per_frame, coalesced, codes, fails, keys


@pytest.fixture(scope="module")
def runs(torch):
    return {relay: _chain(torch, relay) for relay in (False, True)}


@pytest.mark.parametrize("mf", CUTS)
@pytest.mark.parametrize("relay", [False, True])
def test_both_cuttings_carry_the_same_plaintext(runs, relay, mf):
    (want, sr), coalesced, _, _, keys = runs[relay]
    got, cr = coalesced[mf]
    cut = mf or 16384
    for c in range(S):
        assert got[c] == want[c], c
        assert int(cr[c]["plain_len"]) == len(want[c]) == int(sr[c]["plain_len"]), c
        assert int(cr[c]["n_records"]) == (len(want[c]) + cut - 1) // cut, c
        assert int(cr[c]["out_len"]) == len(want[c]) + int(cr[c]["n_records"]) * TS.overhead(keys[S + c]), c
    if not mf:  # seal_parts' own cut: never more records than one per frame, and several frames share one
        assert (cr["n_records"] <= sr["n_records"]).all()
        assert int(cr["n_records"].sum()) < int(sr["n_records"].sum())


@pytest.mark.parametrize("relay", [False, True])
def test_a_failed_connection_still_ends_with_its_close(runs, relay):
    _, coalesced, codes, fails, _ = runs[relay]
    assert sorted(c for c in range(S) if fails[c]["code"]) == sorted(WANT)
    for mf in CUTS:
        got, _ = coalesced[mf]
        for c, (_, _, code) in WANT.items():
            assert codes[c] == code and got[c].endswith(CR.close_frame(code, 1)), (c, mf)
